"""Saturated rows for the categorical head, sampler and loss kernels (csrc/elem.h: cat_dist / cat_logp / cat_pick / cat_loss_row),
shared by tests/test_cat_edges_cpu.py and tests/test_gpu_cat_edges.py. CPU only: nothing here launches a kernel.

tests/cat_cases.py keeps every probability of a batch in [1e-6, 0.99]. A discrete policy that has trained for a while leaves that
regime on most rows: logit gaps of 20 - 200, probabilities below fp32 eps, probabilities that are exactly 0 in fp32. The cases here
are cat_cases-style dicts with a larger `scale` (cc.sharpen), chosen on the CPU so that a batch holds rows of these kinds:
  (a) ordinary   every p_j >= 1e-6
  (b) sub-eps    some 0 < p_j < CLAMP_EPS (torch's fp32 eps, 2^-23: where Categorical(probs=...) starts to clamp)
  (c) zero       some p_j == 0 in fp32 (z_j - max below about -104: expf underflows past the smallest denormal)
  (d) fallback   the fp32 running sum of the probabilities ends at or below 1 - 2^-24, the largest uniform torch.rand returns: no
                 running sum exceeds that uniform and the sampler falls back (cat_pick)
  edge_mid   K=6  S=45 [128,64]/[72]  holds (a), (b), (d)
  edge_hard  the same net, a larger scale: (b), (c), (d), and (d) rows whose index K - 1 has p == 0 ("d0")
  edge_k16   the hard regime at the full head row
  edge_k2    the smallest distribution: K = 2 cannot hold a zero next to a partner that is not 1, so it is held to (b) and (d)
For every n >= 64 each required kind covers at least KIND_SHARE of the rows (tests/test_cat_edges_cpu.py asserts it from the fp32
and the float64 restatement at every n the GPU tests use; the GPU tests re-assert half of it on the engine's own logits).

How the scales were chosen (scanned on the CPU, smallest share over every n in use). One scale moves every gap of a batch
together: kind (d) needs two classes of comparable probability in a row (a one-hot row sums to exactly 1) and leaves the batch
as the scale grows — 28 % of the rows at 4000, 6 % at 18000, 1 - 4 % from 30000 on (K = 6) — while kind (c) needs a gap beyond
104 and only appears from 16000 on. So the hard scales sit where both hold, 18000 (K = 6) and 20000 (K = 16), and K = 2, which
needs a gap below 17.3 for (d) and above 15.9 for (b) in different rows, takes 5000. A row of kind (d) whose LAST class has
p == 0 — the row on which the sampler's old fall-back drew an impossible action — needs a small gap and a gap beyond 104 in one
row, which a scale alone yields on under 1 % of the rows; the hard cases therefore add `last_bias` = -150 to the last column's
bias (seeded_nets): a class the policy has given up, p[K - 1] == 0 in fp32 on every row, kind (c) elsewhere besides.

The reference of every comparison is float64 on the SAME fp32 logits (head64, loss64, pick64), so no gate depends on the compute
mode. No tolerance is a measured number: each gate is EPS32 = 2^-24 (the fp32 unit roundoff) times the magnitudes that enter the
quantity, derived next to the function that returns it (Gates). emulate32 restates the kernels' fp32 arithmetic in numpy, in
their operation order, so that the gates can be checked without a GPU: tests/test_cat_edges_cpu.py holds it to every gate.

The deviation that stays: Categorical(probs=softmax(z)) clamps the probabilities to [CLAMP_EPS, 1 - CLAMP_EPS] before it takes
their log, so the reference's log-prob of a class below CLAMP_EPS is log(2^-23) = -15.94 with a zero gradient. The kernels
compute the exact log-softmax (elem.h: "not reproduced"). The two coincide on rows of kind (a); everywhere else the tests pin
the kernels to the exact log-softmax."""
import functools

import numpy as np
import torch

import cat_cases as cc

EPS32 = 2.0 ** -24                                     # fp32 unit roundoff (tests/ppo_ref64.py)
CLAMP_EPS = float(torch.finfo(torch.float32).eps)      # 2^-23: Categorical's clamp_probs bound
U_MAX = np.float32(1.0 - 2.0 ** -24)                   # the largest value torch.rand returns (multiples of 2^-24)
TINY32 = 2.0 ** -126                                   # the smallest fp32 normal
BAND = 1e-6                                            # tests/test_gpu_cat.py::test_sample's boundary band
KIND_SHARE = 0.05
BAND_SHARE = 0.01
ENT_COEF = cc.ENTROPY_COEFF

_NET = dict(kind="mlp", S=45, A=1, enc=[128, 64], head=[72], B=64)
EDGE_CASES = {
    "edge_mid": dict(_NET, K=6, seed=200, scale=4000.0, last_bias=0.0),
    "edge_hard": dict(_NET, K=6, seed=200, scale=18000.0, last_bias=-150.0),
    "edge_k16": dict(_NET, K=16, seed=201, scale=20000.0, last_bias=-150.0),
    "edge_k2": dict(_NET, K=2, seed=202, scale=5000.0, last_bias=0.0),
}
# the kinds a case must hold (KIND_SHARE of the rows each, n >= 64); "d0": kind (d) rows whose p[K - 1] == 0
REQUIRED = {"edge_mid": ("a", "b", "d"), "edge_hard": ("b", "c", "d", "d0"), "edge_k16": ("b", "c", "d", "d0"),
            "edge_k2": ("b", "d")}
# batch sizes of tests/test_gpu_cat_edges.py::test_loss_stage_vs_float64: loss_block(n) goes from 256 to 1024 threads at n = 512,
# and each block's `i += blockDim.x` loop takes a second trip past 256 / 1024 rows
LOSS_NS = {"edge_hard": (2, 3, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2048), "edge_mid": (64, 513, 1025),
           "edge_k16": (64, 513, 1025), "edge_k2": (64, 513, 1025)}
HEAD_NS = (1, 255, 256, 257, 4097)       # cat_head_kernel: 256 rows per block, 4097 = 16 blocks + 1 row (the grid guard)
SAMPLE_NS = (1, 256, 257, 4097)
ROLLOUT_ES = (1, 65, 256, 257)           # act_finish_cat_kernel: one 256-thread block looping over E
POOL_N = 256                             # rows of a case the head / sampler / rollout tests draw from


def sized(case, n):
    return dict(case, B=int(n))


# ------------------------------------------------------------------------------------------ float64 reference
def head64(logits, acts=None):
    """fp32 logits [n, K] -> float64 dict: t = z - max, s = sum exp(t), ls = log s, lg = log p (t - ls), p, H = -sum p log p
    (0 log 0 = 0), and lp = log p of the indices acts [n] (None without)."""
    z = np.asarray(logits, dtype=np.float32).astype(np.float64)
    t = z - z.max(axis=1, keepdims=True)
    e = np.exp(t)
    s = e.sum(axis=1)
    ls = np.log(s)
    lg = t - ls[:, None]
    p = e / s[:, None]
    with np.errstate(invalid="ignore"):
        H = -np.where(p > 0, p * lg, 0.0).sum(axis=1)
    lp = None if acts is None else lg[np.arange(len(z)), np.asarray(acts, dtype=np.int64)]
    return dict(t=t, e=e, s=s, ls=ls, lg=lg, p=p, H=H, lp=lp)


def adv_norm64(advs):
    """-> (an, mean, Bessel std) in float64: (a - a.mean()) / (a.std() + 1e-5), torch's std, as cat_cases.CatOracle has it."""
    a = np.asarray(advs, dtype=np.float32).astype(np.float64).reshape(-1)
    mean = a.mean()
    std = np.sqrt(((a - mean) ** 2).sum() / (len(a) - 1))
    return (a - mean) / (std + 1e-5), mean, std


def loss64(logits, acts, advs, ent_coef=ENT_COEF, values=None, rets=None):
    """The loss stage of both learners in float64 on fp32 inputs: head64's fields plus an, dz — the kernel's documented gradient
    row (1 / n) (-an ([j == a] - p_j) + ent_coef p_j (log p_j + H)) — and the record scalars: `a2c` (A2C.update's keys; the critic's
    with values / rets given) and `rf` (Reinforce.update's; advs/std is numpy's population std there)."""
    h = head64(logits, acts)
    n, K = h["p"].shape
    an, amean, astd = adv_norm64(advs)
    hit = np.zeros((n, K))
    hit[np.arange(n), np.asarray(acts, dtype=np.int64)] = 1.0
    with np.errstate(invalid="ignore"):
        plg = np.where(h["p"] > 0, h["p"] * (h["lg"] + h["H"][:, None]), 0.0)
    dz = (-an[:, None] * (hit - h["p"]) + ent_coef * plg) / n
    lp = h["lp"]
    loss = np.mean(-lp * an) - ent_coef * h["H"].mean()
    a = np.asarray(advs, dtype=np.float32).astype(np.float64).reshape(-1)
    a2c = {"Training/policy_loss": loss, "ent": h["H"].mean(), "log_prob": lp.mean()}
    if values is not None:
        v = np.asarray(values, dtype=np.float64).reshape(-1)
        r = np.asarray(rets, dtype=np.float32).astype(np.float64).reshape(-1)
        a2c.update({"Training/vf_loss": np.mean((v - r) ** 2), "v_pred/mean": v.mean(), "v_pred/std": v.std(ddof=1),
                    "v_pred/max": v.max(), "v_pred/min": v.min()})
    rf = {"advs/mean": amean, "advs/std": a.std(), "advs/max": a.max(), "advs/min": a.min(), "Training/policy_loss": loss,
          "ent": h["H"].mean(), "logprob/mean": lp.mean(), "logprob/std": lp.std(ddof=1), "logprob/max": lp.max(),
          "logprob/min": lp.min()}
    return dict(h, an=an, amean=amean, astd=astd, hit=hit, dz=dz, a2c=a2c, rf=rf)


def pick64(probs32, u):
    """The sampler's reference: probs fp32 [n, K], u [n] -> (the first k whose float64 running sum of the fp32 probabilities
    exceeds u — if none does, the LAST k with p_k > 0, and K - 1 only for an all-zero row —, the distance of u to the nearest
    running sum). On rows whose probabilities are all positive this is cat_cases.inverse_cdf."""
    p = np.asarray(probs32, dtype=np.float32).astype(np.float64)
    c = np.cumsum(p, axis=1)
    u = np.asarray(u, dtype=np.float64).reshape(-1, 1)
    K = p.shape[1]
    first = (c <= u).sum(axis=1)
    pos = p > 0
    last = np.where(pos.any(axis=1), K - 1 - np.argmax(pos[:, ::-1], axis=1), K - 1)
    return np.where(first < K, first, last).astype(np.int64), np.abs(c - u).min(axis=1)


def pick_range(probs32, u, band=BAND):
    """-> (lo, hi): the picks of u - band and of u + band. A running sum in fp32 differs from the float64 one by at most
    (K - 1) EPS32 < band, so the kernel's index lies in [lo, hi] on every row, the boundary band included."""
    u = np.asarray(u, dtype=np.float64)
    return pick64(probs32, u - band)[0], pick64(probs32, u + band)[0]


# ------------------------------------------------------------------------------------------ fp32 emulation
def _seq_sum32(x):
    s = np.zeros(len(x), dtype=np.float32)
    run = np.empty_like(x)
    for j in range(x.shape[1]):
        s = (s + x[:, j]).astype(np.float32)
        run[:, j] = s
    return s, run


def dist32(logits):
    """cat_dist in fp32 numpy, in the kernel's operation order -> dict p, lg [n, K], ent [n], s [n] (all float32)."""
    z = np.asarray(logits, dtype=np.float32)
    with np.errstate(under="ignore"):
        t = (z - z.max(axis=1, keepdims=True)).astype(np.float32)
        e = np.exp(t).astype(np.float32)
        s, _ = _seq_sum32(e)
        ls = np.log(s).astype(np.float32)
        lg = (t - ls[:, None]).astype(np.float32)
        p = (e / s[:, None]).astype(np.float32)
        ent = np.zeros(len(z), dtype=np.float32)
        for j in range(z.shape[1]):
            ent = (ent - (p[:, j] * lg[:, j]).astype(np.float32)).astype(np.float32)
    return dict(p=p, lg=lg, ent=ent, s=s)


def pick32(probs32, u, fixed=True):
    """cat_pick in fp32 numpy: the first k whose fp32 running sum exceeds u; none: the last k with p_k > 0 (fixed=False: K - 1, the
    fall-back this arithmetic had before: kept to show what the crafted rows catch). u < 0: the first argmax."""
    p = np.asarray(probs32, dtype=np.float32)
    u = np.asarray(u, dtype=np.float32).reshape(-1)
    K = p.shape[1]
    _, run = _seq_sum32(p)
    over = run > u[:, None]
    first = np.where(over.any(axis=1), np.argmax(over, axis=1), K)
    pos = p > 0
    last = np.where(pos.any(axis=1), K - 1 - np.argmax(pos[:, ::-1], axis=1), K - 1) if fixed else np.full(len(p), K - 1)
    idx = np.where(first < K, first, last)
    return np.where(u < 0, np.argmax(p, axis=1), idx).astype(np.int64)


def emulate32(logits, acts=None, advs=None, ent_coef=ENT_COEF, u=None):
    """cat_dist / cat_logp / cat_pick / cat_loss_row in fp32 numpy -> dict: p, lg, ent, s; lp (acts given); idx (u given); an, dz
    and the record scalars a2c / rf (acts and advs given: fp32 rows, double sums, as the loss kernels reduce them)."""
    d = dist32(logits)
    n, K = d["p"].shape
    if acts is not None:
        acts = np.asarray(acts, dtype=np.int64)
        d["lp"] = d["lg"][np.arange(n), acts]
    if u is not None:
        d["idx"] = pick32(d["p"], u)
    if acts is None or advs is None:
        return d
    f = np.float32
    a = np.asarray(advs, dtype=np.float32).reshape(-1)
    _, amean, astd = adv_norm64(a)               # adv_stats_body: double sums, rounded once
    an = ((a - f(amean)).astype(f) / (f(astd) + f(1e-5))).astype(f)
    hit = np.zeros((n, K), dtype=f)
    hit[np.arange(n), acts] = 1.0
    inv_n, ec = f(1.0) / f(n), f(ent_coef)
    pg = ((-an[:, None] * (hit - d["p"]).astype(f)).astype(f)
          + ((ec * d["p"]).astype(f) * (d["lg"] + d["ent"][:, None]).astype(f)).astype(f)).astype(f)
    d["an"], d["dz"] = an, (inv_n * pg).astype(f)
    lp = d["lp"]
    s_loss = (-lp * an).astype(f).astype(np.float64).sum()
    lp64, ent64 = lp.astype(np.float64), d["ent"].astype(np.float64)
    loss = f(s_loss / n - float(ec) * (ent64.sum() / n))
    lpm = lp64.sum() / n
    lps = np.sqrt(max(0.0, ((lp64 ** 2).sum() - n * lpm * lpm) / (n - 1.0)))
    a64 = a.astype(np.float64)
    d["a2c"] = {"Training/policy_loss": loss, "ent": f(ent64.sum() / n), "log_prob": f(lpm)}
    d["rf"] = {"advs/mean": f(amean), "advs/std": f(np.sqrt(float(f(((a64 - amean) ** 2).sum())) / n)), "advs/max": a.max(),
               "advs/min": a.min(), "Training/policy_loss": loss, "ent": f(ent64.sum() / n), "logprob/mean": f(lpm),
               "logprob/std": f(lps), "logprob/max": lp.max(), "logprob/min": lp.min()}
    return d


# ------------------------------------------------------------------------------------------ gates
# Every gate bounds the fp32 rounding of one quantity of cat_dist, given the float64 fields of head64 on the same logits. With
# u = EPS32, a correctly rounded fp32 operation has a relative error <= u, and:
#   t_j = z_j - max                   one subtraction: |dt_j| <= u |t_j|
#   e_j = expf(t_j)                   a library expf within 2 ulp = C_FN u; the error of its argument becomes a relative one of
#                                     |dt_j|:                                      rel(e_j) <= u (|t_j| + C_FN)
#   s = e_0 + .. + e_15               K positive terms added in order, K - 1 roundings: rel(s) <= sum_j e_j rel(e_j) / s + (K - 1) u;
#                                     e_j |t_j| = |t_j| exp(-|t_j|) <= 1 / e = 0.37 for the K - 1 terms with t_j != 0 and
#                                     s >= 1:                                      rel(s) <= u (C_FN + 1.37 (K - 1))
#   ls = logf(s)                      |d ls| <= rel(s) + C_FN u |ls|
#   lg_j = (t_j) - ls                 |d lg_j| <= |dt_j| + |d ls| + u |lg_j| <= u (2 |t_j| + (1 + C_FN) |ls| + C_FN + 1.37 (K - 1))
#                                     <= C_LG(K) u (|t_j| + |ls| + 1)     with  C_LG(K) = max(1 + C_FN, C_FN + 1.37 (K - 1))
#   p_j = e_j / s                     rel(p_j) <= rel(e_j) + rel(s) + u <= u (|t_j| + C_P(K)),  C_P(K) = 2 C_FN + 1 + 1.37 (K - 1);
#                                     plus TINY32 absolute: an expf or a quotient below the smallest normal may be flushed to 0
#                                     or keep fewer bits
#   H = -sum_j p_j lg_j               per term p_j |d lg_j| + |lg_j| |d p_j| + u p_j |lg_j| (the product), plus K - 1 roundings
#                                     of the running sum, each <= u sum_j p_j |lg_j|
C_FN = 4.0   # expf / logf within 2 ulp; 1 ulp = 2 u


def c_lg(K):
    return max(1.0 + C_FN, C_FN + 1.37 * (K - 1))


def c_p(K):
    return 2.0 * C_FN + 1.0 + 1.37 * (K - 1)


def head_gates(h):
    """head64's dict -> absolute bounds dict lg, p [n, K], H [n]."""
    K = h["p"].shape[1]
    at = np.abs(h["t"])
    g_lg = c_lg(K) * EPS32 * (at + np.abs(h["ls"])[:, None] + 1.0)
    g_p = EPS32 * (at + c_p(K)) * h["p"] + TINY32
    plg = h["p"] * np.abs(h["lg"])
    g_H = (h["p"] * g_lg + np.abs(h["lg"]) * g_p + EPS32 * plg).sum(axis=1) + (K - 1) * EPS32 * plg.sum(axis=1)
    return dict(lg=g_lg, p=g_p, H=g_H)


def loss_gates(R, advs, ent_coef=ENT_COEF, values=None, rets=None):
    """loss64's dict -> bounds: dz [n, K], rowsum [n], and per record key for `a2c` and `rf`.
    an = (a - mean) / (std + 1e-5): a difference of two ~4.0's over a std of 0.05 — e_an = 8 u (|a| + |mean|) / std, the bound
    tests/test_gpu_loss_adam.py uses for the same expression.
    dz_j = inv_n (A_j + B_j), A_j = -an (hit - p_j), B_j = ent_coef p_j (lg_j + H):
      |dA_j| <= |hit - p_j| e_an + |an| |dp_j| + 2 u |A_j|                   (hit - p_j: |dp_j| plus one rounding; the product)
      |dB_j| <= ent_coef (|dp_j| |lg_j + H| + p_j (|d lg_j| + |dH|)) + 3 u |B_j|  (the sum lg_j + H and two products)
      the sum A_j + B_j, inv_n = 1 / n in fp32 and the product with it: 3 u (|A_j| + |B_j|)
    A row sums to 0 exactly; what the kernel's row sums to is bounded by the sum of its elements' bounds."""
    g = head_gates(R)
    n, K = R["p"].shape
    a = np.abs(np.asarray(advs, dtype=np.float64).reshape(-1))
    e_an = 8 * EPS32 * (a + abs(R["amean"])) / R["astd"]
    an = np.abs(R["an"])
    A = an[:, None] * np.abs(R["hit"] - R["p"])
    lgH = np.abs(R["lg"] + R["H"][:, None])
    B = ent_coef * R["p"] * lgH
    dA = np.abs(R["hit"] - R["p"]) * e_an[:, None] + an[:, None] * g["p"] + 2 * EPS32 * A
    dB = ent_coef * (g["p"] * lgH + R["p"] * (g["lg"] + g["H"][:, None])) + 3 * EPS32 * B
    g_dz = (dA + dB + 3 * EPS32 * (A + B)) / n + 1e-30
    e_lp = g["lg"][R["hit"] > 0]
    lp = np.abs(R["lp"])
    # policy_loss = mean(-lp an) - ent_coef mean(H): fp32 products, double sums, one rounding of the result (as
    # test_gpu_loss_adam gates policy_loss: the rows' own errors plus 8 u of the magnitudes)
    g_loss = np.mean(an * e_lp + lp * e_an) + ent_coef * np.mean(g["H"]) + 8 * EPS32 * (np.mean(lp * an) + ent_coef * np.mean(R["H"]))
    g_ent = np.mean(g["H"]) + 2 * EPS32 * abs(R["H"].mean()) + 1e-30
    g_lpm = np.mean(e_lp) + 2 * EPS32 * abs(R["lp"].mean())
    amean, astd = abs(R["amean"]), R["astd"]
    g_astd = 8 * EPS32 * astd + 4 * EPS32 * amean / np.sqrt(n)     # test_gpu_loss_adam's advs/std
    a2c = {"Training/policy_loss": g_loss, "ent": g_ent, "log_prob": g_lpm}
    if values is not None:
        v = np.abs(np.asarray(values, dtype=np.float64).reshape(-1))
        r = np.abs(np.asarray(rets, dtype=np.float64).reshape(-1))
        d = v + r
        diff = np.abs(np.asarray(values, dtype=np.float64).reshape(-1) - np.asarray(rets, dtype=np.float64).reshape(-1))
        # vf_loss as test_gpu_loss_adam gates it; v_pred/*: double sums of fp32 values, rounded once
        a2c.update({"Training/vf_loss": 8 * EPS32 * np.mean(d * (d + diff)) + 1e-30, "v_pred/mean": 2 * EPS32 * np.mean(v) + 1e-30,
                    "v_pred/std": 2 * EPS32 * (R["a2c"]["v_pred/std"] + np.mean(v) / np.sqrt(n)) + 1e-30,
                    "v_pred/max": 0.0, "v_pred/min": 0.0})
    rf = {"advs/mean": 2 * EPS32 * amean, "advs/std": g_astd, "advs/max": 0.0, "advs/min": 0.0, "Training/policy_loss": g_loss,
          "ent": g_ent, "logprob/mean": g_lpm, "logprob/std": 2 * np.max(e_lp) + 4 * EPS32 * R["rf"]["logprob/std"],
          "logprob/max": np.max(e_lp), "logprob/min": np.max(e_lp)}
    return dict(dz=g_dz, rowsum=g_dz.sum(axis=1), a2c=a2c, rf=rf, e_an=e_an, bessel_std=g_astd)


def ratio(err, bound):
    """max of err / bound; an element with err == 0 passes whatever its bound."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300)).max())


def head_ratios(got_p, got_lg, got_ent, h):
    """error / gate of probabilities [n, K], log-probabilities [n, K] (None: not compared) and entropies [n] against head64's h."""
    g = head_gates(h)
    out = {"p": ratio(np.abs(np.asarray(got_p, dtype=np.float64) - h["p"]), g["p"]),
           "ent": ratio(np.abs(np.asarray(got_ent, dtype=np.float64) - h["H"]), g["H"])}
    if got_lg is not None:
        out["logp"] = ratio(np.abs(np.asarray(got_lg, dtype=np.float64) - h["lg"]), g["lg"])
    return out


# ------------------------------------------------------------------------------------------ row kinds
def row_kinds(logits):
    """fp32 logits -> dict of boolean [n] masks a, b, c, d, d0 (module docstring), from dist32 (p, the running sum) and head64."""
    d = dist32(logits)
    p = d["p"]
    h = head64(logits)
    _, run = _seq_sum32(p)
    dk = run[:, -1] <= U_MAX
    return {"a": (h["p"] >= 1e-6).all(axis=1) & (p >= 1e-6).all(axis=1),
            "b": ((p > 0) & (p < CLAMP_EPS)).any(axis=1) & ((h["p"] > 0) & (h["p"] < CLAMP_EPS)).any(axis=1),
            "c": (p == 0).any(axis=1), "d": dk, "d0": dk & (p[:, -1] == 0)}


def kind_counts(logits):
    return {k: int(v.sum()) for k, v in row_kinds(logits).items()}


def need(n, share=KIND_SHARE):
    """Rows of a required kind a batch of n >= 64 rows must hold (none is required of a smaller one)."""
    return int(np.ceil(share * n)) if n >= 64 else 0


def check_kinds(name, logits, share=KIND_SHARE):
    """Assert REQUIRED[name] on a batch's logits -> the counts."""
    got = kind_counts(logits)
    n = len(logits)
    for k in REQUIRED[name]:
        assert got[k] >= need(n, share), (name, n, k, got)
    return got


# ------------------------------------------------------------------------------------------ inputs
def make_acts(case, logits, update=0):
    """int64 [n] action indices on a batch's logits: half the float64 argmax, a quarter the float64 argmin (so stored actions
    of probability < CLAMP_EPS and exactly 0 occur), the rest uniform, in a seeded order; where n >= K the first K of the
    uniform (then argmax) positions hold 0 .. K - 1, so every index is present."""
    z = np.asarray(logits, dtype=np.float64)
    n, K = z.shape
    rs = np.random.RandomState(1000 * case["seed"] + 931 + update)
    perm = rs.permutation(n)
    top, low = perm[:n // 2], perm[n // 2:n // 2 + n // 4]
    rest = perm[n // 2 + n // 4:]
    acts = rs.randint(0, K, size=n)
    acts[top], acts[low] = z[top].argmax(axis=1), z[low].argmin(axis=1)
    if n >= K:
        acts[np.concatenate([rest, top])[:K]] = np.arange(K)
    return acts.astype(np.int64)


def make_advs(case, n, update=0):
    """4.0 + 0.05 randn: tests/test_gpu_loss_adam.py's large-mean batch (the normalisation subtracts two ~4.0's)."""
    rs = np.random.RandomState(1000 * case["seed"] + 947 + update + 7 * n)
    return (4.0 + 0.05 * rs.randn(n)).astype(np.float32)


def seeded_nets(networks, policies, case):
    """cc.seeded_nets (the head's last weight times `scale`), then `last_bias` added to the last column's bias: a class the
    policy has given up, p[K - 1] == 0 in fp32 on every row of the hard cases."""
    pf, vf = cc.seeded_nets(networks, policies, case)
    keys = [k for k in pf.state_dict() if k.startswith("seq_append_fcs.") and k.endswith(".bias")]
    with torch.no_grad():
        pf.state_dict()[keys[-1]][-1] += case["last_bias"]
    return pf, vf


@functools.lru_cache(maxsize=None)
def _oracle(name, f64=False):
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    case = EDGE_CASES[name]
    pf, vf = seeded_nets(networks, policies, case)
    return cc.fresh_a2c_oracle(case, dtype=torch.float64 if f64 else torch.float32, init=(pf.state_dict(), vf.state_dict()))


def logits_of(name, obs, dtype=torch.float32):
    """The restatement's logits (orc.FORWARDS through the case's oracle) of observation rows, fp32 or float64 -> numpy."""
    o = _oracle(name, dtype == torch.float64)
    with torch.no_grad():
        return o.fwd(o.pf, torch.as_tensor(obs).to(dtype), o.S, o.mode).numpy()


@functools.lru_cache(maxsize=None)
def batch(name, n):
    """The inputs of a loss evaluation at n rows, chosen on the CPU: obs fp32 [n, S], the fp32 and float64 restatement's logits,
    acts (make_acts on the float64 logits), advs (make_advs), estimate_returns. Cached: shared, not to be written to."""
    case = sized(EDGE_CASES[name], n)
    b = cc.host_batch(case, 0)
    obs = np.asarray(b["obs"], dtype=np.float32)
    z32, z64 = logits_of(name, obs), logits_of(name, obs, torch.float64)
    return dict(obs=obs, logits32=z32, logits64=z64, acts=make_acts(case, z64), advs=make_advs(case, n),
                rets=np.asarray(b["estimate_returns"], dtype=np.float32).reshape(n))


def acts_kinds(logits, acts):
    """-> (stored actions with 0 < p < CLAMP_EPS, stored actions with p == 0) in dist32's fp32 probabilities."""
    p = dist32(logits)["p"][np.arange(len(acts)), acts]
    return int(((p > 0) & (p < CLAMP_EPS)).sum()), int((p == 0).sum())


# ------------------------------------------------------------------------------------------ crafted rows
def crafted_logits(K):
    """Hand-built logits rows [m, K]: gaps of 0, 16, 17 (exp(-16) straddles CLAMP_EPS), 88 (below the smallest normal), 104
    (below the smallest denormal), 200 and 1e4 between the first column and the rest; the same with the maximum in the last
    column; exact ties of two and of all maxima over a far tail; a large common offset; a descending staircase."""
    rows = []
    for gap in (0.0, 16.0, 17.0, 88.0, 104.0, 200.0, 1e4):
        r = np.full(K, -gap)
        r[0] = 0.0
        rows.append(r)
        r = np.full(K, 3.0 - gap)
        r[-1] = 3.0
        rows.append(r)
        r = np.full(K, -gap)
        r[0] = r[K // 2] = 0.0            # two exact maxima (K = 2: both columns)
        rows.append(r)
    rows.append(np.full(K, 7.5))          # all tied
    rows.append(1e4 + 2.0 * np.arange(K))   # a large common offset: the subtraction of the maximum is exact
    rows.append(-20.0 * np.arange(K))     # p_j falls by exp(-20) per column: sub-eps from j = 1, zero from j = 6
    rows.append(-20.0 * np.arange(K)[::-1] + 1e3)
    return np.asarray(rows, dtype=np.float32)


def crafted_probs(K):
    """Hand-built probability rows for the sampler -> (probs fp32 [m, K], u fp32 [m], the right index [m]); exact in fp32, so the
    kernel's index is compared with `want` on every row, boundary or not.
      - [1/4, 1/4, 1/4, 1/4 - 2^-24, 0 ...] at u = 1 - 2^-24: the running sum ends AT u; the pick is 3, the last positive class,
        not K - 1 (K >= 6; with trailing zeros at K = 16)
      - [1, 0 .. 0] at u = 0, 0.5 and 1 - 2^-24: 0
      - [1/2, 1/2 - 2^-24, 0 ...] (K = 2: no trailing zero) at u = 1 - 2^-24: 1
      - [0 .. 0, 1]: K - 1;  [0, 1/2, 0, 1/2 - 2^-24, 0 ..] (K >= 6) at u = 1 - 2^-24: 3;  an all-zero row: K - 1
      - u exactly on a boundary: [1/4, 1/4, 1/2] at u = 1/4 -> 1 (the first running sum that EXCEEDS u)"""
    z = lambda *head: np.asarray(list(head) + [0.0] * (K - len(head)), dtype=np.float64)
    q = 2.0 ** -24
    rows, us, want = [], [], []
    add = lambda r, u, w: (rows.append(r), us.append(u), want.append(w))
    if K >= 6:
        add(z(0.25, 0.25, 0.25, 0.25 - q), 1 - q, 3)
        add(z(0.25, 0.25, 0.25, 0.25 - q), 0.75, 3)
        add(z(0.0, 0.5, 0.0, 0.5 - q), 1 - q, 3)
        add(z(0.25, 0.25, 0.5), 0.25, 1)
    for u in (0.0, 0.5, 1 - q):
        add(z(1.0), u, 0)
    add(z(0.5, 0.5 - q), 1 - q, 1)
    add(z(0.5, 0.5 - q), 0.0, 0)
    last = z()
    last[-1] = 1.0
    add(last, 1 - q, K - 1)
    add(last, 0.0, K - 1)
    add(z(), 0.5, K - 1)
    return np.asarray(rows, dtype=np.float32), np.asarray(us, dtype=np.float32), np.asarray(want, dtype=np.int64)


def tie_probs(K):
    """Rows with exact ties for the deterministic pick -> (probs fp32 [m, K], the first maximum [m])."""
    rows = [np.full(K, 1.0 / K), np.r_[np.zeros(K - 2), 0.5, 0.5], np.r_[0.5, np.zeros(K - 2), 0.5], np.zeros(K)]
    p = np.asarray(rows, dtype=np.float32)
    return p, np.asarray([0, K - 2, 0, 0], dtype=np.int64)


def mixed_uniforms(case, n):
    """[n] fp32 uniforms for the sampler / rollout tests: 0, 1 - 2^-24 and seeded uniforms, mixed across rows (row i: i % 4 == 0 ->
    1 - 2^-24, i % 4 == 1 -> 0, else cc.uniforms)."""
    u = cc.uniforms(case, n).copy()
    i = np.arange(n)
    u[i % 4 == 0] = U_MAX
    u[i % 4 == 1] = 0.0
    return u
