"""CPU: the inputs, the float64 reference and the gates of tests/test_gpu_cat_edges.py (tests/cat_edge_cases.py), checked without a
GPU. The row-kind conditions every case's `scale` is chosen for, at every batch size the GPU tests use; the fp32 numpy restatement
of cat_dist / cat_logp / cat_pick / cat_loss_row (emulate32) held to every gate — the proof that the reference and the gates
agree with correctly rounded fp32 arithmetic before a kernel runs; the sampler's reference on crafted rows, the row the old
fall-back got wrong among them; and where torch's Categorical(probs=softmax) coincides with the exact log-softmax and where it
does not (the documented deviation, pinned once)."""
import numpy as np
import pytest
import torch

import cat_cases as cc
import cat_edge_cases as ce
from cat_edge_cases import EDGE_CASES

NAMES = list(EDGE_CASES)
SIZES = {name: sorted(set(ce.LOSS_NS[name]) | {ce.POOL_N}) for name in NAMES}


@pytest.mark.parametrize("name", NAMES)
def test_row_kinds_at_every_size(name):
    """REQUIRED[name] from the fp32 and the float64 restatement (orc.FORWARDS through the case's oracle) at every n the GPU tests
    use: at least KIND_SHARE of the rows of every required kind for n >= 64. The stored actions: every index where n >= K, and
    among them probabilities below CLAMP_EPS and (the cases that hold kind (c)) exactly 0."""
    K = EDGE_CASES[name]["K"]
    for n in SIZES[name]:
        b = ce.batch(name, n)
        got = ce.check_kinds(name, b["logits32"])
        got64 = ce.check_kinds(name, b["logits64"].astype(np.float32))
        sub, zero = ce.acts_kinds(b["logits32"], b["acts"])
        print("\n[%s n=%d] rows of kind %s (float64 logits: %s); stored actions below eps %d, at zero %d" % (name, n, got, got64, sub, zero))
        acts = b["acts"]
        assert acts.dtype == np.int64 and acts.shape == (n,) and acts.min() >= 0 and acts.max() < K
        if n >= K:
            assert set(acts.tolist()) == set(range(K))
        if n >= 64:
            assert sub >= 1 and (zero >= 1 or "c" not in ce.REQUIRED[name])
        z64 = b["logits64"]
        assert (acts == z64.argmax(axis=1)).sum() >= n // 2 - K and (acts == z64.argmin(axis=1)).sum() >= n // 4 - K
        assert abs(float(b["advs"].mean()) - 4.0) < 0.05 and b["advs"].dtype == np.float32
    assert EDGE_CASES["edge_hard"]["scale"] > EDGE_CASES["edge_mid"]["scale"]


def _worst(into, key, r):
    into[key] = max(into.get(key, 0.0), r)


@pytest.mark.parametrize("name", NAMES)
def test_emulation_stays_within_every_gate(name):
    """emulate32 against head64 / loss64 / pick64 through the gate functions for every n: every error / gate ratio <= 1."""
    case = EDGE_CASES[name]
    worst = {}
    for n in SIZES[name]:
        b = ce.batch(name, n)
        z, acts, advs = b["logits32"], b["acts"], b["advs"]
        u = ce.mixed_uniforms(case, n)
        e = ce.emulate32(z, acts, advs, u=u)
        R = ce.loss64(z, acts, advs)
        for k, r in ce.head_ratios(e["p"], e["lg"], e["ent"], R).items():
            _worst(worst, k, r)
        assert np.isfinite(e["p"]).all() and np.isfinite(e["lg"]).all() and np.isfinite(e["ent"]).all()
        assert np.abs(e["p"].astype(np.float64).sum(axis=1) - 1.0).max() <= case["K"] * ce.EPS32
        if n >= 2:
            G = ce.loss_gates(R, advs)
            _worst(worst, "dz", ce.ratio(np.abs(e["dz"].astype(np.float64) - R["dz"]), G["dz"]))
            _worst(worst, "rowsum", ce.ratio(np.abs(e["dz"].astype(np.float64).sum(axis=1)), G["rowsum"]))
            for learner in ("a2c", "rf"):
                for k, got in e[learner].items():
                    _worst(worst, learner + "/" + k, ce.ratio(abs(float(got) - R[learner][k]), G[learner][k]))
        want, dist = ce.pick64(e["p"], u)
        clear = dist > ce.BAND
        assert (e["idx"][clear] == want[clear]).all()
        lo, hi = ce.pick_range(e["p"], u)
        assert ((lo <= e["idx"]) & (e["idx"] <= hi)).all()
        assert (e["p"][np.arange(n), e["idx"]] > 0).all()
    print("\n[%s] worst error / gate of the fp32 emulation: %s" % (name, " ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("K", [2, 6, 16])
def test_emulation_on_crafted_logits(K):
    """The hand-built rows of the head test (gaps of 0 .. 1e4, ties, a common offset of 1e4): emulate32 within the gates, nothing
    NaN or Inf, and the probabilities of a gap of 104 and beyond exactly 0 in fp32 while float64 keeps them positive."""
    z = ce.crafted_logits(K)
    h = ce.head64(z, np.zeros(len(z), dtype=np.int64))
    e = ce.dist32(z)
    r = ce.head_ratios(e["p"], e["lg"], e["ent"], h)
    print("\n[K=%d] %d crafted rows, error / gate %s" % (K, len(z), r))
    assert max(r.values()) <= 1.0, r
    assert all(np.isfinite(e[k]).all() for k in ("p", "lg", "ent"))
    far = np.abs(h["t"]) >= 104.0
    assert far.any() and (e["p"][far] == 0).all() and (h["p"][np.abs(h["t"]) < 700] > 0).all()
    assert (e["ent"] >= 0).all() and e["ent"].max() <= np.log(K) * (1 + 1e-6)


@pytest.mark.parametrize("K", [2, 6, 16])
def test_sampler_reference_on_crafted_rows(K):
    """pick64 and the fp32 restatement of cat_pick on the crafted probability rows: both return the stated index on every row —
    3 on [1/4, 1/4, 1/4, 1/4 - 2^-24, 0, ..] at u = 1 - 2^-24 — and never a class of probability 0 (the all-zero row excepted);
    the fall-back to K - 1 this arithmetic had returns K - 1 = 5 / 15 on that row."""
    p, u, want = ce.crafted_probs(K)
    i64, _ = ce.pick64(p, u)
    i32 = ce.pick32(p, u)
    assert i64.tolist() == want.tolist() and i32.tolist() == want.tolist()
    some = p.sum(axis=1) > 0
    assert (p[np.arange(len(p)), i32][some] > 0).all()
    if K >= 6:
        row = np.zeros((1, K), dtype=np.float32)
        row[0, :4] = [0.25, 0.25, 0.25, 0.25 - 2.0 ** -24]
        assert float(row[0, 3]) == 0.25 - 2.0 ** -24                       # representable: the row is exact in fp32
        assert ce.pick32(row, [ce.U_MAX]).tolist() == [3] and ce.pick64(row, [ce.U_MAX])[0].tolist() == [3]
        assert ce.pick32(row, [ce.U_MAX], fixed=False).tolist() == [K - 1]  # what the K - 1 fall-back returned
    tp, first = ce.tie_probs(K)
    assert ce.pick32(tp, np.full(len(tp), -1.0)).tolist() == first.tolist()


@pytest.mark.parametrize("name", NAMES)
def test_sampler_reference_on_case_rows(name):
    """On every case's probabilities (dist32 of the pool's logits, cycled to 4096 rows): u = 0 picks the first positive class,
    u = 1 - 2^-24 a class of positive probability on every row (kind (d) rows included: there the old fall-back returned K - 1,
    of probability 0 on the hard cases); with the seeded uniforms the fp32 pick equals pick64 outside the 1e-6 band, which holds
    at most BAND_SHARE of the rows."""
    case = EDGE_CASES[name]
    K = case["K"]
    p = ce.dist32(ce.batch(name, ce.POOL_N)["logits32"])["p"]
    rows = p[np.arange(4096) % len(p)]
    n = len(rows)
    zero = ce.pick32(rows, np.zeros(n))
    assert (zero == np.argmax(rows > 0, axis=1)).all() and (zero == ce.pick64(rows, np.zeros(n))[0]).all()
    top = ce.pick32(rows, np.full(n, ce.U_MAX))
    assert (rows[np.arange(n), top] > 0).all()
    lo, hi = ce.pick_range(rows, np.full(n, ce.U_MAX))
    assert ((lo <= top) & (top <= hi)).all()
    old = ce.pick32(rows, np.full(n, ce.U_MAX), fixed=False)
    bad = int((rows[np.arange(n), old] == 0).sum())
    print("\n[%s] u = 1 - 2^-24: the K - 1 fall-back picks a class of probability 0 on %d of %d rows" % (name, bad, n))
    if "d0" in ce.REQUIRED[name]:
        assert bad >= ce.need(n) // 2
    u = cc.uniforms(case)
    want, dist = ce.pick64(rows, u)
    near = float((dist <= ce.BAND).mean())
    got = ce.pick32(rows, u)
    assert near <= ce.BAND_SHARE, near
    assert (got[dist > ce.BAND] == want[dist > ce.BAND]).all() and got.min() >= 0 and got.max() < K
    assert (rows[np.arange(n), got] > 0).all()
    # cat_cases.inverse_cdf is the same function wherever every probability is positive (the cases of tests/cat_cases.py)
    pos = (rows > 0).all(axis=1)
    if pos.any():
        assert (cc.inverse_cdf(rows[pos], u[pos])[0] == want[pos]).all()


def test_reference_clamp_coincides_on_ordinary_rows_only():
    """Where the documented deviation is inactive and where it is not. On rows of kind (a) fp32
    torch.distributions.Categorical(probs=softmax(z)) — what the reference's CategoricalDisPolicy builds — equals head64 within
    the gates: log-prob of every index, entropy, probabilities. On a row of kind (b) it does not: Categorical clamps the
    probabilities to [eps, 1 - eps] before their log, so a class below eps gets log(2^-23) = -15.94 whatever its logit, and no
    gradient reaches the logits through it. The kernels compute the exact log-softmax there (elem.h, cat_dist: "not reproduced");
    tests/test_gpu_cat_edges.py holds them to head64 on every row."""
    b = ce.batch("edge_mid", 1025)
    z = b["logits32"]
    kinds = ce.row_kinds(z)
    a_rows = np.flatnonzero(kinds["a"])
    assert len(a_rows) >= ce.need(len(z))
    za = torch.tensor(z[a_rows])
    dis = cc.categorical(za)
    h = ce.head64(z[a_rows])
    g = ce.head_gates(h)
    K = z.shape[1]
    lg = torch.stack([dis.log_prob(torch.full((len(a_rows),), j)) for j in range(K)], dim=1).double().numpy()
    # torch normalises the probabilities once more (probs / probs.sum(-1)) and takes logf of the quotient: 3 more roundings of
    # p (3 EPS32 relative, the same in log p) and one library log (C_FN EPS32 |log p|) on top of the softmax's own bound
    extra = ce.EPS32 * (3 + ce.C_FN * np.abs(h["lg"]))
    assert ce.ratio(np.abs(lg - h["lg"]), g["lg"] + extra) <= 1.0
    assert ce.ratio(np.abs(dis.probs.double().numpy() - h["p"]), g["p"] + 3 * ce.EPS32 * h["p"]) <= 1.0
    g_ent = g["H"] + (h["p"] * extra + 3 * ce.EPS32 * h["p"] * np.abs(h["lg"])).sum(axis=1)
    assert ce.ratio(np.abs(dis.entropy().double().numpy() - h["H"]), g_ent) <= 1.0
    # the pin: one row of kind (b)
    i = int(np.flatnonzero(kinds["b"])[0])
    hb = ce.head64(z[i:i + 1])
    j = int(np.argmin(hb["p"][0]))
    assert 0 < hb["p"][0, j] < ce.CLAMP_EPS
    zb = torch.tensor(z[i:i + 1], requires_grad=True)
    lp = cc.categorical(zb).log_prob(torch.tensor([j]))
    assert abs(lp.item() - np.log(ce.CLAMP_EPS)) < 1e-5 and abs(np.log(ce.CLAMP_EPS) + 15.94) < 5e-3
    assert hb["lg"][0, j] < np.log(ce.CLAMP_EPS) - 0.05          # the exact log-softmax lies below the clamp's value
    grad, = torch.autograd.grad(lp.sum(), [zb])
    assert float(grad.abs().max()) == 0.0                         # the clamp passes no gradient
