"""The KL-adaptive learning rates of PPO(desired_kl=...): the cases tests/test_kl_lr_cpu.py and
tests/test_gpu_kl_lr.py share, and the semantics restated over oracle.ppo_oracle.PPOOracle.

The restatement wraps three functions of the oracle module for the length of a run, the way tests/kl_cases.py::oracle_run does:

  log_prob_entropy   called twice per update, for the live policy and then for the frozen target: approx_kl[u] = mean(log pi_old) -
                     mean(log pi), in float64 from the oracle's fp32 rows.
  adam_step          the policy's step of update u comes after both calls: there the decision d[u] is taken (-1 if approx_kl >
                     2 * desired_kl, +1 if approx_kl < 0.5 * desired_kl, else 0; a NaN compares false twice) and both rates change
                     in Python floats (doubles), each with one operation and its clamp: max(lr / factor, lr_min) or
                     min(lr * factor, lr_max). The step itself still runs at the rate the update was opened with: the new pair is
                     handed to update u + 1. No step is skipped by the option.
  clip_grad_norm     unchanged (kept wrapped so that a non-finite norm skips its step as skip_nonfinite_steps does).

A case is one of tests/kl_cases.py's geometries and data sets (T = E = 8, B = 32, the narrow policy log sigma = -3 that turns small
parameter steps into large KLs) with starting rates, desired_kl, factor and the clamps. The target stays frozen over a run, so
approx_kl starts at the noise floor (theta == target but for the critic's first step) and grows from update to update: a run
begins with +1 decisions, and with desired_kl inside the range the run reaches it goes on to 0 or -1.

Which cases are valid is decided by the oracle alone (`validity`, asserted by tests/test_kl_lr_cpu.py) in each compute mode:
every update's approx_kl lies at least 2 * kl_cases.kl_tol(mode, logprob/mean) away from both thresholds, so that a device whose
estimate is within kl_tol of the oracle's takes the oracle's decisions. Over the set of cases (`coverage`) each decision occurs,
one run shows two different decisions with the change of rate visible in a later approx_kl (against the fixed-rate run), and one
reaches a clamp. The numbers were chosen on the CPU from the oracle's runs; the rates stay at the order tests/kl_cases.py explains.
"""
import numpy as np
import torch

import kl_cases as kc
import util
from oracle import ppo_oracle as orc

MODES = kc.MODES
T, E, B = kc.T, kc.E, kc.B

# name -> the kl_cases case whose geometry, data and initial log sigma it takes, the starting rates, and the option's four numbers
CASES = {
    # decisions +1, 0, 0, -1, -1, -1 (approx_kl 1e-4, 0.58, 0.58, 1.8, 2.1, 1.9 against the thresholds 0.3 and 1.2): the rate raised
    # by update 0 shows in approx_kl[2] (0.58 against the fixed-rate run's 0.37). The critic's rate starts on kl_lr_min, goes up
    # once and is clamped there by the second -1 while the policy's goes on falling
    "mlp_all_three": dict(base="mlp_s93", plr=4e-4, vlr=1e-5, U=6, desired_kl=0.6, factor=1.5, lr_min=1e-5, lr_max=1e-2),
    # every decision +1 (approx_kl <= 0.62 against 0.5 * desired_kl = 1): the policy's rate is clamped at kl_lr_max = 3e-4 by the
    # first one (2e-4 * 1.5 rounds to just above it) and stays; the critic's keeps growing, six times
    "loco_clamp_max": dict(base="loco_s84", plr=2e-4, vlr=1e-5, U=6, desired_kl=2.0, factor=1.5, lr_min=1e-5, lr_max=3e-4),
    # with skip_nonfinite_steps: update 0's minibatch holds a NaN advantage and its policy step is skipped. The estimate does not
    # depend on the advantages: it stays finite (5e-6, 5e-5, 0.13) and decides +1 each time; the policy's rate sits on kl_lr_max.
    # Three updates: the f16 flavour of the oracle overflows in the scaled backward of update 3 of this run (a second skip that
    # belongs to the oracle, not to the case)
    "mlp_nan_guard": dict(base="mlp_s93", plr=4e-4, vlr=1e-5, U=3, desired_kl=1.0, factor=1.5, lr_min=1e-5, lr_max=4e-4,
                          nan_update=0, guard=True),
}
PLAIN = sorted(k for k, c in CASES.items() if not c.get("guard"))


def geometry(name):
    return kc.geometry(CASES[name]["base"])


def data(name, nan_update=None):
    """kl_cases.data of the case's base, cut to the case's U updates (nan_update: default the case's own, if it has one)."""
    nan_update = CASES[name].get("nan_update") if nan_update is None else nan_update
    dat = kc.data(CASES[name]["base"], nan_update)
    return dat[:5] + (dat[5][:CASES[name]["U"]],)


def cpu_nets(name):
    return kc.cpu_nets(CASES[name]["base"])


def init_policy(pf, name):
    kc.init_policy(pf, CASES[name]["base"])


def decide(kl, desired_kl):
    return -1 if kl > 2.0 * desired_kl else 1 if kl < 0.5 * desired_kl else 0


def next_rate(lr, d, factor, lr_min, lr_max):
    if d < 0:
        return max(lr / factor, lr_min)
    if d > 0:
        return min(lr * factor, lr_max)
    return lr


def oracle_run(name, mode, opf, ovf, dat, desired_kl, rows=None, guard=None, factor=None, lr_min=None, lr_max=None):
    """PPOOracle over `rows` (default: all of the case's) with the adaptive rates; desired_kl None: fixed rates (approx_kl and the
    decision the case's desired_kl would take are still recorded). opf / ovf: initial parameters (cloned). guard (default: the case's): non-finite
    norms skip their step. factor / lr_min / lr_max: instead of the case's.
    -> dict(kl [U] float64, d [U] int, lrs [U + 1][2] the (pf, vf) pair each update opened with and the pair after the run,
    infos, pf, vf, steps {"pf", "vf"})."""
    c = CASES[name]
    guard = c.get("guard", False) if guard is None else guard
    factor = c["factor"] if factor is None else factor
    lr_min = c["lr_min"] if lr_min is None else lr_min
    lr_max = c["lr_max"] if lr_max is None else lr_max
    case, obs, acts, advs, rets = dat[:5]
    rows = dat[5] if rows is None else rows
    kind = case["kind"]
    opf = {k: v.clone() for k, v in opf.items()}
    ovf = util.share_encoder(opf, {k: v.clone() for k, v in ovf.items()}, kind)
    oracle = orc.PPOOracle(kind, opf, ovf, {k: v.clone() for k, v in opf.items()}, case["S"], mode)
    oracle.sync_target()
    clip0, adam0, lpe0 = orc.clip_grad_norm, orc.adam_step, orc.log_prob_entropy
    cur = {"lps": [], "norm": None, "lr": (float(c["plr"]), float(c["vlr"]))}
    kls, ds, lrs, steps = [], [], [], {"pf": 0, "vf": 0}

    def lpe(mean, std, actions, tanh_action=False):
        lp, ent = lpe0(mean, std, actions, tanh_action)
        cur["lps"].append(lp.detach().double().mean().item())
        return lp, ent

    def clip(grads, max_norm):
        g, n = clip0(grads, max_norm)
        cur["norm"] = n
        return g, n

    def adam(params, grads, state, lr, step, *a, **kw):
        which = "pf" if state is oracle.pf_state else "vf"
        if which == "pf":  # both log_prob_entropy calls of this update have run: [live, target]
            live, old = cur["lps"]
            kl = old - live
            d = decide(kl, c["desired_kl"] if desired_kl is None else desired_kl)
            kls.append(kl)
            ds.append(d)
            if desired_kl is not None:  # from the next update on: this step runs at `lr`, the rate the update opened with
                cur["lr"] = tuple(next_rate(r, d, factor, lr_min, lr_max) for r in cur["lr"])
        if guard and not torch.isfinite(cur["norm"]):
            return
        steps[which] += 1
        adam0(params, grads, state, lr, steps[which], *a, **kw)

    orc.clip_grad_norm, orc.adam_step, orc.log_prob_entropy = clip, adam, lpe
    infos = []
    try:
        f = lambda x: torch.tensor(x, dtype=torch.float32)
        for r in rows:
            cur["lps"] = []
            lrs.append(cur["lr"])
            infos.append(oracle.update(f(obs[r]), f(acts[r]), f(advs[r]).view(-1, 1), f(rets[r]).view(-1, 1),
                                       f(rets[r]).view(-1, 1), cur["lr"][0], cur["lr"][1]))
    finally:
        orc.clip_grad_norm, orc.adam_step, orc.log_prob_entropy = clip0, adam0, lpe0
    lrs.append(cur["lr"])
    return dict(kl=np.array(kls), d=np.array(ds, dtype=np.int64), lrs=np.array(lrs, dtype=np.float64), infos=infos, pf=opf, vf=ovf,
                steps=steps)


def margins(name, mode, run):
    """Per update: (distance of approx_kl from the nearer threshold, 2 * kl_tol of that update)."""
    c = CASES[name]
    lo, hi = 0.5 * c["desired_kl"], 2.0 * c["desired_kl"]
    return [(min(abs(k - lo), abs(k - hi)), 2 * kc.kl_tol(mode, i["logprob/mean"])) for k, i in zip(run["kl"], run["infos"])]


def validity(name, mode, run):
    """-> the violated conditions of an adaptive oracle run as strings (empty: valid)."""
    bad = []
    for u, (dist, need) in enumerate(margins(name, mode, run)):
        if not dist >= need:  # (a NaN fails)
            bad.append("update %d: approx_kl %g is %g from a threshold, inside 2 * kl_tol = %g" % (u, run["kl"][u], dist, need))
    return bad


def coverage(mode, runs, fixed):
    """runs / fixed: name -> the adaptive / the fixed-rate oracle run of `mode`. -> the violated set conditions as strings."""
    bad = []
    seen = set(int(d) for r in runs.values() for d in r["d"])
    if seen != {-1, 0, 1}:
        bad.append("decisions seen: %s" % sorted(seen))
    two = False
    for name, r in runs.items():
        ch = [u for u in range(len(r["d"])) if r["d"][u] != 0 and not np.array_equal(r["lrs"][u + 1], r["lrs"][u])]
        if len(set(int(d) for d in r["d"])) >= 2 and ch:
            u = ch[0]  # the first change of rate: the fixed-rate run's approx_kl parts from this run's after it, beyond the tolerance
            later = [abs(r["kl"][v] - fixed[name]["kl"][v]) for v in range(u + 1, len(r["d"]))]
            tol = [2 * kc.kl_tol(mode, i["logprob/mean"]) for i in r["infos"][u + 1:]]
            two = two or any(a > b for a, b in zip(later, tol))
    if not two:
        bad.append("no run with two different decisions and a visible change of rate")
    clamp = False
    for name, r in runs.items():
        c = CASES[name]
        for u, d in enumerate(r["d"]):
            for w in range(2):
                raw = r["lrs"][u][w] / c["factor"] if d < 0 else r["lrs"][u][w] * c["factor"]
                clamp = clamp or (d != 0 and raw != r["lrs"][u + 1][w] and r["lrs"][u + 1][w] in (c["lr_min"], c["lr_max"]))
    if not clamp:
        bad.append("no run reaches a clamp")
    return bad
