"""-m gpu: policies.GaussianContPolicy (log sigma from the head's last layer, per row; tests/sd_cases.py) on the HIP engine:
forward and Gaussian head, the loss launch teacher-forced against float64, two PPO updates (and the epoch's hipGraph), the
rollout step on every route the net kind takes, the training loop with checkpoint / resume, and a policy with a logstd parameter
next to it in one process.

Tolerances are the rules of tests/test_gpu_parity.py (its module docstring), tests/test_gpu_wide_actions.py::test_two_updates
(restated here number for number: they are literals of that function), tests/test_gpu_loss_adam.py (gates in units of
EPS32 = 2^-24 times the magnitudes that enter a quantity) and tests/test_gpu_rollout_epilogue.py (ROLLOUT_C x EPS32 x
ppo_ref64.sample_stage_bounds), none of them new."""
import copy
import os

import numpy as np
import pytest
import torch

import ppo_ref64 as ref
import sd_cases as sc
import test_gpu_parity as par
import test_gpu_resume as rsm
import test_gpu_wide_actions as wide
import util
from oracle import ppo_oracle as orc

pytestmark = pytest.mark.gpu

MODES = par.MODES
NAMES = list(sc.SD_CASES)
EPS, C = ref.EPS32, ref.ROLLOUT_C
CLIP, ENT = sc.CLIP_PARA, sc.ENTROPY_COEFF
IX = {k: i for i, k in enumerate(util.STAT_KEYS)}
ST_F16_SAT = 23
# the loss-stage test's log-sigma half of the last layer's bias: below, at, above both clamp bounds and inside
LS_BIAS = [-5.0, 2.0, -6.5, 2.75, -0.4, -4.0, 1.0, 0.3]


def _build(case, mode, dev, seed=None, disjoint=False):
    os.environ["V4L_COMPUTE"] = mode
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    torch.manual_seed(case["seed"] if seed is None else seed)
    pf, vf = sc.build_nets(networks, policies, case)
    if disjoint:  # a pair without a common parameter: each net runs its own base (the layer-by-layer step)
        vf.base = copy.deepcopy(pf.base)
    return pf.to(dev), vf.to(dev)


def _last(pf):
    """weight and bias of the head's last linear layer ([2A, k], [2A])."""
    keys = [k for k in pf.state_dict() if k.startswith("seq_append_fcs.")]
    return pf.state_dict(keep_vars=True)[keys[-2]], pf.state_dict(keep_vars=True)[keys[-1]]


def _spread(pf, A, wscale, lim=1.5):
    """Give every action column its own O(1) mean and its own log sigma on both sides of the clamp bounds: the mean half of the
    last bias = linspace(-lim, lim, A), the log-sigma half = LS_BIAS[:A], the log-sigma rows of the last weight x wscale."""
    w, b = _last(pf)
    with torch.no_grad():
        b[:A].copy_(torch.linspace(-lim, lim, A))
        b[A:].copy_(torch.tensor(LS_BIAS[:A]))
        w[A:].mul_(wscale)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_forward_and_gauss_head(name, mode, device):
    """tests/test_gpu_tact.py::test_forward_and_gauss_head's statements and bounds: the head row [mean | raw log sigma] against
    the same-mode restatement (f32 gate / the restatement's own envelope), value likewise, the fixture distance for the two
    fixture cases; std / log_std are [B, A] and exp / clamp of the engine's own row; log-prob / entropy of update() against
    orc.log_prob_entropy on the engine's own mean and std."""
    case = sc.SD_CASES[name]
    A, B, tanh = case["A"], case["B"], case["kind"].endswith("_tanh")
    pf, vf = _build(case, mode, device)
    b = util.make_batch(case)
    obs = torch.tensor(b["obs"], dtype=torch.float32)
    acts = torch.tensor(b["acts"], dtype=torch.float32)
    mean, std, log_std = pf(obs.to(device))
    value = vf(obs.to(device))
    up = pf.update(obs.to(device), acts.to(device))
    opf, ovf = par._oracle_params(pf, vf, case["kind"])
    with torch.no_grad():
        oo = orc.FORWARDS[case["kind"]](opf, obs, case["S"], mode)
        ov = orc.FORWARDS[case["kind"]](ovf, obs, case["S"], mode)
    om, ostd, ols, oraw = sc.head(oo)
    row = torch.cat([mean, log_std], dim=-1).cpu()  # (no raw log sigma of these cases is clamped: tests/test_sd_cpu.py)
    assert float(torch.minimum((oraw - sc.LOG_SIG_MIN).abs(), (oraw - sc.LOG_SIG_MAX).abs()).min()) >= sc.CLAMP_MARGIN
    em, ev = util.rel_err(row, oo), util.rel_err(value.cpu(), ov)
    print("\n[%s %s] rel err vs %s-restatement: head row %.2e value %.2e" % (name, mode, mode, em, ev))
    util.record("sd/forward/%s/%s/row_vs_oracle" % (name, mode), em)
    if mode == "f32":
        assert em < par.TOL[mode] and ev < par.TOL[mode]
    else:
        env_m = wide._forward_envelope(name + "/pf", mode, opf, obs, case)
        env_v = wide._forward_envelope(name + "/vf", mode, ovf, obs, case)
        assert em <= max(par.ENV_FACTOR * env_m, par.ENV_FLOOR), (em, env_m)
        assert ev <= max(par.ENV_FACTOR * env_v, par.ENV_FLOOR), (ev, env_v)
    if name in sc.FIXTURE_CASES:
        gold = util.load_golden("ppo_" + name)
        grow = np.concatenate([gold["fwd_mean"], gold["fwd_log_std"]], axis=1)
        gm = util.rel_err(row, grow)
        print("   vs the reference's fixture: head row %.2e" % gm)
        assert gm < (par.TOL["f32"] if mode == "f32" else par.REF_DIST[mode]), gm
    assert tuple(mean.shape) == tuple(std.shape) == tuple(log_std.shape) == (B, A) and tuple(value.shape) == (B, 1)
    assert torch.allclose(std.cpu(), torch.exp(log_std.cpu())) and float(log_std.min()) >= -5.0 and float(log_std.max()) <= 2.0
    if mode == "f32":
        assert torch.allclose(std.cpu(), ostd, rtol=1e-4, atol=1e-6) and torch.allclose(log_std.cpu(), ols, atol=1e-5)
    for k in ("mean", "std", "log_std"):
        assert torch.equal(up[k], {"mean": mean, "std": std, "log_std": log_std}[k]), k
    lp, ent = orc.log_prob_entropy(mean.cpu(), std.cpu(), acts, tanh_action=tanh)
    assert torch.allclose(up["log_prob"].cpu(), lp, rtol=1e-5, atol=1e-5) and torch.allclose(up["ent"].cpu(), ent, atol=1e-6)
    assert tuple(up["log_prob"].shape) == tuple(up["ent"].shape) == (B, 1)
    # explore(): the reference's keys, log_std [B, A]; with return_log_probs the log-prob of the draw itself
    torch.manual_seed(5)
    ex = pf.explore(obs.to(device), return_log_probs=True)
    assert tuple(ex["log_std"].shape) == tuple(ex["action"].shape) == (B, A) and tuple(ex["log_prob"].shape) == (B, 1)
    z = ex["pre_tanh"] if tanh else ex["action"]
    want = torch.distributions.Normal(ex["mean"], ex["std"]).log_prob(z).sum(-1, keepdim=True)
    if tanh:
        want = want - torch.log(1 - ex["action"] * ex["action"] + 1e-6).sum(-1, keepdim=True)
    assert torch.allclose(ex["log_prob"], want, rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------------------------------------ loss stage, teacher-forced
def _away(x, points, gap):
    x = x.copy()
    for p in points:
        near = np.abs(x - p) < gap
        x[near] = p + np.where(x[near] >= p, gap, -gap)
    return x


def _ls_conditions(raw):
    """The conditions on the log-sigma half of the head rows a launch left in the workspace."""
    lo, hi = raw < sc.LOG_SIG_MIN, raw > sc.LOG_SIG_MAX
    inside = ~lo & ~hi
    straddle = any((lo[:, a].any() and inside[:, a].any()) or (hi[:, a].any() and inside[:, a].any()) for a in range(raw.shape[1]))
    gap = np.minimum(np.abs(raw - sc.LOG_SIG_MIN), np.abs(raw - sc.LOG_SIG_MAX)).min()
    return bool(lo.any() and hi.any() and inside.any() and straddle and gap >= 1e-4)


def _loss_inputs(pf, tpf, vf, case, n, device, seed, tanh):
    """A rollout of n slots around the nets' own outputs (one preliminary forward of each net), like
    tests/test_gpu_loss_adam.py::_inputs with sigma per row."""
    rs = np.random.RandomState(seed)
    A = case["A"]
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float32), device=device)
    net = pf.hip
    net.ensure_bound()
    st, im = net.alloc_rollout(n, device)
    net.ingest(t(util.obs_rows(rs, n, case)), st, im)
    row0 = net.forward(st, im, n)[:, :2 * A].double().cpu().numpy()
    v0 = vf.hip.forward(st, im, n)[:, 0].double().cpu().numpy()
    mean0, sig = row0[:, :A], np.exp(np.clip(row0[:, A:], -5.0, 2.0))
    x = mean0 + sig * np.clip(rs.randn(n, A), -2.0, 2.0)
    acts = np.clip(np.tanh(x), -0.999, 0.999) if tanh else x
    acts = acts.astype(np.float32).astype(np.float64)
    R0 = sc.loss_stage64(row0, None, np.zeros(n), acts, np.ones(n) + np.arange(n), A, CLIP, ENT, tanh)
    r = _away(np.exp(rs.uniform(np.log(0.3), np.log(3.0), n)), (1 - CLIP, 1 + CLIP), 2e-3)
    logp = R0["lp"] - np.log(r)
    advs = 4.0 + 0.05 * rs.randn(n)
    rets = v0 + rs.choice([-1.0, 1.0], n) * rs.uniform(0.05, 2.0, n)
    oldv = v0 + rs.uniform(-0.6, 0.6, n)
    arrs = {k: t(v) for k, v in dict(acts=acts, advs=advs, rets=rets, oldv=oldv, logp=logp).items()}
    rows = torch.tensor(rs.permutation(n).astype(np.int32)[None], device=device)
    return st, im, arrs, rows, {k: v.double().cpu().numpy() for k, v in arrs.items()}


def _check_loss_stage(tag, got, inp, rows, A, n, tanh, stored):
    """What the launches left against sc.loss_stage64 on the same fp32 head rows. Gates as in
    tests/test_gpu_loss_adam.py::_check_loss_stage, with sigma per row."""
    sl = rows[0].cpu().numpy()
    pick = {k: v[sl] for k, v in inp.items()}
    gs = got["gs"]
    R = sc.loss_stage64(got["row"], None if stored else got["trow"], pick["logp"] if stored else None, pick["acts"], pick["advs"],
                        A, CLIP, ENT, tanh, gs)
    st, s = got["stats"], R["stats"]
    an, ratio = R["an"], R["ratio"]
    amean, astd = s["advs/mean"], s["advs/std"]
    raw, opn = R["raw"], R["open"]
    assert _ls_conditions(raw), tag  # the conditions hold on the rows the loss launch read

    def row_err(rr):  # fp32 error of one policy's log pi on head rows rr: (e_lp [n], x, d, var, z2, e_x)
        mu, sig = rr[:, :A], np.exp(np.clip(rr[:, A:2 * A], -5.0, 2.0))
        x = np.arctanh(pick["acts"]) if tanh else pick["acts"]
        z2 = ((x - mu) / sig) ** 2
        corr = np.abs(np.log(1 - pick["acts"] ** 2 + 1e-6)).sum(1) if tanh else 0.0
        e_x = 4 * EPS * (1 + np.abs(x)) if tanh else np.zeros_like(x)
        e_d2 = (np.abs(x - mu) * e_x / sig ** 2).sum(1)
        mag = (0.5 * z2 + np.abs(np.log(sig)) + 1.0).sum(1) + corr
        return 8 * EPS * (A + 2) * mag + e_d2, x, x - mu, sig ** 2, z2, e_x
    e_lp, x, d, var, z2, e_x = row_err(got["row"])
    e_lpo = 8 * EPS * np.abs(pick["logp"]) if stored else row_err(got["trow"])[0]
    e_ratio = e_lp + e_lpo + 8 * EPS * np.abs(R["lp"])
    e_an = 8 * EPS * (np.abs(pick["advs"]) + abs(amean)) / astd
    worst = {}

    def gate(name, err, lim):
        r = float(np.max(err / lim)) if np.size(err) else 0.0
        worst[name] = r
        util.record("sd/loss_stage/%s/%s_err_over_gate" % (tag, name), r)
        assert r <= 1.0, (tag, name, r, np.argmax(err / lim))
    gate("advs/mean", abs(st[0] - amean), 2 * EPS * abs(amean))
    gate("advs/std", abs(st[1] - astd), 8 * EPS * astd + 4 * EPS * abs(amean) / np.sqrt(n))
    assert st[2] == s["advs/max"] and st[3] == s["advs/min"]
    dv = np.abs(got["values"]) + np.abs(pick["rets"])
    vf_loss = np.mean((got["values"] - pick["rets"]) ** 2)
    gate("vf_loss", abs(st[4] - vf_loss), 8 * EPS * np.mean(dv * (dv + np.abs(got["values"] - pick["rets"]))) + 1e-30)
    gate("logprob/mean", abs(st[7] - s["logprob/mean"]), np.mean(e_lp) + 2 * EPS * abs(s["logprob/mean"]))
    gate("logprob/std", abs(st[8] - s["logprob/std"]), 2 * np.max(e_lp) + 4 * EPS * s["logprob/std"])
    gate("logprob/max", abs(st[9] - s["logprob/max"]), np.max(e_lp))
    gate("logprob/min", abs(st[10] - s["logprob/min"]), np.max(e_lp))
    # log_std/*: statistics of the clamped [n, A] tensor — fp32 values the float64 restatement holds exactly
    gate("log_std/mean", abs(st[IX["log_std/mean"]] - s["log_std/mean"]), 2 * EPS * 5.0)
    gate("log_std/std", abs(st[IX["log_std/std"]] - s["log_std/std"]), 8 * EPS * 5.0)
    assert st[IX["log_std/max"]] == s["log_std/max"] == 2.0 and st[IX["log_std/min"]] == s["log_std/min"] == -5.0
    gate("ratio/max", abs(st[15] - s["ratio/max"]), np.max(e_ratio * ratio) + 2 * EPS * s["ratio/max"])
    gate("ratio/min", abs(st[16] - s["ratio/min"]), np.max(e_ratio * ratio) + 2 * EPS * s["ratio/min"])
    sur_mag = ratio * (np.abs(an) * (e_ratio + 4 * EPS) + e_an)
    gate("policy_loss", abs(st[6] - s["Training/policy_loss"]),
         np.mean(sur_mag) + 8 * EPS * (np.mean(ratio * np.abs(an)) + ENT * A * 8))
    edge = (np.abs(ratio - (1 - CLIP)) < 1e-4) | (np.abs(ratio - (1 + CLIP)) < 1e-4)
    assert edge.sum() <= (max(1, n // 500) if stored else n), edge.sum()
    # ---- the d(out) rows the backward consumed, scaled back by grad_scale (a power of two)
    dout = got["dout"] / gs
    # fixed numbers: no gradient through a clamped log sigma, nothing in the columns past 2 A
    assert np.all(got["dout"][:, A:2 * A][~opn] == 0.0) and np.all(got["dout"][:, 2 * A:] == 0.0)
    assert np.all(R["dout"][:, A:][~opn] == 0.0) and np.all(R["dout"][:, A:][opn] != 0.0)
    keep = ~edge
    dlp = np.abs(ratio * an / n)
    e_d = e_x + 2 * EPS * (np.abs(x) + np.abs(got["row"][:, :A]))
    rel = (e_ratio + 16 * EPS)[:, None]
    lim_m = np.abs(R["dout"][:, :A]) * rel + (ratio * e_an / n)[:, None] * np.abs(d) / var + dlp[:, None] * e_d / var + 1e-30
    lim_l = (dlp[:, None] * (2 * np.abs(d) * e_d / var + (z2 + 1) * 16 * EPS) + (z2 + 1) * ((ratio * e_an / n) + dlp * e_ratio)[:, None]
             + 8 * EPS * ENT / n + 1e-30)
    want = R["dout"]
    lim = np.concatenate([lim_m, lim_l], axis=1)
    clamp = sc.F16_GRAD_CLAMP / gs
    sat = np.abs(want) > clamp
    amb = np.abs(np.abs(want) - clamp) <= lim
    if gs != 1.0:
        want = np.where(sat, np.sign(want) * clamp, want)
    err = np.where(amb, 0.0, np.abs(dout[:, :2 * A] - want))
    gate("dmean", err[keep][:, :A], lim_m[keep])
    gate("dlogsigma", np.where(opn, err[:, A:], 0.0)[keep], lim_l[keep])
    nsat = int(round(st[ST_F16_SAT] - got["sat_critic"]))
    if gs == 1.0:
        assert nsat == 0 and R["sat"] == 0
    else:
        assert int(sat[~amb].sum()) <= nsat <= int((sat | amb).sum()) + int(edge.sum()) * 2 * A, (nsat, int(sat.sum()), R["sat"])
    return worst, int(sat.sum())


@pytest.mark.parametrize("stored", [True, False], ids=["stored_logp", "target_forward"])
@pytest.mark.parametrize("tanh", [False, True], ids=["plain", "tanh"])
@pytest.mark.parametrize("mode", MODES)
def test_loss_stage_vs_float64(mode, tanh, stored, device):
    """actor_loss_sd_kernel through the trainer's own launches (begin -> critic_grads -> actor_grads, no step), A = 8, n = 23
    (a partial wave of the 256-thread block), 257 (a second trip) and 513 (the 1024-thread block), against sc.loss_stage64 fed
    the fp32 head rows the launches left in the workspace. The head is spread first (_spread: wscale 250) so that the log-sigma
    elements lie below -5, inside and above 2, a column has rows on both sides of a bound and none lies within 1e-4 of one —
    asserted on the rows read back. Seed: the first of 77, 87, 97, ... whose forward in this mode meets the conditions at all
    three batch sizes (printed): 77 in f32 and bf16, 107 in f16 (its forward misses a condition at 77, 87 and 97)."""
    from vision4leg_amd.engine import HipTrainer
    ns, A = (23, 257, 513), 8
    for seed in range(77, 137, 10):
        case = dict(kind="mlp_tanh" if tanh else "mlp", S=93, A=A, seed=seed, B=64, enc=[256, 256], head=[256, 256])
        pf, vf = _build(case, mode, device)
        _spread(pf, A, 250.0, lim=1.0 if tanh else 1.5)
        tpf = copy.deepcopy(pf).to(device)
        if not stored:  # a target that differs: ratios on both sides of 1 from the forward itself
            w, b = _last(tpf)
            with torch.no_grad():
                b[:A].add_(torch.linspace(-0.3, 0.3, A, device=device) * torch.exp(torch.tensor(LS_BIAS[:A], device=device).clamp(-5, 2)))
                b[A:].add_(0.07)
        tr = HipTrainer(pf.hip, vf.hip, tpf.hip, max(ns), CLIP, ENT)
        tr.sync_target()
        runs = []
        for n in ns:
            st_, im, arrs, rows, inp = _loss_inputs(pf, tpf, vf, case, n, device, seed=2000 + n, tanh=tanh)
            ro = HipTrainer.rollout(st_, im, arrs["acts"], arrs["advs"], arrs["rets"], arrs["oldv"], arrs["logp"] if stored else None)
            stats = torch.zeros(1, 24, device=device)
            tr._pre(n)
            tr.begin(rows, stats, 1e-3, 1e-3)
            tr.critic_grads(ro, n)
            got = {"values": vf.hip.ws_view(n, "out", n, 16, tr.ws)[:, 0].double().cpu().numpy(),
                   "sat_critic": float(tr.stats_cur()[ST_F16_SAT].item())}
            tr.actor_grads(ro, n)
            torch.cuda.synchronize()
            got["row"] = pf.hip.ws_view(n, "out", n, 16, tr.ws).double().cpu().numpy()
            got["dout"] = pf.hip.ws_view(n, "dout", n, 16, tr.ws).double().cpu().numpy()
            if not stored:  # the frozen target's rows: its workspace starts behind the larger of pf's / vf's (v4l_trainer_actor_grads)
                off = max(pf.hip.ws_floats(n), vf.hip.ws_floats(n)) + tpf.hip.ws_offset(n, "out")
                got["trow"] = tr.ws[off:off + n * 16].view(n, 16).double().cpu().numpy()
            got["stats"] = tr.stats_cur().double().cpu().numpy()
            got["gs"] = pf.hip.grad_scale(n)
            runs.append((n, got, inp, rows))
        if all(_ls_conditions(g["row"][:, A:2 * A]) for _, g, _, _ in runs):
            break
    else:
        raise AssertionError("no seed in 77 .. 127 meets the log-sigma conditions in mode %s" % mode)
    print("\n[sd loss stage %s%s %s] seed %d" % (mode, " tanh" if tanh else "", "stored" if stored else "target", seed))
    assert pf.hip.param_names == [k for k in pf.state_dict()] and tr.g_pf.numel() == pf.hip.total_params  # no logstd slot
    for n, got, inp, rows in runs:
        tag = "A8%s/%s/n%d/%s" % ("_tanh" if tanh else "", "stored" if stored else "target", n, mode)
        worst, nsat = _check_loss_stage(tag, got, inp, rows, A, n, tanh, stored)
        print("   n = %4d: worst error / gate %s; clamped elements (f16) %d" % (n, " ".join("%s %.2f" % kv for kv in worst.items()), nsat))


# ------------------------------------------------------------------------------------------------------------ two updates
def _ppo(pf, vf, case, device, **kw):
    from vision4leg_amd.torchrl.algo import PPO

    class Coll: epoch_frames = 1
    return PPO(pf=pf, vf=vf, plr=sc.LR, vlr=sc.LR, clip_para=CLIP, opt_epochs=3, tau=0.95, shuffle=True, entropy_coeff=ENT,
               env=None, replay_buffer=None, collector=Coll(), logger=None, device=device, discount=0.99, num_epochs=1500,
               batch_size=case["B"], save_dir=None, **kw)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_two_updates(name, mode, device):
    """tests/test_gpu_wide_actions.py::test_two_updates on these cases, its bounds number for number: 18 infos and every
    parameter of pf and vf after each PPO.update against the same-mode restatement; in f32 also against the reference's
    fixture for the two fixture cases."""
    case = sc.SD_CASES[name]
    n_updates = sc.updates_of(case)
    pf, vf = _build(case, mode, device)
    agent = _ppo(pf, vf, case, device)
    oracle = sc.oracle_of(pf.state_dict(), vf.state_dict(), case, mode)
    opf, ovf = oracle.pf, oracle.vf
    gold = util.load_golden("ppo_" + name) if name in sc.FIXTURE_CASES else None
    ref32 = sc.oracle_of(pf.state_dict(), vf.state_dict(), case, "f32") if gold is None and mode != "f32" and n_updates > 1 else None
    agent.trainer.sync_target()
    for u in range(n_updates):
        before = {k: v.detach().cpu().clone() for k, v in pf.state_dict().items()}
        args = sc.batch_tensors(case, u) + (sc.LR, sc.LR)
        info = agent.update(sc.host_batch(case, u))
        oinfo = oracle.update(*args)
        ginfo = dict(zip(util.STAT_KEYS, gold["u%d/info" % u])) if gold is not None else ref32.update(*args) if ref32 else None
        print("\n[%s %s] update %d info (hip / restatement):" % (name, mode, u))
        for k in util.STAT_KEYS:
            print("   %-22s % .6f % .6f" % (k, info[k], oinfo[k]))
        assert np.isfinite([info[k] for k in util.STAT_KEYS]).all()  # log_std/std too, at A = 1
        for k in util.STAT_KEYS:
            tol = (5e-4 if mode == "f32" else 5e-3) * max(1.0, abs(oinfo[k]))
            if mode == "f16" and u == 0 and gold is not None:
                assert abs(info[k] - ginfo[k]) <= 1e-3 * max(1.0, abs(ginfo[k])), (u, k, info[k], ginfo[k])
            strict_ok = abs(info[k] - oinfo[k]) <= tol
            if mode != "f32" and u >= 1 and k in ("grad_norm/pf", "ratio/max", "ratio/min", "Training/policy_loss"):
                assert strict_ok or abs(info[k] - ginfo[k]) <= 5e-2 * max(1.0, abs(ginfo[k])), (u, k, info[k], oinfo[k], ginfo[k])
                continue
            assert strict_ok, (u, k, info[k], oinfo[k])
            if mode == "f32" and gold is not None:
                assert abs(info[k] - ginfo[k]) <= tol, (u, k, info[k], ginfo[k])
        worst, tot, cnt = 0.0, 0.0, 0
        for tag, net, onet in (("pf", pf, opf), ("vf", vf, ovf)):
            for k, v in net.state_dict().items():
                dd = (v.detach().cpu() - onet[k]).abs()
                worst = max(worst, dd.max().item())
                tot += dd.sum().item(); cnt += dd.numel()
                assert dd.max().item() <= (2e-5 if mode == "f32" else 2.2e-4 * (u + 1)), (u, tag, k, dd.max().item())
                if mode == "f32" and gold is not None and ("u%d/%s/%s" % (u, tag, k)) in gold.files:
                    assert np.abs(v.detach().cpu().numpy() - gold["u%d/%s/%s" % (u, tag, k)]).max() <= 2e-5, (u, tag, k)
        util.record("sd/ppo_update/%s/%s/u%d/worst_abs_param_vs_oracle" % (name, mode, u), worst)
        assert tot / cnt <= (1e-7 if mode == "f32" else 2e-5 * (u + 1))
        assert max((pf.state_dict()[k].cpu() - before[k]).abs().max().item() for k in before) > 5e-5  # the optimiser stepped
        w0, w1 = before[list(before)[-2]], pf.state_dict()[list(before)[-2]].cpu()
        assert (w1 - w0)[case["A"]:].abs().max().item() > 0  # ... in the log-sigma rows of the last layer as well
    assert agent.f16_saturated == 0


def _epoch_agent(case, seed, dev, **kw):
    """tests/test_gpu_resume.py::_agent on these nets."""
    from vision4leg_amd.torchrl.algo import PPO
    from vision4leg_amd.torchrl.replay_buffers import DeviceOnPolicyReplayBuffer
    pf, vf = _build(case, os.environ["V4L_COMPUTE"], dev, seed=seed)
    buf = DeviceOnPolicyReplayBuffer(max_replay_buffer_size=rsm.T * rsm.E, env_nums=rsm.E, time_limit_filter=True)

    class Coll: epoch_frames = rsm.T * rsm.E
    agent = PPO(pf=pf, vf=vf, plr=rsm.LR, vlr=2 * rsm.LR, clip_para=CLIP, opt_epochs=rsm.OPT_EPOCHS, tau=0.95, entropy_coeff=ENT,
                shuffle=True, collector=Coll(), replay_buffer=buf, logger=rsm._Log(), device=dev, discount=0.99,
                num_epochs=rsm.NUM_EPOCHS, batch_size=rsm.B, **kw)
    agent.records = []
    return agent


@pytest.mark.parametrize("opts", [dict(), dict(clipped_value_loss=True, skip_nonfinite_steps=True, optimizer_class="AdamW",
                                               optimizer_kwargs={"weight_decay": 0.01})], ids=["plain", "options"])
@pytest.mark.parametrize("mode", MODES)
def test_epoch_graph_equals_per_update_replays_and_eager(mode, opts, device, monkeypatch):
    """Two epochs of update_per_epoch on the same data: through the epoch's hipGraph, through per-update replays
    (V4L_EPOCH_GRAPH=0) and through eager launches (V4L_GRAPH=0) — parameters, moments and every statistics record bit-equal.
    options: clipped_value_loss, skip_nonfinite_steps and AdamW with weight decay on the same three paths."""
    monkeypatch.setenv("V4L_COMPUTE", mode)
    case = sc.SD_CASES["sd_mlp_odd"]
    out = []
    for env in (dict(V4L_EPOCH_GRAPH="1", V4L_GRAPH="1"), dict(V4L_EPOCH_GRAPH="0", V4L_GRAPH="1"), dict(V4L_GRAPH="0")):
        for k in ("V4L_EPOCH_GRAPH", "V4L_GRAPH"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        a = _epoch_agent(case, case["seed"], device, **opts)
        np.random.seed(5)
        for epoch in range(2):
            rsm._epoch(a, case, epoch)
        assert all(np.isfinite(r[:, :18].numpy()).all() for r in a.records) and a.trainer.adam_steps() == (2 * rsm.U, 2 * rsm.U)
        out.append((rsm._state(a), a.records))
    for st, rec in out[1:]:
        rsm._assert_same(out[0][0], st)
        assert all(torch.equal(x, y) for x, y in zip(out[0][1], rec))


# --------------------------------------------------------------------------------------------------------------- rollout
def _rows_bounds(mean, ls, eps, acts, tanh):
    """ppo_ref64.sample_stage / sample_stage_bounds row by row (they take one log sigma per column)."""
    act, ent, lp, b_act, b_ent, b_lp = [], [], [], [], [], []
    for i in range(mean.shape[0]):
        _, _, a64, e64 = ref.sample_stage(mean[i:i + 1], ls[i], eps[i:i + 1], tanh)
        l64 = ref.log_prob_entropy(torch.tensor(mean[i:i + 1]), torch.tensor(ls[i]), torch.tensor(acts[i:i + 1]), tanh)[0]
        b = ref.sample_stage_bounds(mean[i:i + 1], ls[i], eps[i:i + 1], acts[i:i + 1], tanh)
        act.append(a64.numpy()[0]); ent.append(float(e64[0])); lp.append(float(l64[0]))
        b_act.append(b["action"].numpy()[0]); b_ent.append(float(b["ent"][0])); b_lp.append(float(b["logp"][0]))
    return (np.array(act), np.array(ent), np.array(lp)), (np.array(b_act), np.array(b_ent), np.array(b_lp))


ROLLOUT = [(mode, E, shared, tanh) for mode in ("f32", "bf16", "f16") for E in (3, 64) for shared in (True, False)
           for tanh in (False, True)]


@pytest.mark.parametrize("mode,E,shared,tanh", ROLLOUT,
                         ids=["%s-E%d-%s-%s" % (m, e, "shared" if s else "own", "tanh" if t else "plain") for m, e, s, t in ROLLOUT])
def test_rollout_step(mode, E, shared, tanh, device):
    """engine.HipActor on the shipped geometry (A = 6) with a spread head (sigma differs per row and column, log sigmas beyond
    both clamp bounds), known noise. Per step, on what the kernel consumed (actor.eps) and returned: the route's name; mean and
    log sigma against the layer-by-layer forward; action == mean + std * eps (through tanh), entropy per row and the filed
    log-prob against float64 within ROLLOUT_C x EPS32 x sample_stage_bounds; the filed log-prob against
    pf.update(obs, action)["log_prob"]; filing; the deterministic step and eval_act return the mean (through tanh).
    Routes ("GaussianContPolicy"): a shared base runs rollout_mlp_kernel's per-row-sigma instantiation
    (MLP_PER_SAMPLE) in every mode — never MLP_ONE_BLOCK, which the same geometry with a logstd parameter takes in the 16-bit
    modes at E <= 64 —, a pair without a common parameter the layer-by-layer step (GENERAL: act_finish_sd_kernel)."""
    from vision4leg_amd import engine
    from vision4leg_amd.torchrl.policies import RolloutActor
    case = dict(sc.SD_CASES["sd_mlp_tanh" if tanh else "sd_mlp"])
    A = case["A"]
    pf, vf = _build(case, mode, device, disjoint=not shared)
    _spread(pf, A, 20.0, lim=1.0 if tanh else 1.5)
    with torch.no_grad():  # tanh: sigma <= 1 (no sampled action rounds to +-1, where atanh of the stored action ends)
        if tanh:
            _last(pf)[1][A:].clamp_(max=-0.4)
    net = pf.hip
    net.ensure_bound()
    T = 3
    slots = (T + 1) * E
    state, image = net.alloc_rollout(slots, device)
    SENT = -7.0
    acts = torch.full((slots, A), SENT, device=device)
    vals, logp = torch.full((slots,), SENT, device=device), torch.full((slots,), SENT, device=device)
    want_acts, want_vals, want_logp = acts.clone(), vals.clone(), logp.clone()
    obs = torch.tensor(util.obs_rows(np.random.RandomState(3), T * E, case), dtype=torch.float32, device=device)
    ra = RolloutActor(pf, vf, E)
    actor = ra._actor
    assert actor.shared_encoder == shared and tuple(actor.eps.shape) == (E, A)
    assert actor.route() == ("MLP_PER_SAMPLE" if shared else "GENERAL")
    if shared and mode != "f32":  # the twin with a logstd parameter: the one-block kernel
        bpf, bvf = par._build(dict(case, kind="mlp"), mode, device)
        assert engine.HipActor(bpf.hip, bvf.hip, E, shared_encoder=True, graph=False).route() == "MLP_ONE_BLOCK"
    actor.attach((state, image, acts, vals, logp))
    actor.seek(0)
    tol = 1e-5 if mode == "f32" else 4e-3
    f64 = lambda t: t.detach().double().cpu().numpy()
    worst = {}
    for s in range(T):
        det = s == T - 1
        ob = obs[s * E:(s + 1) * E]
        torch.manual_seed(100 + s)
        actor.step(ob, deterministic=det)
        torch.cuda.synchronize()
        out = {k: v.clone() for k, v in actor._out.items()}
        eps = actor.eps.clone()
        assert bool((eps == 0).all()) == det
        sl = slice(s * E, (s + 1) * E)
        mean, std, action, ent, value = (f64(out[k]) for k in ("mean", "std", "action", "ent", "value"))
        assert mean.shape == std.shape == action.shape == (E, A)
        ent, value = ent.reshape(E), value.reshape(E)
        stored_a, stored_lp = f64(acts[sl]), f64(logp[sl])
        with torch.no_grad():
            sep_mean, sep_std, sep_ls = pf(ob)
            sep_value = vf(ob)
            up = pf.update(ob, acts[sl])
            st_, im_, _ = pf.hip.stage(ob)
            sep_raw = pf.hip.forward(st_, im_, E)[:, A:2 * A].double().cpu().numpy()  # the layer-by-layer row's raw log sigma
        sep_mean, sep_ls, sep_value = f64(sep_mean), f64(sep_ls), f64(sep_value).reshape(E)
        ls = np.log(std)  # the kernel's own clamped log sigma (std = expf of it: 4 EPS32 relative)
        r = {"mean": np.abs(mean - sep_mean).max() / (tol * max(1.0, np.abs(sep_mean).max())),
             # (log sigma is the same GEMM's output as the mean: the same rule on the raw columns' magnitude; + expf / log of std)
             "log_std": np.abs(ls - sep_ls).max() / (tol * max(1.0, np.abs(sep_raw).max()) + 8 * EPS * 5),
             "value": np.abs(value - sep_value).max() / (tol * max(1.0, np.abs(sep_value).max()))}
        (act64, ent64, lp64), (b_act, b_ent, b_lp) = _rows_bounds(mean, ls, f64(eps), stored_a, tanh)
        slack = 8 * EPS * (1 + ((stored_a if not tanh else np.arctanh(stored_a)) - mean) ** 2 / std ** 2).sum(1)  # log(std)'s own rounding in lp
        r["action"] = util_ratio(np.abs(action - act64), C * EPS * b_act)
        r["ent"] = util_ratio(np.abs(ent - ent64), C * EPS * b_ent + 8 * EPS * A)
        r["logp"] = util_ratio(np.abs(stored_lp - lp64), C * EPS * b_lp + slack)
        # the filed log-prob against pf.update(obs, action)["log_prob"] (layer-by-layer forward: its mean / log sigma are within tol)
        x = np.arctanh(stored_a) if tanh else stored_a
        sens = (np.abs(x - sep_mean) / np.exp(sep_ls) ** 2 + (x - sep_mean) ** 2 / np.exp(sep_ls) ** 2 + 1.0).sum(1)
        r["logp_vs_update"] = util_ratio(np.abs(stored_lp - f64(up["log_prob"]).reshape(E)),
                                         tol * max(1.0, np.abs(sep_mean).max(), np.abs(sep_raw).max()) * sens + C * EPS * b_lp + slack)
        print("\n[sd rollout %s E%d %s %s step %d] error / bound: %s" % (mode, E, "shared" if shared else "own", "tanh" if tanh else "plain",
                                                                        s, " ".join("%s %.3f" % kv for kv in r.items())))
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
            assert v <= 1.0, (s, k, v)
        if tanh:
            assert np.abs(stored_a).max() < 1.0
        assert np.isfinite(stored_lp).all()
        # sigma per row: the rows differ, both clamp bounds are reached, and a clamped element is exactly exp(bound)
        assert not (std == std[:1]).all() and std.max() <= np.float32(np.exp(np.float32(2.0))) * (1 + 4 * EPS)
        assert (sep_ls == -5.0).any() and ((sep_ls == 2.0).any() or tanh)
        if det:
            want = torch.tanh(out["mean"]) if tanh else out["mean"]
            assert torch.equal(out["action"], want) if not tanh else torch.allclose(out["action"], want, rtol=1e-6, atol=1e-7)
        want_acts[sl], want_vals[sl], want_logp[sl] = out["action"], out["value"].view(E), logp[sl]
        assert torch.equal(acts, want_acts) and torch.equal(vals, want_vals) and torch.equal(logp, want_logp), s
        assert bool((logp[sl] != SENT).all()) and bool((acts[(s + 1) * E:] == SENT).all()) and bool((logp[(s + 1) * E:] == SENT).all())
    for k, v in worst.items():
        util.record("sd/rollout/%s-E%d-%s-%s/%s" % (mode, E, "shared" if shared else "own", "tanh" if tanh else "plain", k), v)
    # eval_act: the mean (through tanh), from the fused step and from the module
    if E == 3:
        one = RolloutActor(pf, vf, 1)
        a1 = one.eval_act(obs[:1])
        m1 = pf.eval_act(obs[:1])
        assert a1.shape == m1.shape == (A,) and np.abs(a1 - m1).max() <= tol * max(1.0, np.abs(m1).max())


def util_ratio(err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    return float(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300)).max())


# ------------------------------------------------------------------------------------------------------------------ loop
def _loop_agent(case, seed, device, save_dir, E, T, B, num_epochs, **kw):
    from vision4leg_amd.torchrl.algo import PPO
    from vision4leg_amd.torchrl.collector import VecOnPolicyCollector
    from vision4leg_amd.torchrl.replay_buffers import DeviceOnPolicyReplayBuffer
    pf, vf = _build(case, os.environ["V4L_COMPUTE"], device, seed=seed)
    env = util.FakeVecEnv(E, case["S"], case["A"], img=0, seed=9, p_done=0.12, time_limit_key=True)
    eval_env = util.FakeVecEnv(E, case["S"], case["A"], img=0, seed=1, p_done=0.3)
    buf = DeviceOnPolicyReplayBuffer(max_replay_buffer_size=E * T, env_nums=E, time_limit_filter=True)
    coll = VecOnPolicyCollector(vf, env=env, eval_env=eval_env, pf=pf, replay_buffer=buf, device=device, epoch_frames=E * T)
    assert coll.fast_path
    return PPO(pf=pf, vf=vf, plr=sc.LR, vlr=sc.LR, clip_para=CLIP, opt_epochs=2, tau=0.95, shuffle=True, entropy_coeff=ENT,
               env=None, replay_buffer=buf, collector=coll, logger=rsm._Log(), device=device, discount=0.99, num_epochs=num_epochs,
               batch_size=B, save_interval=1, eval_interval=1, save_dir=save_dir, **kw)


@pytest.mark.parametrize("mode", MODES)
def test_train_loop_checkpoint_and_resume(mode, device, tmp_path, monkeypatch):
    """PPO.train() over tests/util.FakeVecEnv(E = 4, S = 93, A = 6) with the resident buffer (fused rollout step, stored log
    pi_old), T = 16, B = 32, three epochs; then fresh objects resumed from the second epoch's train state with the simulator put
    back: parameters, Adam moments, step counts and the third epoch's infos are equal bit for bit. The reference-format model
    files hold exactly the reference class's keys (the fixture's) and load back."""
    monkeypatch.setenv("V4L_COMPUTE", mode)
    case = sc.SD_CASES["sd_mlp"]
    E, T, B = 4, 16, 32
    U = 2 * (E * T // B)
    np.random.seed(3); torch.manual_seed(3); torch.cuda.manual_seed(3)
    a = _loop_agent(case, case["seed"], device, str(tmp_path / "first"), E, T, B, 3, save_train_state=True)
    assert tuple(a.replay_buffer.step_arrays(a.pf.hip.act_dim)[2].shape) == (E * T, case["A"])
    snap, inner = {}, a.save_checkpoint

    def save(prefix, epoch):
        inner(prefix, epoch)
        if epoch == 1:
            c = a.collector
            snap.update(env_rs=c.env.rs.get_state(), env_ob=c.env.ob.copy(), eval_rs=c.eval_env.rs.get_state(),
                        ob=np.array(c.current_ob, copy=True))
    a.save_checkpoint = save
    a.train()
    assert a.trainer.adam_steps() == (3 * U, 3 * U) and len(a.logger.updates) == 3 * U and a.f16_saturated == 0
    for x in a.logger.updates:
        assert sorted(x) == sorted(util.STAT_KEYS) and np.isfinite(list(x.values())).all()
    b = _loop_agent(case, case["seed"] + 100, device, str(tmp_path / "resumed"), E, T, B, 3, save_train_state=True,
                    resume=(str(tmp_path / "first"), 1))
    assert b.start_epoch == 2 and b.trainer.adam_steps() == (2 * U, 2 * U) and b.total_frames == 2 * E * T
    c = b.collector
    c.env.rs.set_state(snap["env_rs"]); c.env.ob = snap["env_ob"].copy(); c.eval_env.rs.set_state(snap["eval_rs"])
    c.current_ob = snap["ob"].copy()
    b.load_checkpoint(str(tmp_path / "first"), 1, restore_collector=True)
    b.train()
    assert [e[0] for e in b.logger.epochs] == [2] and b.trainer.adam_steps() == (3 * U, 3 * U)
    assert a.logger.updates[2 * U:] == b.logger.updates
    rsm._assert_same(rsm._state(a), rsm._state(b))
    # the reference-format files: the reference class's key set, loadable
    gold = util.load_golden("ppo_sd_mlp")
    for tag, net in (("pf", a.pf), ("vf", a.vf)):
        sd = torch.load(os.path.join(str(tmp_path / "first"), "model_%s_finish.pth" % tag), map_location="cpu")
        pre = "u0/sum/%s/" % tag
        assert sorted(sd) == sorted(k[len(pre):] for k in gold.files if k.startswith(pre)) and "logstd" not in sd
        assert all(torch.equal(sd[k], v.cpu()) for k, v in net.state_dict().items())


# ------------------------------------------------------------------------------------------------------- no neighbour moved
@pytest.mark.parametrize("mode", MODES)
def test_policy_with_a_logstd_parameter_next_to_it_is_unmoved(mode, device):
    """mlp_s93 with GaussianContPolicyBasicBias, two PPO updates: alone, and with a GaussianContPolicy trainer built, updated
    and interleaved in the same process — the same parameter bits."""
    def run(with_neighbour):
        case = util.CASES["mlp_s93"]
        pf, vf = par._build(case, mode, device)
        agent = wide_agent(pf, vf, case, device)
        if with_neighbour:
            ncase = sc.SD_CASES["sd_mlp"]
            npf, nvf = _build(ncase, mode, device)
            nagent = _ppo(npf, nvf, ncase, device)
            nagent.trainer.sync_target()
            nagent.update(sc.host_batch(ncase, 0))
        agent.trainer.sync_target()
        for u in range(2):
            b = util.make_batch(case, update=u)
            agent.update({k: b[k] for k in ("obs", "acts", "advs", "estimate_returns", "values")})
            if with_neighbour:
                nagent.update(sc.host_batch(ncase, 1))
        torch.cuda.synchronize()
        return {k: v.detach().cpu().clone() for k, v in list(pf.state_dict().items()) + [("vf/" + k, v) for k, v in vf.state_dict().items()]}
    alone, beside = run(False), run(True)
    assert alone.keys() == beside.keys()
    for k in alone:
        assert torch.equal(alone[k], beside[k]), k


def wide_agent(pf, vf, case, device):
    from vision4leg_amd.torchrl.algo import PPO

    class Coll: epoch_frames = 1
    return PPO(pf=pf, vf=vf, plr=1e-4, vlr=1e-4, clip_para=0.2, opt_epochs=3, tau=0.95, shuffle=True, entropy_coeff=0.005,
               env=None, replay_buffer=None, collector=Coll(), logger=None, device=device, discount=0.99, num_epochs=1500,
               batch_size=case["B"], save_dir=None)
