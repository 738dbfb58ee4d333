"""-m gpu: algo.PPODiscrete — the clipped-surrogate PPO update on policies.CategoricalDisPolicy (tests/ppo_cat_cases.py) — on the HIP
engine: the loss launch (actor_loss_cat_kernel) teacher-forced against float64 on both log pi_old routes, the updates of every
case against the same-mode restatement and the reference's fixture, the stored-log-pi route against the target route, graph
replays against eager launches, the launch count against a Gaussian PPO update's, the training loop over a discrete vec env with
both buffers, and the C entry points that keep refusing a categorical net.

No bound here is new. The loss stage's gates are ppo_cat_cases.loss_stage_gates (EPS32 times the magnitudes that enter a quantity,
derived there on top of tests/cat_edge_cases.py's head gates); the updates are held to the literals of
tests/test_gpu_sd.py::test_two_updates (infos 5e-4 / 5e-3 relative to max(1, |x|), every parameter element 2e-5 / 2.2e-4 (u + 1),
the mean 1e-7 / 2e-5 (u + 1), its either-or rule for the 16-bit modes from the second update on) and the fixture to
tests/test_gpu_cat.py::test_against_reference_fixture's (5e-4, 2e-5); the training loop's first-update ratios to the 0.01 under
which tests/test_gpu_kl_stop.py holds an epoch's opening approx_kl."""
import copy
import hashlib
import os

import numpy as np
import pytest
import torch

import cat_cases as cc
import cat_edge_cases as ce
import ppo_cat_cases as pc
import sd_cases as sc
import test_gpu_cat as tgc
import test_gpu_parity as par
import test_gpu_resume as rsm
import test_gpu_update_route as route
import util
from ppo_cat_cases import PPO_CAT_CASES

pytestmark = pytest.mark.gpu

MODES = par.MODES
NAMES = list(PPO_CAT_CASES)
CLIP, ENT = pc.CLIP_PARA, pc.ENTROPY_COEFF
IX = {k: i for i, k in enumerate(util.STAT_KEYS)}
LS_KEYS = [k for k in util.STAT_KEYS if k.startswith("log_std/")]
ST_F16_SAT = 23
EITHER_OR = ("grad_norm/pf", "ratio/max", "ratio/min", "Training/policy_loss")
EDGES = (1.0 - CLIP, 1.0 + CLIP)


class _Coll:
    epoch_frames = 1


def _build(case, mode, dev):
    os.environ["V4L_COMPUTE"] = mode
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    pf, vf = pc.seeded_nets(networks, policies, case)
    return pf.to(dev), vf.to(dev)


def _agent(pf, vf, case, device, **kw):
    from vision4leg_amd.torchrl.algo import PPODiscrete
    args = dict(plr=pc.lr_of(case), vlr=pc.lr_of(case), clip_para=CLIP, opt_epochs=3, tau=0.95, shuffle=True, entropy_coeff=ENT,
                env=None, replay_buffer=None, collector=_Coll(), logger=None, device=device, discount=0.99, num_epochs=1500,
                batch_size=case["B"], save_dir=None, clipped_value_loss=bool(case.get("clipped_value_loss", False)))
    args.update(kw)
    return PPODiscrete(pf=pf, vf=vf, **args)


def _up(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)


def _last(pf):
    """weight and bias of the head's last linear layer ([K, k], [K])."""
    keys = [k for k in pf.state_dict() if k.startswith("seq_append_fcs.")]
    return pf.state_dict(keep_vars=True)[keys[-2]], pf.state_dict(keep_vars=True)[keys[-1]]


def _perturb_live_head(pf, K, seed):
    """The live policy moves away from the frozen target: seeded noise of 0.1 rms(W) on the last layer's weight, and on its bias
    +-0.5 (1 + k / K) with alternating sign — the log-ratio of a class against the row's dominant class is then about the
    difference of two such entries, on both sides of log(1 +- clip)."""
    w, b = _last(pf)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        w.add_((0.1 * w.pow(2).mean().sqrt().item() * torch.randn(w.shape, generator=g)).to(w.device))
        b.add_(torch.tensor([0.5 * (-1.0) ** k * (1.0 + k / K) for k in range(K)], dtype=torch.float32, device=b.device))
    pf.mark_params_changed()


def _acts(rs, n, K):
    acts = np.concatenate([np.arange(K)[:min(K, n)], rs.randint(0, K, size=max(0, n - K))])
    return acts[rs.permutation(n)].astype(np.int64)


def _near_edge(r, gap):
    return min(abs(r - EDGES[0]), abs(r - EDGES[1])) < gap


def _steer_acts(acts, ratios, an):
    """Target route: the ratio of row i is ratios[i, acts[i]], set by the two forwards. A row whose ratio lies within 3e-3 of
    1 +- clip takes the next action index whose ratio does not. n = 2: one zero-slope row and one row with a slope, by
    construction (one row takes a class whose ratio is clipped on the side of its advantage's sign, the other one that is not)."""
    n, K = ratios.shape
    acts = acts.copy()
    zero = lambda i, k: (ratios[i, k] > EDGES[1] and an[i] > 0) or (ratios[i, k] < EDGES[0] and an[i] < 0)
    ok = [[k for k in [(acts[i] + d) % K for d in range(K)] if not _near_edge(ratios[i, k], 3e-3)] for i in range(n)]
    assert all(ok), ratios
    if n == 2:
        for clipped in (0, 1):
            pick = [[k for k in ok[i] if zero(i, k) == (i == clipped)] for i in range(2)]
            if all(pick):
                return np.array([pick[0][0], pick[1][0]], dtype=np.int64)
        raise AssertionError("no action pair with one zero-slope row: %s" % (ratios,))
    return np.array([o[0] for o in ok], dtype=np.int64)


def _away(x, points, gap):
    x = x.copy()
    for p in points:
        near = np.abs(x - p) < gap
        x[near] = p + np.where(x[near] >= p, gap, -gap)
    return x


# ------------------------------------------------------------------------------------------ loss stage, teacher-forced
LOSS_NS = (2, 23, 64, 513, 1024)  # the smallest batch, a partial wave, one wave, the 1024-thread block with a tail, a full one
LOSS_SCALE = {2: 850.0, 6: 800.0, 16: 800.0}


def _loss_inputs(pf, tpf, vf, case, n, device, seed, stored):
    """A rollout of n slots around the nets' own outputs (one preliminary forward of each net), like
    tests/test_gpu_loss_adam.py::_inputs: advantages ~ 4 +- 0.05, returns and old values around the critic's output, log pi_old
    = log p0(a) - log r with r log-uniform in [0.3, 3], nudged 3e-3 away from 1 +- clip (stored route: the assertion is on 2e-3), or actions steered away from
    those edges (target route: the ratio comes from the two forwards)."""
    rs = np.random.RandomState(seed)
    K = case["K"]
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float32), device=device)
    net = pf.hip
    net.ensure_bound()
    st, im = net.alloc_rollout(n, device)
    net.ingest(t(util.obs_rows(rs, n, case)), st, im)
    row0 = net.forward(st, im, n)[:, :K].double().cpu().numpy()
    v0 = vf.hip.forward(st, im, n)[:, 0].double().cpu().numpy()
    acts = _acts(rs, n, K)
    advs = np.array([4.05, 3.95]) if n == 2 else 4.0 + 0.05 * rs.randn(n)
    advs = advs.astype(np.float32).astype(np.float64)
    an = ce.adv_norm64(advs)[0]
    logp = np.zeros(n)
    if stored:
        r = _away(np.exp(rs.uniform(np.log(0.3), np.log(3.0), n)), EDGES, 3e-3)
        if n == 2:
            r = np.array([1.5, 1.1])  # row 0 (an > 0): clipped, zero slope; row 1: inside the clip range
        logp = ce.head64(row0, acts)["lp"] - np.log(r)
    else:
        trow0 = tpf.hip.forward(st, im, n)[:, :K].double().cpu().numpy()
        acts = _steer_acts(acts, np.exp(ce.head64(row0)["lg"] - ce.head64(trow0)["lg"]), an)
    rets = v0 + rs.choice([-1.0, 1.0], n) * rs.uniform(0.05, 2.0, n)
    oldv = v0 + rs.uniform(-0.6, 0.6, n)
    arrs = {k: t(v) for k, v in dict(acts=acts.reshape(n, 1), advs=advs, rets=rets, oldv=oldv, logp=logp).items()}
    rows = torch.tensor(rs.permutation(n).astype(np.int32)[None], device=device)
    return st, im, arrs, rows, {k: v.double().cpu().numpy() for k, v in arrs.items()}


def _check_loss_stage(tag, got, inp, rows, K, n, stored):
    """What the launches left against pc.loss_stage64 on the fp32 logits rows the loss launch itself read."""
    sl = rows[0].cpu().numpy()
    pick = {k: v[sl] for k, v in inp.items()}
    gs = got["gs"]
    R = pc.loss_stage64(got["row"], None if stored else got["trow"], pick["logp"] if stored else None, pick["acts"].reshape(n),
                        pick["advs"], K, CLIP, ENT)
    G = pc.loss_stage_gates(R, stored, CLIP, ENT)
    share = R["zero"].mean()
    gap = min(np.abs(R["ratio"] - EDGES[0]).min(), np.abs(R["ratio"] - EDGES[1]).min())
    print("   [%s] zero-slope share %.3f, smallest |ratio - (1 +- clip)| %.4f, ratio in [%.3f, %.3f]"
          % (tag, share, gap, R["ratio"].min(), R["ratio"].max()))
    # conditions on the inputs, from the float64 reference
    assert gap >= pc.RATIO_GAP, (tag, gap)
    if n >= 23:
        assert pc.ZERO_SLOPE_RANGE[0] <= share <= pc.ZERO_SLOPE_RANGE[1], (tag, share)
    if n == 2:
        assert R["zero"].sum() == 1, (tag, R["zero"], R["ratio"], R["an"])
    st, s = got["stats"], R["stats"]
    worst = {}

    def gate(name, err, lim):
        r = ce.ratio(err, lim)
        worst[name] = r
        util.record("ppo_cat/loss_stage/%s/%s_err_over_gate" % (tag, name), r)
        assert r <= 1.0, (tag, name, r)
    for k in ("advs/mean", "advs/std", "Training/policy_loss", "logprob/mean", "logprob/std", "logprob/max", "logprob/min",
              "ratio/max", "ratio/min"):
        gate(k, abs(st[IX[k]] - s[k]), G["stats"][k])
    assert st[IX["advs/max"]] == s["advs/max"] and st[IX["advs/min"]] == s["advs/min"]
    assert all(st[IX[k]] == 0.0 for k in LS_KEYS), [st[IX[k]] for k in LS_KEYS]  # as the opening launch cleared them
    assert st[ST_F16_SAT] == 0.0
    assert np.all(got["dout"][:, K:] == 0.0)  # columns K .. 15: exactly zero
    gate("dz", np.abs(got["dout"][:, :K] / gs - R["dz"]), G["dz"])
    assert np.all((got["dout"][:, :K] != 0.0).any(axis=1) | R["zero"])  # a row with a slope has a gradient
    return worst


@pytest.mark.parametrize("stored", [True, False], ids=["stored_logp", "target_forward"])
@pytest.mark.parametrize("K", [2, 6, 16])
@pytest.mark.parametrize("mode", MODES)
def test_loss_stage_vs_float64(mode, K, stored, device):
    """actor_loss_cat_kernel through the trainer's own launches (begin -> critic_grads -> actor_grads, no step) at n = 2, 23, 64,
    513 and 1024 on a [128, 64] / [72] pair with a common base, against pc.loss_stage64 fed the fp32 logits rows the launches left
    in the workspace: the gate is fp32 rounding only, in every compute mode. Stored route: log pi_old handed in; target route:
    after sync_target the live head's last layer is perturbed with seeded noise and the frozen target's rows are read back too.
    Checks: the d(out) rows, columns K .. 15 exactly zero, every record slot the launch fills, log_std/* and ST_F16_SAT zero."""
    from vision4leg_amd.engine import HipTrainer
    case = dict(pc._SMALL, K=K, B=64, seed=170 + K, shared=True, scale=LOSS_SCALE[K])
    pf, vf = _build(case, mode, device)
    tpf = copy.deepcopy(pf).to(device)
    with torch.cuda.device(device):
        tr = HipTrainer(pf.hip, vf.hip, tpf.hip, max(LOSS_NS), CLIP, ENT)
        tr.sync_target()
        if not stored:
            _perturb_live_head(pf, K, seed=5)
        print("\n[ppo_cat loss stage %s K=%d %s]" % (mode, K, "stored" if stored else "target"))
        for n in LOSS_NS:
            st_, im, arrs, rows, inp = _loss_inputs(pf, tpf, vf, case, n, device, seed=3000 + 17 * K + n, stored=stored)
            ro = HipTrainer.rollout(st_, im, arrs["acts"], arrs["advs"], arrs["rets"], arrs["oldv"], arrs["logp"] if stored else None)
            stats = torch.zeros(1, 24, device=device)
            tr._pre(n)
            tr.begin(rows, stats, 1e-3, 1e-3)
            tr.critic_grads(ro, n)
            tr.actor_grads(ro, n)
            torch.cuda.synchronize()
            got = {"row": pf.hip.ws_view(n, "out", n, 16, tr.ws).double().cpu().numpy(),
                   "dout": pf.hip.ws_view(n, "dout", n, 16, tr.ws).double().cpu().numpy(),
                   "stats": tr.stats_cur().double().cpu().numpy(), "gs": pf.hip.grad_scale(n)}
            if not stored:  # the frozen target's rows: its workspace starts behind the larger of pf's / vf's (v4l_trainer_actor_grads)
                off = max(pf.hip.ws_floats(n), vf.hip.ws_floats(n)) + tpf.hip.ws_offset(n, "out")
                got["trow"] = tr.ws[off:off + n * 16].view(n, 16).double().cpu().numpy()
            tag = "K%d/%s/n%d/%s" % (K, "stored" if stored else "target", n, mode)
            worst = _check_loss_stage(tag, got, inp, rows, K, n, stored)
            print("   n = %4d: worst error / gate %s" % (n, " ".join("%s %.2f" % kv for kv in worst.items())))


# ------------------------------------------------------------------------------------------ updates
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_two_updates(name, mode, device):
    """tests/test_gpu_sd.py::test_two_updates on these cases, its bounds number for number: the 14 infos and every parameter of
    pf and vf after each PPODiscrete.update (host batches: the target-policy route) against the same-mode restatement; in f32 also
    against the reference's fixture for the fixture case; Adam steps counted on both optimisers; nothing saturates in f16.
    (That function's one statement against the fp32 FIXTURE in f16 mode — first update within 1e-3 — is not a statement about the
    same-mode restatement and is not carried over: on the sharpened head the f16 restatement itself lies 1.1e-3 from the fp32
    reference in ratio/min, 0.976224 against 0.977340, and the engine 7e-6 from the f16 restatement.)"""
    case = PPO_CAT_CASES[name]
    n_updates, lr = pc.updates_of(case), pc.lr_of(case)
    pf, vf = _build(case, mode, device)
    assert (vf.base is pf.base) == case["shared"]
    agent = _agent(pf, vf, case, device)
    oracle = pc.oracle_of(pf.state_dict(), vf.state_dict(), case, mode)
    gold = util.load_golden(pc.FIXTURE) if name == pc.FIXTURE_CASE else None
    ref32 = pc.oracle_of(pf.state_dict(), vf.state_dict(), case, "f32") if gold is None and mode != "f32" else None
    agent.trainer.sync_target()
    for u in range(n_updates):
        before = {k: v.detach().cpu().clone() for k, v in pf.state_dict().items()}
        args = pc.batch_tensors(case, u) + (lr, lr)
        info = agent.update(pc.host_batch(case, u))
        oinfo = oracle.update(*args)
        ginfo = dict(zip(pc.INFO_KEYS, gold["u%d/info" % u])) if gold is not None else ref32.update(*args) if ref32 else None
        assert list(info) == pc.INFO_KEYS
        print("\n[%s %s] update %d info (hip / restatement):" % (name, mode, u))
        for k in pc.INFO_KEYS:
            print("   %-22s % .6f % .6f" % (k, info[k], oinfo[k]))
        assert np.isfinite([info[k] for k in pc.INFO_KEYS]).all()
        for k in pc.INFO_KEYS:
            tol = (5e-4 if mode == "f32" else 5e-3) * max(1.0, abs(oinfo[k]))
            strict_ok = abs(info[k] - oinfo[k]) <= tol
            if mode != "f32" and u >= 1 and k in EITHER_OR:
                assert strict_ok or abs(info[k] - ginfo[k]) <= 5e-2 * max(1.0, abs(ginfo[k])), (u, k, info[k], oinfo[k], ginfo[k])
                continue
            assert strict_ok, (u, k, info[k], oinfo[k])
            if mode == "f32" and gold is not None:
                assert abs(info[k] - ginfo[k]) <= tol, (u, k, info[k], ginfo[k])
        worst, tot, cnt = 0.0, 0.0, 0
        for tag, net, onet in (("pf", pf, oracle.pf), ("vf", vf, oracle.vf)):
            for k, v in net.state_dict().items():
                dd = (v.detach().cpu() - onet[k]).abs()
                worst = max(worst, dd.max().item())
                tot += dd.sum().item(); cnt += dd.numel()
                assert dd.max().item() <= (2e-5 if mode == "f32" else 2.2e-4 * (u + 1)), (u, tag, k, dd.max().item())
                if mode == "f32" and gold is not None and ("u%d/%s/%s" % (u, tag, k)) in gold.files:
                    assert np.abs(v.detach().cpu().numpy() - gold["u%d/%s/%s" % (u, tag, k)]).max() <= 2e-5, (u, tag, k)
        util.record("ppo_cat/update/%s/%s/u%d/worst_abs_param_vs_oracle" % (name, mode, u), worst)
        print("   worst |param - restatement| %.3e, mean %.3e" % (worst, tot / cnt))
        assert tot / cnt <= (1e-7 if mode == "f32" else 2e-5 * (u + 1))
        assert max((pf.state_dict()[k].cpu() - before[k]).abs().max().item() for k in before) > 5e-5  # the optimiser stepped
        assert agent.trainer.adam_steps() == (u + 1, u + 1) and agent.training_update_num == u + 1
    assert agent.f16_saturated == 0


def test_against_reference_fixture(device):
    """f32 mode against what the unmodified reference's PPO logged and stepped to (tests/golden/ppo_cat_mlp.npz):
    tests/test_gpu_cat.py::test_against_reference_fixture's bounds."""
    case = PPO_CAT_CASES[pc.FIXTURE_CASE]
    gold = util.load_golden(pc.FIXTURE)
    pf, vf = _build(case, "f32", device)
    agent = _agent(pf, vf, case, device)
    agent.trainer.sync_target()
    for u in range(2):
        info = agent.update(pc.host_batch(case, u))
        assert list(info) == pc.INFO_KEYS
        for k, want in zip(pc.INFO_KEYS, gold["u%d/info" % u]):
            assert abs(info[k] - want) <= 5e-4 * max(1.0, abs(want)), (u, k, info[k], want)
        seen = 0
        for tag, net in (("pf", pf), ("vf", vf)):
            for k, v in net.state_dict().items():
                key = "u%d/%s/%s" % (u, tag, k)
                if key in gold.files:
                    seen += 1
                    assert np.abs(v.detach().cpu().numpy() - gold[key]).max() <= 2e-5, (u, tag, k)
        assert seen >= 4


# ------------------------------------------------------------------------------------------ the two log pi_old routes
@pytest.mark.parametrize("mode", MODES)
def test_stored_logp_equals_target_route(mode, device):
    """The same batch (ppo_cat_mlp's geometry, n = 64, the live head perturbed after sync_target) through a rollout with stored
    log pi — taken from the frozen target's head via v4l_cat_head — and through the target route: the records and the d(out) rows
    the backward consumes agree to fp32 rounding of the log-softmax. The gate, derived here: both log pi_old values are fp32
    log-softmaxes of the target's logits rows at the action, each within cat_edge_cases.head_gates' |d lg| of the exact one — and
    2-Lipschitz in the rows, should the two forwards of the frozen target differ at all — so
      |d lpo| <= 2 |d lg| + 2 max_j |d row_j| =: e;   rel(ratio) <= e + 2 u;   |d dz_j| <= |A_j| (e + 4 u), A_j = dlp (hit - p_j)
    (the entropy term does not see lpo); ratio/* within ratio (e + 2 u), policy_loss within mean(ratio |an| e) + 8 u of its
    magnitudes; log pi itself, the advantage statistics and the critic's slots do not depend on the route: equal bits."""
    from vision4leg_amd.engine import HipTrainer
    case = PPO_CAT_CASES["ppo_cat_mlp"]
    K, n, u = case["K"], case["B"], ce.EPS32
    pf, vf = _build(case, mode, device)
    tpf = copy.deepcopy(pf).to(device)
    with torch.cuda.device(device):
        tr = HipTrainer(pf.hip, vf.hip, tpf.hip, n, CLIP, ENT)
        tr.sync_target()
        _perturb_live_head(pf, K, seed=6)
        b = pc.host_batch(case, 0)
        net = pf.hip
        st, im = net.alloc_rollout(n, device)
        net.ingest(_up(b["obs"], device), st, im)
        row0 = net.forward(st, im, n)[:, :K].double().cpu().numpy()
        tout = tpf.hip.forward(st, im, n)
        trow0 = tout[:, :K].double().cpu().numpy()
        advs = np.asarray(b["advs"], dtype=np.float32).astype(np.float64).reshape(n)
        acts = _steer_acts(np.asarray(b["acts"]), np.exp(ce.head64(row0)["lg"] - ce.head64(trow0)["lg"]), ce.adv_norm64(advs)[0])
        acts_t = _up(acts.reshape(n, 1), device)
        logp = tpf.hip.cat_head(tout, n, acts_t)[2].clone()
        arrs = [acts_t, _up(b["advs"], device).reshape(n), _up(b["estimate_returns"], device).reshape(n), _up(b["values"], device).reshape(n)]
        out = {}
        for route_, lp_old in (("stored", logp), ("target", None)):
            ro = HipTrainer.rollout(st, im, *arrs, lp_old)
            stats = torch.zeros(1, 24, device=device)
            tr._pre(n)
            tr.begin(None, stats, 1e-3, 1e-3)
            tr.critic_grads(ro, n)
            tr.actor_grads(ro, n)
            torch.cuda.synchronize()
            out[route_] = {"stats": tr.stats_cur().double().cpu().numpy(), "row": pf.hip.ws_view(n, "out", n, 16, tr.ws).double().cpu().numpy(),
                           "dout": pf.hip.ws_view(n, "dout", n, 16, tr.ws).double().cpu().numpy() / pf.hip.grad_scale(n)}
        off = max(pf.hip.ws_floats(n), vf.hip.ws_floats(n)) + tpf.hip.ws_offset(n, "out")
        trow = tr.ws[off:off + n * 16].view(n, 16).double().cpu().numpy()
    a, t = out["stored"], out["target"]
    assert np.array_equal(a["row"], t["row"])  # one live policy, one forward kernel
    R = pc.loss_stage64(t["row"], trow, None, acts, advs, K, CLIP, ENT)
    gap = min(np.abs(R["ratio"] - EDGES[0]).min(), np.abs(R["ratio"] - EDGES[1]).min())
    assert gap >= pc.RATIO_GAP and 0 < R["zero"].sum() < n, (gap, R["zero"].sum())
    e = 2 * ce.head_gates(R["th"])["lg"][R["hit"] > 0] + 2 * np.abs(trow[:, :K] - trow0).max(axis=1)
    ratio, an = R["ratio"], np.abs(R["an"])
    A = np.abs(R["dlp"])[:, None] * np.abs(R["hit"] - R["p"])
    r_dz = ce.ratio(np.abs(a["dout"][:, :K] - t["dout"][:, :K]), A * (e + 4 * u)[:, None] + 1e-30)
    r_rmax = ce.ratio(abs(a["stats"][IX["ratio/max"]] - t["stats"][IX["ratio/max"]]), np.max(ratio * (e + 2 * u)))
    r_rmin = ce.ratio(abs(a["stats"][IX["ratio/min"]] - t["stats"][IX["ratio/min"]]), np.max(ratio * (e + 2 * u)))
    r_loss = ce.ratio(abs(a["stats"][IX["Training/policy_loss"]] - t["stats"][IX["Training/policy_loss"]]),
                      np.mean(ratio * an * e) + 8 * u * (np.mean(ratio * an) + ENT * np.mean(R["H"])))
    print("\n[stored vs target %s] difference / gate: d(out) %.3f ratio/max %.3f ratio/min %.3f policy_loss %.3f; target rows of the two "
          "forwards differ by %.1e" % (mode, r_dz, r_rmax, r_rmin, r_loss, np.abs(trow[:, :K] - trow0).max()))
    assert max(r_dz, r_rmax, r_rmin, r_loss) <= 1.0
    assert np.all(a["dout"][:, K:] == 0) and np.all(t["dout"][:, K:] == 0)
    for k in util.STAT_KEYS:
        if k not in ("ratio/max", "ratio/min", "Training/policy_loss", "grad_norm/pf", "grad_norm/vf"):
            assert a["stats"][IX[k]] == t["stats"][IX[k]], k


# ------------------------------------------------------------------------------------------ graphs and launches
def _digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def _device_run(agent, pf, batches, device, stored, categorical=True):
    """A device rollout of the given host minibatches for agent.run_updates -> (ro, rowidx). stored: with log pi_old — of the
    (synchronised) target's head at the stored actions (v4l_cat_head); for a Gaussian policy (the launch count's twin) a constant."""
    from vision4leg_amd.engine import HipTrainer
    U, n = len(batches), len(batches[0]["advs"])
    hip = pf.hip
    hip.ensure_bound()
    st, im = hip.alloc_rollout(U * n, device)
    hip.ingest(_up(np.concatenate([b["obs"] for b in batches]), device), st, im)
    cat = lambda k: _up(np.concatenate([b[k] for b in batches]), device)
    acts_t = cat("acts").reshape(U * n, -1)
    logp = None
    if stored and categorical:
        thip = agent.target_pf.hip
        logp = thip.cat_head(thip.forward(st, im, U * n), U * n, acts_t)[2].clone()
    elif stored:
        logp = torch.full((U * n,), -1.0, device=device)
    ro = HipTrainer.rollout(st, im, acts_t, cat("advs").reshape(-1), cat("estimate_returns").reshape(-1), cat("values").reshape(-1), logp)
    rowidx = torch.arange(U * n, dtype=torch.int32, device=device).view(U, n).flip(0).contiguous()
    return ro, rowidx


def _run_twice(case, device, stored, U=3):
    pf, vf = _build(case, "f16", device)
    agent = _agent(pf, vf, case, device)
    out = []
    with torch.cuda.device(device):
        agent.trainer.sync_target()
        ro, rowidx = _device_run(agent, pf, [pc.host_batch(case, u) for u in range(U)], device, stored)
        for _ in range(2):
            stats = torch.zeros(U, 24, dtype=torch.float32, device=device)
            agent.run_updates(ro, rowidx, stats)
            torch.cuda.synchronize()
            tr = agent.trainer
            out.append((stats.cpu().clone(), _digest(list(pf.state_dict().values()) + list(vf.state_dict().values())
                                                      + [tr.m_pf, tr.v_pf, tr.m_vf, tr.v_vf])))
        assert agent.trainer.adam_steps() == (2 * U, 2 * U)
    return out


@pytest.mark.parametrize("stored", [True, False], ids=["stored_logp", "target_forward"])
def test_run_equals_eager(stored, device, monkeypatch):
    """U = 3 updates twice (f16, ppo_cat_mlp, PPO.run_updates on a device rollout): the graphed epoch (the second run replays the
    whole run as one hipGraph), one replay per update (V4L_EPOCH_GRAPH=0) and eager launches (V4L_GRAPH=0) leave identical bits in
    parameters, moments and records: actor_loss_cat_kernel reduces in a fixed order, without float atomics."""
    case = PPO_CAT_CASES["ppo_cat_mlp"]
    runs = []
    for env in (dict(), dict(V4L_EPOCH_GRAPH="0"), dict(V4L_GRAPH="0")):
        for k in ("V4L_EPOCH_GRAPH", "V4L_GRAPH"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        runs.append(_run_twice(case, device, stored))
    base = runs[0]
    assert all(np.isfinite(s.numpy()[:, :18]).all() for s, _ in base) and base[0][1] != base[1][1]
    assert (base[1][0][:, [IX[k] for k in LS_KEYS]] == 0).all() and (base[1][0][:, ST_F16_SAT] == 0).all()
    for other in runs[1:]:
        for r in range(2):
            assert torch.equal(base[r][0], other[r][0]), r
            assert base[r][1] == other[r][1], r


@pytest.mark.parametrize("kind", ["host", "resident"])
def test_launch_count(kind, device):
    """An update of PPODiscrete launches what a GaussianContPolicy PPO update of the same geometry (sd_cases' sd_mlp: S = 93,
    [256, 256] / [256, 256], B = 64, vf.base = pf.base) launches on the same buffer kind — host batches: the frozen target's
    forward runs; resident: stored log pi, it does not —: the same labels with the same call counts, read from the library's
    profiler for both (no literal). The categorical loss takes the Gaussian loss launch's position and adds none."""
    import test_gpu_sd as tsd
    case, g = PPO_CAT_CASES["ppo_cat_mlp"], sc.SD_CASES["sd_mlp"]
    assert (g["S"], g["enc"], g["head"], g["B"]) == (case["S"], case["enc"], case["head"], case["B"])

    def profile(agent, pf, batches, categorical):
        agent.trainer.sync_target()
        if kind == "host":
            agent.update(batches[0])
            return route._profiled(lambda: agent.update(batches[1]))
        ro, rowidx = _device_run(agent, pf, batches, device, True, categorical)
        stats = torch.zeros(1, 24, dtype=torch.float32, device=device)
        agent.run_updates(ro, rowidx[:1].contiguous(), stats)
        return route._profiled(lambda: agent.run_updates(ro, rowidx[1:].contiguous(), stats))

    def both():
        gpf, gvf = tsd._build(g, "f16", device)
        gauss = profile(tsd._ppo(gpf, gvf, g, device), gpf, [sc.host_batch(g, u) for u in range(2)], False)
        pf, vf = _build(case, "f16", device)
        return gauss, profile(_agent(pf, vf, case, device), pf, [pc.host_batch(case, u) for u in range(2)], True)
    with torch.cuda.device(device):
        gauss, cat = route._with_env("f16", {}, both)
    calls = lambda rows: sum(r[1] for r in rows)
    print("\n[%s] launches per update: GaussianContPolicy PPO %d, PPODiscrete %d: %s" % (kind, calls(gauss), calls(cat), [r[:2] for r in cat]))
    assert calls(cat) == calls(gauss) > 0
    assert [r[:2] for r in cat] == [r[:2] for r in gauss]
    assert [r[1] for r in cat if r[0].endswith("|actor_loss")] == [1]  # one loss launch: actor_loss_cat_kernel's


# ------------------------------------------------------------------------------------------ training loop
LOOP_CASE = dict(PPO_CAT_CASES["ppo_cat_k16"], B=32, lr=pc.LR)


def _loop_agent(device, buffer, shared, save_dir, E, T, B, num_epochs):
    from vision4leg_amd.torchrl.algo import PPODiscrete
    from vision4leg_amd.torchrl.collector import VecOnPolicyCollector
    from vision4leg_amd.torchrl.replay_buffers import DeviceOnPolicyReplayBuffer, OnPolicyReplayBuffer
    case = dict(LOOP_CASE, shared=shared)
    pf, vf = _build(case, "f16", device)
    env = tgc.DiscreteFakeVecEnv(E, case["S"], case["K"], seed=9, p_done=0.12)
    eval_env = tgc.DiscreteFakeVecEnv(E, case["S"], case["K"], seed=1, p_done=0.3)
    cls = DeviceOnPolicyReplayBuffer if buffer == "device" else OnPolicyReplayBuffer
    buf = cls(max_replay_buffer_size=E * T, env_nums=E, time_limit_filter=True)
    coll = VecOnPolicyCollector(vf, env=env, eval_env=eval_env, pf=pf, replay_buffer=buf, device=device, epoch_frames=E * T)
    assert coll.fast_path == (buffer == "device") and coll.continuous is False
    agent = PPODiscrete(pf=pf, vf=vf, plr=pc.LR, vlr=pc.LR, clip_para=CLIP, opt_epochs=2, tau=0.95, shuffle=True, entropy_coeff=ENT,
                        env=None, replay_buffer=buf, collector=coll, logger=rsm._Log(), device=device, discount=0.99,
                        num_epochs=num_epochs, batch_size=B, save_interval=1, eval_interval=1, save_dir=save_dir)
    return agent, pf, env, eval_env


@pytest.mark.parametrize("shared", [False, True], ids=["no_common_parameter", "common_base"])
def test_train_loop_buffers(shared, device, tmp_path, monkeypatch):
    """train() over tests/test_gpu_cat.py's discrete vec env (action_space.n = 16, E = 4), T = 16, B = 32, two epochs with
    opt_epochs = 2, f16, on the resident buffer (the rollout step files [E][1] action rows and log pi_old: the stored route) and
    on the host buffer (the target-policy route): parameters move, the logger gets the 14 keys, every stored log pi is finite and
    <= 0, the env only ever sees int64 actions in [0, K). On the resident buffer the first update of an epoch has theta = target,
    so ratio/max and ratio/min measure how far the rollout step's log pi and the update's differ: within exp(+-0.01), the 0.01
    under which tests/test_gpu_kl_stop.py holds an epoch's opening approx_kl — for the pair without a common parameter. With a
    common base the critic's step, taken first, moves the policy's trunk before its forward (the reference's own fixture logs
    ratio/max = 1.0206 in its first update): no rollout-versus-update bound applies, the ratios are held to bracket 1."""
    monkeypatch.setenv("V4L_COMPUTE", "f16")
    E, T, B = 4, 16, 32
    U = 2 * (E * T // B)
    for buffer in ("device", "host"):
        np.random.seed(3); torch.manual_seed(3); torch.cuda.manual_seed(3)
        agent, pf, env, eval_env = _loop_agent(device, buffer, shared, str(tmp_path / buffer), E, T, B, 2)
        assert (agent.vf.base is agent.pf.base) == shared
        before = {k: v.detach().cpu().clone() for k, v in pf.state_dict().items()}
        agent.train()
        assert len(agent.logger.updates) == 2 * U and len(agent.logger.epochs) == 2 and agent.f16_saturated == 0
        assert len(env.log) == 2 * T and len(eval_env.log) > 0 and env.closed
        assert agent.trainer.adam_steps() == (2 * U, 2 * U)
        assert max((pf.state_dict()[k].cpu() - before[k]).abs().max().item() for k in before) > 5e-5
        for x in agent.logger.updates:
            assert list(x) == pc.INFO_KEYS and len(x) == 14 and np.isfinite(list(x.values())).all()
        if buffer == "device":
            buf = agent.replay_buffer
            assert tuple(buf._acts_dev.shape) == (T * E, 1) and buf._acts_dev.min().item() >= 0 and buf._acts_dev.max().item() < LOOP_CASE["K"]
            logp = buf.device_rollout()[6]
            assert logp is not None and bool(torch.isfinite(logp).all()) and logp.max().item() <= 0.0
            for epoch in range(2):
                first = agent.logger.updates[epoch * U]
                print("\n[ppo_cat train loop %s] epoch %d first update: ratio/max %.6f ratio/min %.6f"
                      % ("shared" if shared else "sep", epoch, first["ratio/max"], first["ratio/min"]))
                assert 0.0 < first["ratio/min"] <= 1.0 + 1e-6 and first["ratio/max"] >= 1.0 - 1e-6, first
                if not shared:
                    assert np.exp(-0.01) <= first["ratio/min"] <= first["ratio/max"] <= np.exp(0.01), first
        else:
            buf = agent.replay_buffer
            assert tuple(buf._acts.shape) == (T, E) and (buf._acts == np.round(buf._acts)).all()


# ------------------------------------------------------------------------------------------ refusals that stay
def test_c_refusals_that_stay(device):
    """v4l_trainer_vmpo, v4l_trainer_kl_stop and v4l_trainer_kl_adapt (so the armed update entry points too) still refuse a net
    flagged by v4l_net_set_categorical: their log pi_old code is Gaussian. The PPO entry points take it."""
    from vision4leg_amd.engine import HipTrainer
    case = PPO_CAT_CASES["ppo_cat_k16"]
    n = case["B"]
    pf, vf = _build(case, "f32", device)
    tpf = copy.deepcopy(pf).to(device)
    b = pc.host_batch(case, 0)
    with torch.cuda.device(device):
        tr = HipTrainer(pf.hip, vf.hip, tpf.hip, n, CLIP, ENT)
        tr.sync_target()
        st, im = pf.hip.alloc_rollout(n, device)
        pf.hip.ingest(_up(b["obs"], device), st, im)
        ro = HipTrainer.rollout(st, im, _up(b["acts"], device).reshape(n, 1), _up(b["advs"], device).reshape(n),
                                _up(b["estimate_returns"], device).reshape(n), _up(b["values"], device).reshape(n))
        stats = torch.zeros(1, 24, device=device)
        tr._pre(n)
        tr.begin(None, stats, 1e-4, 1e-4)
        with pytest.raises(RuntimeError, match="v4l_trainer_kl_stop: the KL early stop belongs to the PPO update, which takes Gaussian"):
            tr.kl_arm(torch.zeros(1, 2, device=device), 0.01)
        with pytest.raises(RuntimeError, match="v4l_trainer_kl_adapt: the adaptive rates belong to the PPO update, which takes Gaussian"):
            tr.kl_adapt_arm(torch.zeros(1, 4, device=device), 0.01)
        with pytest.raises(RuntimeError, match="v4l_trainer_kl_update: arm the run first"):  # (and arming is refused)
            tr.kl_update_next(ro, n, graph=False)
        with pytest.raises(RuntimeError, match="v4l_trainer_kl_adapt_update"):
            tr.kl_adapt_update_next(ro, n, graph=False)
        tr.vmpo_init()
        with pytest.raises(RuntimeError, match="v4l_trainer_vmpo: a categorical policy"):
            tr.vmpo_actor_grads(ro, n)
        with pytest.raises(RuntimeError, match="v4l_trainer_vmpo: a categorical policy"):
            tr.vmpo_update_next(ro, n, None, graph=False)
        # ... and the PPO update of the same trainer runs
        tr.begin(None, stats, 1e-4, 1e-4)
        tr.update_next(ro, n, graph=False)
        torch.cuda.synchronize()
        rec = stats[0].cpu().numpy()
    assert np.isfinite(rec[:18]).all() and rec[IX["ratio/max"]] > 0 and all(rec[IX[k]] == 0 for k in LS_KEYS)
