"""-m gpu: the state-MLP net with Tanh activations (tests/tact_cases.py) on the HIP engine: forward and Gaussian head,
gradients, two PPO updates, saturated units, the rollout step on every route the kind takes, the kernel routes against the
ReLU net's recorded tables, and the training loop with checkpoint / resume.

The reference arithmetic is tact_cases.tact_forward (pinned to the unmodified reference by tests/golden/make_golden_tact.py and
tests/test_tact_cpu.py). Tolerances are the rules of tests/test_gpu_parity.py (its module docstring) and the bounds of
tests/test_gpu_wide_actions.py::test_two_updates / test_rollout_step, imported or restated, none of them new.

mlp_tact_b300 runs two updates in every mode: on the CPU, the 16-bit restatement run again with its parameters nudged by 3e-6
(three seeds) stays inside test_two_updates' bounds after the second update too (worst parameter 4.3e-5 bf16 / 8.6e-6 f16 of
4.4e-4, infos 5.0e-4 of 5e-3)."""
import os

import numpy as np
import pytest
import torch

import test_gpu_parity as par
import test_gpu_resume as rsm
import test_gpu_rollout_route as rollout_route
import test_gpu_update_route as route
import test_gpu_wide_actions as wide
import util
from oracle import ppo_oracle as orc
from tact_cases import FIXTURE_CASES, SATURATION, TACT_CASES, tact_forward

pytestmark = pytest.mark.gpu

MODES = par.MODES
NAMES = list(TACT_CASES)


def _policy_params(opf):
    return {k: v for k, v in opf.items() if k != "logstd"}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_forward_and_gauss_head(name, mode, device):
    """tests/test_gpu_wide_actions.py::test_forward_and_gauss_head's statements: mean against the same-mode restatement (f32 gate
    / the restatement's own envelope), value likewise, the fixture distance for mlp_tact, std / log-prob / entropy."""
    case = TACT_CASES[name]
    A, tanh = case["A"], case["kind"].endswith("_tanh")
    pf, vf = par._build(case, mode, device)
    b = util.make_batch(case)
    obs = torch.tensor(b["obs"], dtype=torch.float32)
    acts = torch.tensor(b["acts"], dtype=torch.float32)
    mean, std, log_std = pf(obs.to(device))
    value = vf(obs.to(device))
    up = pf.update(obs.to(device), acts.to(device))
    opf, ovf = par._oracle_params(pf, vf, case["kind"])
    pm = _policy_params(opf)
    with torch.no_grad():
        om = orc.FORWARDS[case["kind"]](pm, obs, case["S"], mode)
        ov = orc.FORWARDS[case["kind"]](ovf, obs, case["S"], mode)
        relu = orc.mlp_forward(pm, obs, case["S"], mode)
    em, ev = util.rel_err(mean.cpu(), om), util.rel_err(value.cpu(), ov)
    print("\n[%s %s] rel err vs %s-restatement: mean %.2e value %.2e (the ReLU oracle is %.2e away)"
          % (name, mode, mode, em, ev, util.rel_err(relu, om)))
    util.record("tact/forward/%s/%s/mean_vs_oracle" % (name, mode), em)
    util.record("tact/forward/%s/%s/value_vs_oracle" % (name, mode), ev)
    if mode == "f32":
        assert em < par.TOL[mode] and ev < par.TOL[mode]
    else:
        env_m = wide._forward_envelope(name + "/pf", mode, pm, obs, case)
        env_v = wide._forward_envelope(name + "/vf", mode, ovf, obs, case)
        util.record("tact/forward/%s/%s/mean_envelope_p95" % (name, mode), env_m)
        assert em <= max(par.ENV_FACTOR * env_m, par.ENV_FLOOR), (em, env_m)
        assert ev <= max(par.ENV_FACTOR * env_v, par.ENV_FLOOR), (ev, env_v)
    if name in FIXTURE_CASES:
        gold = util.load_golden("ppo_" + name)
        gm, gv = util.rel_err(mean.cpu(), gold["fwd_mean"]), util.rel_err(value.cpu(), gold["fwd_value"])
        print("   vs the reference's fixture: mean %.2e value %.2e" % (gm, gv))
        assert gm < (par.TOL["f32"] if mode == "f32" else par.REF_DIST[mode]), gm
        assert gv < (par.TOL["f32"] if mode == "f32" else par.REF_DIST[mode]), gv
    assert tuple(mean.shape) == tuple(std.shape) == (case["B"], A) and tuple(log_std.shape) == (A,)
    assert tuple(value.shape) == (case["B"], 1)
    _, ostd, ols = orc.gaussian(om, opf["logstd"])
    assert torch.allclose(std.cpu(), ostd) and torch.allclose(log_std.cpu(), ols)
    lp, ent = orc.log_prob_entropy(mean.cpu(), std.cpu(), acts, tanh_action=tanh)
    assert torch.allclose(up["log_prob"].cpu(), lp, rtol=1e-5, atol=1e-5) and torch.allclose(up["ent"].cpu(), ent, atol=1e-6)


def _hip_grads(net, obs, w, A, device):
    """-> ({name: gradient of sum(out * w)}, the engine's head output) through HipNet.forward(train) + backward."""
    hip, n = net.hip, obs.shape[0]
    st, im, _ = hip.stage(obs.to(device))
    out = hip.forward(st, im, n, train=True)[:, :A].cpu().clone()
    dout = torch.zeros(n, 16, dtype=torch.float32, device=device)
    dout[:, :A] = w.to(device)
    # NaN-filled: the backward pass must WRITE every element (the trainer does not clear its gradient buffers)
    grads = torch.full((hip.total_params,), float("nan"), dtype=torch.float32, device=device)
    hip.backward(st, im, n, dout, grads)
    if "logstd" in hip.param_names:
        hip.grad_view(grads, "logstd").zero_()  # the policy's logstd gradient comes from the loss kernel
    assert not torch.isnan(grads).any(), "backward left gradient elements unwritten"
    return {k: hip.grad_view(grads, k).cpu().clone() for k in hip.param_names if k != "logstd"}, out


def _check_gradients(name, case, mode, device):
    """tests/test_gpu_parity.py::test_backward's rule: the f32 gate; in the 16-bit modes every tensor <= ENV_FACTOR x the p95
    envelope, the flat gradient cosine >= COS_MIN and relative L2 <= L2_FACTOR x the envelope's."""
    pf, vf = par._build(case, mode, device)
    obs = torch.tensor(util.make_batch(case)["obs"], dtype=torch.float32)
    opf, ovf = par._oracle_params(pf, vf, case["kind"])
    bad = []
    for tag, net, op, A in (("pf", pf, _policy_params(opf), case["A"]), ("vf", vf, ovf, 1)):
        w = torch.tensor(np.random.RandomState(5).randn(case["B"], A), dtype=torch.float32)
        got, _ = _hip_grads(net, obs, w, A, device)
        assert net.hip.last_grad_scale == orc.probe_scale(mode, float(w.abs().max()))
        keys = list(op)
        q = {k: v.detach().clone().requires_grad_(True) for k, v in op.items()}
        out = orc.FORWARDS[case["kind"]](q, obs, case["S"], mode)
        ref = dict(zip(keys, par._grad((out * w).sum(), [q[k] for k in keys], mode, float(w.abs().max()))))
        if mode != "f32":
            env = par._bf16_envelope(name, tag, case["kind"], op, obs, case["S"], w, mode=mode)
            fh, fo = par._flat(got, keys), par._flat(ref, keys)
            cos = float((fh @ fo) / (fh.norm() * fo.norm()))
            l2 = float((fh - fo).norm() / fo.norm())
            print("\n[%s %s %s] flat gradient: cos %.7f, rel L2 %.2e (envelope p95 %.2e)" % (name, mode, tag, cos, l2, env["l2"]))
            if cos < par.COS_MIN:
                bad.append((tag, "<flat>", "cosine %.6f" % cos))
            if l2 > max(par.L2_FACTOR * env["l2"], par.ENV_FLOOR):
                bad.append((tag, "<flat>", "relative L2 %.2e > %.1f x envelope %.2e" % (l2, par.L2_FACTOR, env["l2"])))
        worst = 0.0
        for k in keys:
            e = util.rel_err(got[k], ref[k])
            worst = max(worst, e)
            if mode == "f32":
                if e >= par.TOL[mode]:
                    bad.append((tag, k, "%.2e" % e))
            elif e > max(par.ENV_FACTOR * env["tensor"][k], par.ENV_FLOOR):
                bad.append((tag, k, "%.2e > %.0f x envelope %.2e" % (e, par.ENV_FACTOR, env["tensor"][k])))
        print("\n[%s %s %s] worst grad rel err %.2e" % (name, mode, tag, worst))
        util.record("tact/backward/%s/%s/%s/worst_grad_vs_oracle" % (name, mode, tag), worst)
    assert not bad, bad


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_gradients(name, mode, device):
    """Parameter gradients of sum(out * w) for pf and vf against autograd on the restatement (1 - a^2 in the data-grad epilogues:
    gemm_nt for B < 256, gemm_nt_deep for mlp_tact_b300)."""
    _check_gradients(name, TACT_CASES[name], mode, device)


@pytest.mark.parametrize("mode", MODES)
def test_gradients_deep_gemm_ragged_rows(mode, device, monkeypatch):
    """mlp_tact_rag again with the deep kernel's row threshold lowered to 16: gemm_nt_deep_kernel's vector and scalar epilogues
    (widths 128 / 64 / 72 / 45) on a ragged 22-row batch."""
    monkeypatch.setenv("V4L_GEMM_DEEP_MIN_M", "16")
    _check_gradients("mlp_tact_rag", TACT_CASES["mlp_tact_rag"], mode, device)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_two_updates(name, mode, device):
    """tests/test_gpu_wide_actions.py::test_two_updates' statements and bounds: 18 infos and every parameter of pf and vf after
    each of two PPO.update calls (the hipGraph epoch included), against the same-mode restatement; the fp32 reference value of
    the either-or rule is the reference's own fixture for mlp_tact and the fp32 restatement elsewhere."""
    from vision4leg_amd.torchrl.algo import PPO
    case = TACT_CASES[name]
    pf, vf = par._build(case, mode, device)

    class Coll: epoch_frames = 1
    agent = PPO(pf=pf, vf=vf, plr=1e-4, vlr=1e-4, clip_para=0.2, opt_epochs=3, tau=0.95, shuffle=True, entropy_coeff=0.005,
                env=None, replay_buffer=None, collector=Coll(), logger=None, device=device, discount=0.99, num_epochs=1500,
                batch_size=case["B"], save_dir=None)
    opf, ovf = par._oracle_params(pf, vf, case["kind"])
    oracle = orc.PPOOracle(case["kind"], opf, ovf, {k: v.clone() for k, v in opf.items()}, case["S"], mode)
    oracle.sync_target()
    gold = util.load_golden("ppo_" + name) if name in FIXTURE_CASES else None
    ref32 = None
    if gold is None and mode != "f32":
        rpf, rvf = par._oracle_params(pf, vf, case["kind"])
        ref32 = orc.PPOOracle(case["kind"], rpf, rvf, {k: v.clone() for k, v in rpf.items()}, case["S"], "f32")
        ref32.sync_target()
    agent.trainer.sync_target()
    t = lambda a: torch.tensor(a, dtype=torch.float32)
    for u in range(2):
        b = util.make_batch(case, update=u)
        before = {k: v.detach().cpu().clone() for k, v in pf.state_dict().items()}
        args = (t(b["obs"]), t(b["acts"]), t(b["advs"]), t(b["estimate_returns"]), t(b["values"]), 1e-4, 1e-4)
        info = agent.update({k: b[k] for k in ("obs", "acts", "advs", "estimate_returns", "values")})
        oinfo = oracle.update(*args)
        ginfo = dict(zip(util.STAT_KEYS, gold["u%d/info" % u])) if gold is not None else ref32.update(*args) if ref32 else None
        print("\n[%s %s] update %d info (hip / restatement):" % (name, mode, u))
        for k in util.STAT_KEYS:
            print("   %-22s % .6f % .6f" % (k, info[k], oinfo[k]))
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
        util.record("tact/ppo_update/%s/%s/u%d/worst_abs_param_vs_oracle" % (name, mode, u), worst)
        util.record("tact/ppo_update/%s/%s/u%d/max_info_rel_vs_oracle" % (name, mode, u),
                    max(abs(info[k] - oinfo[k]) / max(1.0, abs(oinfo[k])) for k in util.STAT_KEYS))
        assert tot / cnt <= (1e-7 if mode == "f32" else 2e-5 * (u + 1))
        assert max((pf.state_dict()[k].cpu() - before[k]).abs().max().item() for k in before) > 5e-5  # the optimiser stepped
        assert (pf.state_dict()["logstd"].cpu() - before["logstd"]).abs().min().item() > 0
    assert agent.f16_saturated == 0


SATURATION_FACTOR = 32.0  # base.seq_fcs.0.weight x 32: 42 % of mlp_tact's (row, unit) pre-activations pass 9.02 (float64, below)


@pytest.mark.parametrize("mode", MODES)
def test_saturated_units(mode, device):
    """mlp_tact with its first layer's weight scaled until a large share of the layer-1 units saturate: fp32 tanh is exactly
    +-1 there and the backward factor 1 - a^2 exactly 0. The share is asserted from the float64 restatement alone. f32: forward
    and gradients meet the f32 gate. Every mode: all gradients finite, one PPO.update logs finite scalars and clamps nothing."""
    from vision4leg_amd.torchrl.algo import PPO
    name, case = "mlp_tact", TACT_CASES["mlp_tact"]
    pf, vf = par._build(case, mode, device)
    with torch.no_grad():
        pf.base.seq_fcs[0].weight.mul_(SATURATION_FACTOR)  # (the base is shared: vf sees it too)
    obs = torch.tensor(util.make_batch(case)["obs"], dtype=torch.float32)
    opf, ovf = par._oracle_params(pf, vf, case["kind"])
    pre = obs.double() @ opf["base.seq_fcs.0.weight"].double().T + opf["base.seq_fcs.0.bias"].double()
    share = (pre.abs() > SATURATION).double().mean().item()
    assert 0.2 <= share <= 0.8, share
    for tag, net, op, A in (("pf", pf, _policy_params(opf), case["A"]), ("vf", vf, ovf, 1)):
        w = torch.tensor(np.random.RandomState(5).randn(case["B"], A), dtype=torch.float32)
        got, out = _hip_grads(net, obs, w, A, device)
        assert all(torch.isfinite(g).all() for g in got.values()) and torch.isfinite(out).all()
        if mode == "f32":
            keys = list(op)
            q = {k: v.detach().clone().requires_grad_(True) for k, v in op.items()}
            o = tact_forward(q, obs, case["S"], mode)
            ref = dict(zip(keys, par._grad((o * w).sum(), [q[k] for k in keys], mode, float(w.abs().max()))))
            assert util.rel_err(out, o.detach()) < par.TOL[mode]
            for k in keys:
                assert util.rel_err(got[k], ref[k]) < par.TOL[mode], (tag, k, util.rel_err(got[k], ref[k]))
            # exactly saturated units pass no gradient to their weight rows: a sample's row term is d * (1 - a^2) * x = 0
            dead = (pre.abs() > 12.0).all(dim=0)  # (a margin over 9.02: the engine's fp32 pre-activation may differ in the last bits)
            if dead.any():
                assert (got["base.seq_fcs.0.weight"][dead] == 0).all() and (got["base.seq_fcs.0.bias"][dead] == 0).all()

    class Coll: epoch_frames = 1
    agent = PPO(pf=pf, vf=vf, plr=1e-4, vlr=1e-4, clip_para=0.2, opt_epochs=3, tau=0.95, entropy_coeff=0.005,
                collector=Coll(), device=device, batch_size=case["B"])
    agent.trainer.sync_target()
    b = util.make_batch(case)
    info = agent.update({k: b[k] for k in ("obs", "acts", "advs", "estimate_returns", "values")})
    assert np.isfinite([info[k] for k in util.STAT_KEYS]).all(), info
    assert all(torch.isfinite(v).all() for v in pf.state_dict().values()) and all(torch.isfinite(v).all() for v in vf.state_dict().values())
    assert agent.f16_saturated == 0


def _rollout_configs():
    out = [(n, E) for n in ("mlp_tact", "mlp_tact_tanh") for E in (1, 17, 64, 65)]
    return out + [("mlp_tact_rag", E) for E in (4, 33)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,E", _rollout_configs())
def test_rollout_step(name, mode, E, device):
    """tests/test_gpu_wide_actions.py::test_rollout_step's statements and tolerances: RolloutActor.step == the separate explore
    + value calls, and the stored log pi_old is the acting policy's log-prob of the filed action. E = 1: the one env of
    ppo_state; 17: a second, partly filled row tile; 64: the one-block kernel's limit; 65: the first count past it (per-sample
    kernel in every mode); mlp_tact_rag: the general route."""
    from vision4leg_amd.torchrl.policies import RolloutActor
    case = TACT_CASES[name]
    A, T, tanh = case["A"], 2, case["kind"].endswith("_tanh")
    pf, vf = par._build(case, mode, device)
    net = pf.hip
    net.ensure_bound()
    state, image = net.alloc_rollout(T * E, device)
    acts, vals, logp = torch.zeros(T * E, A, device=device), torch.zeros(T * E, device=device), torch.zeros(T * E, device=device)
    obs = torch.tensor(util.obs_rows(np.random.RandomState(3), T * E, case), dtype=torch.float32, device=device)
    actor = RolloutActor(pf, vf, E)
    actor.attach((state, image, acts, vals, logp))
    actor.seek(0)
    tol = 1e-5 if mode == "f32" else 4e-3
    for s in range(T):
        ob = obs[s * E:(s + 1) * E]
        torch.manual_seed(100 + s)
        out = {k: v.clone() for k, v in actor.step(ob).items()}
        torch.manual_seed(100 + s)
        eps = torch.randn(E, A, device=device)
        mean, std, _ = pf(ob)
        value = vf(ob)
        dm, dv = (out["mean"] - mean).abs().max().item(), (out["value"] - value).abs().max().item()
        print("\n[%s %s E=%d] step %d: |mean - module| %.2e |value - module| %.2e" % (name, mode, E, s, dm, dv))
        assert dm <= tol * max(1.0, mean.abs().max().item()) and dv <= tol * max(1.0, value.abs().max().item()), (s, dm, dv)
        assert tuple(out["action"].shape) == (E, A) and torch.allclose(out["std"], std)
        pre = out["mean"] + out["std"] * eps
        assert torch.allclose(out["action"], torch.tanh(pre) if tanh else pre, rtol=1e-5, atol=1e-6)
        assert torch.equal(acts[s * E:(s + 1) * E], out["action"]) and torch.equal(vals[s * E:(s + 1) * E], out["value"].view(E))
        stored = logp[s * E:(s + 1) * E]
        if tanh:
            lp, _ = orc.log_prob_entropy(out["mean"].cpu(), out["std"].cpu(), out["action"].cpu(), tanh_action=True)
            assert torch.allclose(stored.cpu(), lp.reshape(-1), rtol=1e-4, atol=1e-4)
        else:
            want = torch.distributions.Normal(out["mean"], out["std"]).log_prob(out["action"]).sum(-1)
            assert torch.allclose(stored, want, rtol=1e-5, atol=1e-5)
        # and the step computed Tanh nets: the same-mode restatement on the step's rows (the forward gate's caps)
        opf, _ = par._oracle_params(pf, vf, case["kind"])
        with torch.no_grad():
            om = orc.FORWARDS[case["kind"]](_policy_params(opf), ob.cpu(), case["S"], mode)
        assert util.rel_err(out["mean"].cpu(), om) < (par.TOL["f32"] if mode == "f32" else par.REF_DIST[mode])
    assert torch.isfinite(acts).all()


@pytest.mark.parametrize("mode", MODES)
def test_same_routes_as_relu(mode, device):
    """A Tanh net of the shipped shape launches what its ReLU twin launches: the forward(train) + backward pair against the
    recorded table of pass/mlp_s93, one rollout step against mlp_s93 (mlp_tact) and mlp_tanh (mlp_tact_tanh) with and without
    the shared encoder — labels, call counts and FLOP strings, at the tables' own geometry (E = 8, N = 6)."""
    from vision4leg_amd import engine

    def pass_rows():
        case = dict(TACT_CASES["mlp_tact"], B=route.N)
        pf, _ = route._nets(case, device)
        hip = pf.hip
        assert hip.cfg.activation == 1
        obs = torch.tensor(util.make_batch(case)["obs"], dtype=torch.float32, device=device)
        st, im, n = hip.stage(obs)
        dout = torch.zeros(n, 16, dtype=torch.float32, device=device)
        dout[:, :case["A"]] = torch.randn(n, case["A"], generator=torch.Generator().manual_seed(7)).to(device)
        grads = torch.zeros(hip.total_params, dtype=torch.float32, device=device)

        def pair():
            hip.forward(st, im, n, train=True)
            hip.backward(st, im, n, dout, grads, scale=1.0)
        pair()
        return route._profiled(pair)
    rows = route._with_env(mode, {}, pass_rows)
    want = route.TABLES[route.ROUTES["pass/mlp_s93/%s/plain" % mode]]
    assert [r[:2] for r in rows] == [r[:2] for r in want]
    assert rows == want

    for name, twin in (("mlp_tact", "mlp_s93"), ("mlp_tact_tanh", "mlp_tanh")):
        for shared in (True, False):
            def step_rows():
                case = TACT_CASES[name]
                pf, vf = route._nets(case, device)
                assert pf.hip.cfg.activation == 1 and vf.hip.cfg.activation == 1
                actor = engine.HipActor(pf.hip, vf.hip, rollout_route.E, shared_encoder=shared, graph=False)
                obs = torch.tensor(np.clip(np.random.RandomState(3).randn(rollout_route.E, case["S"]), -10, 10),
                                   dtype=torch.float32, device=device)
                actor.step(obs)  # (packs the operand-type weights)
                return actor.split_supported(), rollout_route.profile_step(actor, obs)
            split, rows = route._with_env(mode, {}, step_rows)
            want_split, want_rows = rollout_route.ROUTES[rollout_route._key(twin, mode, shared, False)]
            assert split == want_split
            assert rows == want_rows, (name, shared, rows, want_rows)


def _loop_agent(case, seed, device, buffer, save_dir, E, T, B, num_epochs, **kw):
    from vision4leg_amd.torchrl.algo import PPO
    from vision4leg_amd.torchrl.collector import VecOnPolicyCollector
    from vision4leg_amd.torchrl.replay_buffers import DeviceOnPolicyReplayBuffer, OnPolicyReplayBuffer
    pf, vf = rsm._nets(case, seed, device)
    env = util.FakeVecEnv(E, case["S"], case["A"], img=0, seed=9, p_done=0.12, time_limit_key=True)
    eval_env = util.FakeVecEnv(E, case["S"], case["A"], img=0, seed=1, p_done=0.3)
    cls = DeviceOnPolicyReplayBuffer if buffer == "device" else OnPolicyReplayBuffer
    buf = cls(max_replay_buffer_size=E * T, env_nums=E, time_limit_filter=True)
    coll = VecOnPolicyCollector(vf, env=env, eval_env=eval_env, pf=pf, replay_buffer=buf, device=device, epoch_frames=E * T)
    assert coll.fast_path == (buffer == "device")
    return PPO(pf=pf, vf=vf, plr=1e-4, vlr=1e-4, clip_para=0.2, opt_epochs=2, tau=0.95, shuffle=True, entropy_coeff=0.005,
               env=None, replay_buffer=buf, collector=coll, logger=rsm._Log(), device=device, discount=0.99, num_epochs=num_epochs,
               batch_size=B, save_interval=1, eval_interval=1, save_dir=save_dir, **kw)


def test_train_loop_checkpoint_and_resume(device, tmp_path, monkeypatch):
    """tests/test_gpu_wide_actions.py::test_train_loop_buffers_and_resume's pattern on mlp_tact in f16 (E = 4, T = 16, B = 32):
    (a) three epochs with the resident buffer and with the host buffer agree to that test's tolerance; (b) the third epoch
    resumed in fresh objects from the second epoch's train state equals the uninterrupted one bit for bit; (c) the saved
    model_pf_2.pth loads into a plain torch.nn.Sequential of Linear / Tanh whose CPU forward is the engine's within the f16
    forward caps."""
    mode = "f16"
    monkeypatch.setenv("V4L_COMPUTE", mode)
    case = TACT_CASES["mlp_tact"]
    E, T, B = 4, 16, 32
    U = 2 * (E * T // B)
    runs = {}
    for buffer in ("device", "host"):
        np.random.seed(3); torch.manual_seed(3); torch.cuda.manual_seed(3)
        runs[buffer] = _loop_agent(case, case["seed"], device, buffer, str(tmp_path / buffer), E, T, B, 3,
                                   save_train_state=buffer == "device")
    a = runs["device"]
    assert a.pf.hip.cfg.activation == 1
    snap, inner = {}, a.save_checkpoint

    def save(prefix, epoch):
        inner(prefix, epoch)
        if epoch == 1:  # what a caller that restores its simulator keeps beside the file
            c = a.collector
            snap.update(env_rs=c.env.rs.get_state(), env_ob=c.env.ob.copy(), eval_rs=c.eval_env.rs.get_state(),
                        ob=np.array(c.current_ob, copy=True))
    a.save_checkpoint = save
    np.random.seed(3); torch.manual_seed(3); torch.cuda.manual_seed(3)
    a.train()
    assert a.trainer.adam_steps() == (3 * U, 3 * U) and len(a.logger.updates) == 3 * U and a.f16_saturated == 0
    h = runs["host"]
    np.random.seed(3); torch.manual_seed(3); torch.cuda.manual_seed(3)
    h.train()
    assert len(h.logger.updates) == 3 * U
    for u, (x, y) in enumerate(zip(a.logger.updates, h.logger.updates)):
        assert sorted(x) == sorted(util.STAT_KEYS) and np.isfinite(list(x.values())).all()
        for k in util.STAT_KEYS:
            assert abs(x[k] - y[k]) <= 1e-2 * max(1.0, abs(y[k])), (u, k, x[k], y[k])
    # (b) resume
    b = _loop_agent(case, case["seed"] + 100, device, "device", str(tmp_path / "resumed"), E, T, B, 3,
                    save_train_state=True, resume=(str(tmp_path / "device"), 1))
    assert b.start_epoch == 2 and b.trainer.adam_steps() == (2 * U, 2 * U) and b.total_frames == 2 * E * T
    c = b.collector
    c.env.rs.set_state(snap["env_rs"]); c.env.ob = snap["env_ob"].copy(); c.eval_env.rs.set_state(snap["eval_rs"])
    c.current_ob = snap["ob"].copy()
    b.load_checkpoint(str(tmp_path / "device"), 1, restore_collector=True)
    b.train()
    assert [e[0] for e in b.logger.epochs] == [2] and b.trainer.adam_steps() == (3 * U, 3 * U)
    assert a.logger.updates[2 * U:] == b.logger.updates
    rsm._assert_same(rsm._state(a), rsm._state(b))
    # (c) the reference's file, read by plain torch
    sd = torch.load(os.path.join(str(tmp_path / "device"), "model_pf_2.pth"), map_location="cpu", weights_only=True)
    widths = [case["S"]] + case["enc"] + case["head"]
    mods = []
    for i, o in zip(widths[:-1], widths[1:]):
        mods += [torch.nn.Linear(i, o), torch.nn.Tanh()]
    seq = torch.nn.Sequential(*mods, torch.nn.Linear(widths[-1], case["A"]))
    ne = len(case["enc"])
    plain = {}
    for k, v in sd.items():
        if k == "logstd":
            continue
        stack, idx, leaf = k.rsplit(".", 2)
        plain["%d.%s" % (int(idx) + (2 * ne if stack == "seq_append_fcs" else 0), leaf)] = v
    seq.load_state_dict(plain, strict=True)
    obs = torch.tensor(util.make_batch(case)["obs"], dtype=torch.float32)
    with torch.no_grad():
        want = seq(obs)
        restated = tact_forward({k: v for k, v in sd.items() if k != "logstd"}, obs, case["S"])
    assert util.rel_err(restated, want) < 2e-5
    mean, _, _ = a.pf(obs.to(device))
    assert torch.equal(a.pf.state_dict()["base.seq_fcs.0.weight"].cpu(), sd["base.seq_fcs.0.weight"])
    assert util.rel_err(mean.cpu(), want) < par.REF_DIST[mode]
