"""-m gpu: policies with 9 .. 16 action dimensions (tests/wide_cases.py) on the HIP engine: forward and Gaussian head, two
PPO updates, the rollout step, the update's kernel route and the training loop with checkpoint / resume.

Tolerances are the rules of tests/test_gpu_parity.py (its module docstring), none of them new: the f32 bounds; for the 16-bit
modes the forward within ENV_FACTOR x the p95 of the oracle's own nudged runs (computed from the oracle alone), the update
infos within 5e-3 of the same-mode oracle (second update, statistics that are discontinuous in the ratio: or within 5e-2 of the
fp32 reference value), the parameters within 2.2e-4 per update. The fp32 reference value is the reference's own golden for the
two fixture cases and the fp32 oracle elsewhere (tests/test_wide_actions_cpu.py pins that oracle to the reference at A = 12 to
2e-4 on both updates)."""
import os

import numpy as np
import pytest
import torch

import test_gpu_parity as par
import test_gpu_resume as rsm
import test_gpu_update_route as route
import util
from oracle import ppo_oracle as orc
from wide_cases import ALL_CASES, FIXTURE_CASES, WIDE_CASES

pytestmark = pytest.mark.gpu

MODES = par.MODES
NAMES = list(WIDE_CASES)
_FWD_ENV = {}


def _forward_envelope(name, mode, params, obs, case):
    """test_gpu_parity._bf16_envelope's forward part (same seeds, nudge sizes and percentile), without the gradients it also
    computes: p95 over the nudged runs of rel_err(mean) against the un-nudged oracle of the same mode."""
    if (name, mode) not in _FWD_ENV:
        fn = orc.FORWARDS[case["kind"]]
        with torch.no_grad():
            out0 = fn(params, obs, case["S"], mode)
            errs = []
            for scale in par.ENV_SCALES:
                for sd in range(1, par.ENV_SEEDS + 1):
                    gen = torch.Generator().manual_seed(sd)
                    q = {k: v * (1 + scale * torch.randn(v.shape, generator=gen)) for k, v in params.items()}
                    errs.append(util.rel_err(fn(q, obs, case["S"], mode), out0))
        _FWD_ENV[(name, mode)] = float(np.percentile(errs, 95))
    return _FWD_ENV[(name, mode)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_forward_and_gauss_head(name, mode, device):
    """mean / std / log-prob of given actions / entropy (policy forward, update(obs, acts): gauss_head_kernel at A up to 16)."""
    case = WIDE_CASES[name]
    A, tanh = case["A"], case["kind"].endswith("_tanh")
    pf, vf = par._build(case, mode, device)
    b = util.make_batch(case)
    obs = torch.tensor(b["obs"], dtype=torch.float32)
    acts = torch.tensor(b["acts"], dtype=torch.float32)
    mean, std, log_std = pf(obs.to(device))
    up = pf.update(obs.to(device), acts.to(device))
    opf, _ = par._oracle_params(pf, vf, case["kind"])
    pm = {k: v for k, v in opf.items() if k != "logstd"}
    with torch.no_grad():
        om = orc.FORWARDS[case["kind"]](pm, obs, case["S"], mode)
    em = util.rel_err(mean.cpu(), om)
    print("\n[%s %s] mean rel err vs %s-oracle %.2e" % (name, mode, mode, em))
    util.record("wide/forward/%s/%s/mean_vs_oracle" % (name, mode), em)
    if mode == "f32":
        assert em < par.TOL[mode]
    else:
        env = _forward_envelope(name, mode, pm, obs, case)
        util.record("wide/forward/%s/%s/mean_envelope_p95" % (name, mode), env)
        assert em <= max(par.ENV_FACTOR * env, par.ENV_FLOOR), (em, env)
    if name in FIXTURE_CASES:
        gm = util.rel_err(mean.cpu(), util.load_golden("ppo_" + name)["fwd_mean"])
        assert gm < (par.TOL["f32"] if mode == "f32" else par.REF_DIST[mode]), gm
    assert tuple(mean.shape) == tuple(std.shape) == (case["B"], A) and tuple(log_std.shape) == (A,)
    _, ostd, ols = orc.gaussian(om, opf["logstd"])
    assert torch.allclose(std.cpu(), ostd) and torch.allclose(log_std.cpu(), ols)
    # the head's own arithmetic, on the engine's mean: every one of the A terms is in the sums
    lp, ent = orc.log_prob_entropy(mean.cpu(), std.cpu(), acts, tanh_action=tanh)
    assert torch.allclose(up["log_prob"].cpu(), lp, rtol=1e-5, atol=1e-5) and torch.allclose(up["ent"].cpu(), ent, atol=1e-6)
    assert tuple(up["log_prob"].shape) == (case["B"], 1)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(ALL_CASES))
def test_two_updates(name, mode, device):
    """tests/test_gpu_parity.py::test_ppo_update on the wide cases: 18 infos and every parameter of pf and vf after each of two
    PPO.update calls. The fp32 parameter bound leans on the oracle's own fp32 error being far below it on these seeded
    inputs: tests/wide_cases.py ("Seeds"), asserted from the oracle alone in tests/test_wide_actions_cpu.py."""
    from vision4leg_amd.torchrl.algo import PPO
    case = ALL_CASES[name]
    n_updates = case.get("updates", 2)  # (loco_a12_b512: the n >= 512 loss launch, one update — tests/wide_cases.py)
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
    if gold is None and mode != "f32" and n_updates > 1:  # the fp32 value of the either-or rule where the reference itself was not run
        rpf, rvf = par._oracle_params(pf, vf, case["kind"])
        ref32 = orc.PPOOracle(case["kind"], rpf, rvf, {k: v.clone() for k, v in rpf.items()}, case["S"], "f32")
        ref32.sync_target()
    agent.trainer.sync_target()
    t = lambda a: torch.tensor(a, dtype=torch.float32)
    for u in range(n_updates):
        b = util.make_batch(case, update=u)
        before = {k: v.detach().cpu().clone() for k, v in pf.state_dict().items()}
        args = (t(b["obs"]), t(b["acts"]), t(b["advs"]), t(b["estimate_returns"]), t(b["values"]), 1e-4, 1e-4)
        info = agent.update({k: b[k] for k in ("obs", "acts", "advs", "estimate_returns", "values")})
        oinfo = oracle.update(*args)
        ginfo = dict(zip(util.STAT_KEYS, gold["u%d/info" % u])) if gold is not None else ref32.update(*args) if ref32 else None
        print("\n[%s %s] update %d info (hip / oracle):" % (name, mode, u))
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
        util.record("wide/ppo_update/%s/%s/u%d/worst_abs_param_vs_oracle" % (name, mode, u), worst)
        util.record("wide/ppo_update/%s/%s/u%d/max_info_rel_vs_oracle" % (name, mode, u),
                    max(abs(info[k] - oinfo[k]) / max(1.0, abs(oinfo[k])) for k in util.STAT_KEYS))
        assert tot / cnt <= (1e-7 if mode == "f32" else 2e-5 * (u + 1))
        assert max((pf.state_dict()[k].cpu() - before[k]).abs().max().item() for k in before) > 5e-5  # the optimiser stepped
        assert (pf.state_dict()["logstd"].cpu() - before["logstd"]).abs().min().item() > 0  # ... in every one of the A log sigmas
    assert agent.f16_saturated == 0


@pytest.mark.parametrize("E", [4, 33])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_rollout_step(name, mode, E, device):
    """RolloutActor.step == the separate explore + value calls (tests/test_gpu_parity.py::_actor_vs_separate, its tolerances),
    and the stored log pi_old is the acting policy's log-prob of the filed action (test_stored_logp_equals_target_forward's
    statement (a); its statement (b) is test_stored_logp_equals_target_forward_wide below). E = 33: a second, partly filled
    16-row tile."""
    from vision4leg_amd.torchrl.policies import RolloutActor
    case = WIDE_CASES[name]
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
        assert dm <= tol * max(1.0, mean.abs().max().item()) and dv <= tol * max(1.0, value.abs().max().item()), (s, dm, dv)
        assert tuple(out["action"].shape) == (E, A) and torch.allclose(out["std"], std)
        pre = out["mean"] + out["std"] * eps
        assert torch.allclose(out["action"], torch.tanh(pre) if tanh else pre, rtol=1e-5, atol=1e-6)
        assert torch.equal(acts[s * E:(s + 1) * E], out["action"]) and torch.equal(vals[s * E:(s + 1) * E], out["value"].view(E))
        stored = logp[s * E:(s + 1) * E]
        if tanh:  # tests/test_gpu_parity.py::test_tanh_policy_head's statement and tolerance (log-prob through atanh of the STORED action)
            lp, _ = orc.log_prob_entropy(out["mean"].cpu(), out["std"].cpu(), out["action"].cpu(), tanh_action=True)
            assert torch.allclose(stored.cpu(), lp.reshape(-1), rtol=1e-4, atol=1e-4)
        else:  # test_stored_logp_equals_target_forward's statement (a) and tolerance
            want = torch.distributions.Normal(out["mean"], out["std"]).log_prob(out["action"]).sum(-1)
            assert torch.allclose(stored, want, rtol=1e-5, atol=1e-5)
    assert torch.isfinite(acts).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_stored_logp_equals_target_forward_wide(name, mode, device):
    """tests/test_gpu_parity.py::test_stored_logp_equals_target_forward's statement (b), its shapes and its tolerances, on the
    wide cases: minibatch updates fed with the log pi_old the rollout step stored and with the frozen target policy's forward
    (what the reference's update(obs, acts) evaluates, ppo.py:55-57) give the same infos and parameters."""
    from vision4leg_amd.engine import HipTrainer
    from vision4leg_amd.torchrl.algo import PPO
    from vision4leg_amd.torchrl.policies import RolloutActor
    case = dict(WIDE_CASES[name], B=32)
    T, E, B = 8, 8, 32
    rs = np.random.RandomState(11)
    obs = torch.tensor(util.obs_rows(rs, T * E, case), dtype=torch.float32, device=device)
    advs, rets = rs.randn(T * E), rs.randn(T * E)
    rows = np.stack([rs.permutation(T * E)[:B] for _ in range(4)]).astype(np.int32)
    t32 = lambda a: torch.tensor(a, dtype=torch.float32, device=device)
    results = []
    for stored in (True, False):
        pf, vf = par._build(case, mode, device)

        class Coll: epoch_frames = T * E
        agent = PPO(pf=pf, vf=vf, plr=1e-4, vlr=1e-4, clip_para=0.2, opt_epochs=3, tau=0.95, entropy_coeff=0.005,
                    collector=Coll(), device=device, batch_size=B)
        agent.use_graph = False
        net = pf.hip
        net.ensure_bound()
        state, image = net.alloc_rollout(T * E, device)
        acts, vals, logp = torch.zeros(T * E, case["A"], device=device), torch.zeros(T * E, device=device), \
            torch.zeros(T * E, device=device)
        actor = RolloutActor(pf, vf, E)
        actor.attach((state, image, acts, vals, logp))
        actor.seek(0)
        for t in range(T):
            torch.manual_seed(500 + t)
            actor.step(obs[t * E:(t + 1) * E])
        ro = HipTrainer.rollout(state, image, acts, t32(advs), t32(rets), vals, logp if stored else None)
        stats = torch.zeros(len(rows), 24, device=device)
        agent.trainer.sync_target()
        agent.run_updates(ro, torch.tensor(rows, device=device), stats)
        torch.cuda.synchronize()
        results.append(({k: v.detach().cpu().clone() for k, v in pf.state_dict().items()}, stats.cpu().numpy()))
    (ps, ss), (pt, st) = results
    err = np.abs(ss[:, :18] - st[:, :18]) / np.maximum(1.0, np.abs(st[:, :18]))
    print("\n[wide stored logp %s %s] infos: first update %.2e, all updates %.2e" % (name, mode, err[0].max(), err.max()))
    util.record("wide/stored_logp/%s/%s/infos_first_update" % (name, mode), err[0].max())
    util.record("wide/stored_logp/%s/%s/infos_all_updates" % (name, mode), err.max())
    assert np.isfinite(ss[:, :18]).all() and np.isfinite(st[:, :18]).all()
    assert err[0].max() <= (2e-5 if mode == "f32" else 2e-3), err[0]
    assert err.max() <= (2e-4 if mode == "f32" else 2e-2), err.max(axis=1)
    drift = sum((ps[k] - pt[k]).abs().sum().item() for k in ps) / sum(v.numel() for v in ps.values())
    assert drift <= (1e-6 if mode == "f32" else 5e-5), drift


def _stored_update_labels(case, mode, device):
    """Kernel labels of one minibatch update with log pi_old stored at action time (the resident-buffer epoch's update)."""
    from vision4leg_amd.engine import HipTrainer
    from vision4leg_amd.torchrl.algo import PPO

    def run():
        pf, vf = par._build(case, mode, device)
        n = case["B"]
        assert os.environ["V4L_COMPUTE"] == mode

        class Coll: epoch_frames = n
        agent = PPO(pf=pf, vf=vf, plr=1e-4, vlr=1e-4, clip_para=0.2, opt_epochs=3, tau=0.95, entropy_coeff=0.005,
                    collector=Coll(), device=device, batch_size=n)
        agent.use_graph = False
        net = pf.hip
        net.ensure_bound()
        state, image = net.alloc_rollout(n, device)
        b = util.make_batch(case)
        net.ingest(torch.tensor(b["obs"], dtype=torch.float32, device=device), state, image)
        t32 = lambda a: torch.tensor(np.asarray(a).reshape(-1), dtype=torch.float32, device=device)
        acts = torch.tensor(b["acts"], dtype=torch.float32, device=device)
        ro = HipTrainer.rollout(state, image, acts, t32(b["advs"]), t32(b["estimate_returns"]), t32(b["values"]),
                                torch.full((n,), -float(case["A"]), device=device))
        rows = torch.arange(n, dtype=torch.int32, device=device).view(1, n)
        agent.trainer.sync_target()
        agent.run_updates(ro, rows, torch.zeros(1, 24, device=device))
        return route._profiled(lambda: agent.run_updates(ro, rows, torch.zeros(1, 24, device=device)))
    return [r[0] for r in route._with_env(mode, {}, run)]


def test_update_route_at_a12(device):
    """LocoTransformer, A = 12: the layers stay on the wave-per-sample kernels (WPS_PLAIN); the policy's pass is forward + loss
    launch + backward (the route TanhNormal policies take), the critic keeps the fused forward-loss-backward launch. A = 6:
    both nets on the fused launch, as before."""
    wide = _stored_update_labels(dict(WIDE_CASES["loco_a12"], B=6), "f16", device)
    narrow = _stored_update_labels(dict(util.CASES["loco_s84"], B=6), "f16", device)
    fb = lambda tag: tag + ".bwd|layer|wps_layer_fb_stack"
    assert fb("vf") in wide and fb("pf") not in wide
    for label in ("pf.fwd|layer|wps_layer_stack_head", "|loss|actor_loss", "pf.bwd|layer|wps_layer_bwd_stack"):
        assert label in wide, (label, wide)
    assert fb("vf") in narrow and fb("pf") in narrow
    assert not any(l.startswith("pf.fwd|layer") or l == "|loss|actor_loss" for l in narrow), narrow
    # one whole PPO.update (target forward instead of stored log-probs) takes the launch sequence recorded for A = 6
    # (tests/test_gpu_update_route.py; FLOP counts differ with the width of the last head layer)
    def one_update():
        from vision4leg_amd.torchrl.algo import PPO
        case = dict(WIDE_CASES["loco_a12"], B=route.N)
        pf, vf = route._nets(case, device)

        class Coll: epoch_frames = 1
        agent = PPO(pf=pf, vf=vf, plr=1e-4, vlr=1e-4, clip_para=0.2, opt_epochs=3, tau=0.95, entropy_coeff=0.005,
                    collector=Coll(), device=device, batch_size=route.N)
        agent.trainer.sync_target()
        agent.update(util.make_batch(case, update=0))
        return route._profiled(lambda: agent.update(util.make_batch(case, update=1)))
    rows = route._with_env("f16", {}, one_update)
    want = route.TABLES[route.ROUTES["update/loco_s84/f16/plain"]]
    assert [r[:2] for r in rows] == [r[:2] for r in want]


def _loop_agent(case, seed, device, buffer, save_dir, E, T, B, num_epochs, **kw):
    from vision4leg_amd.torchrl.algo import PPO
    from vision4leg_amd.torchrl.collector import VecOnPolicyCollector
    from vision4leg_amd.torchrl.replay_buffers import DeviceOnPolicyReplayBuffer, OnPolicyReplayBuffer
    pf, vf = rsm._nets(case, seed, device)
    env = util.FakeVecEnv(E, case["S"], case["A"], seed=9, p_done=0.12, time_limit_key=True)
    eval_env = util.FakeVecEnv(E, case["S"], case["A"], seed=1, p_done=0.3)
    cls = DeviceOnPolicyReplayBuffer if buffer == "device" else OnPolicyReplayBuffer
    buf = cls(max_replay_buffer_size=E * T, env_nums=E, time_limit_filter=True)
    coll = VecOnPolicyCollector(vf, env=env, eval_env=eval_env, pf=pf, replay_buffer=buf, device=device, epoch_frames=E * T)
    assert coll.fast_path == (buffer == "device")
    return PPO(pf=pf, vf=vf, plr=1e-4, vlr=1e-4, clip_para=0.2, opt_epochs=2, tau=0.95, shuffle=True, entropy_coeff=0.005,
               env=None, replay_buffer=buf, collector=coll, logger=rsm._Log(), device=device, discount=0.99, num_epochs=num_epochs,
               batch_size=B, save_interval=1, eval_interval=1, save_dir=save_dir, **kw)


@pytest.mark.parametrize("mode", MODES)
def test_train_loop_buffers_and_resume(mode, device, tmp_path, monkeypatch):
    """PPO.train() over tests/util.FakeVecEnv(E=4, S=84, A=12), T = 16, B = 32. (a) Three epochs with the resident buffer (fused
    rollout step, row-index minibatches, stored log pi_old) and with the host buffer (the reference's protocol): the update
    infos agree to test_epoch_device_buffer_equals_host_buffer's tolerance. (b) A third epoch: uninterrupted, and in fresh
    objects resumed from the second epoch's train state with the simulator put back where it was (the file does not hold it)
    — parameters, Adam moments, step counts and the epoch's infos are equal bit for bit.
    (Two epochs plus one extra: all runs are built with num_epochs = 3, because the learning-rate schedule is a function of it,
    so the uninterrupted twin of the resumed epoch is simply the third epoch of the first run.)"""
    monkeypatch.setenv("V4L_COMPUTE", mode)
    case = WIDE_CASES["loco_a12"]
    E, T, B = 4, 16, 32
    U = 2 * (E * T // B)
    runs = {}
    for buffer in ("device", "host"):
        np.random.seed(3); torch.manual_seed(3); torch.cuda.manual_seed(3)
        runs[buffer] = _loop_agent(case, case["seed"], device, buffer, str(tmp_path / buffer), E, T, B, 3,
                                   save_train_state=buffer == "device")
    a = runs["device"]
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
    h = runs["host"]  # (three epochs as well: the learning-rate schedule is a function of num_epochs)
    np.random.seed(3); torch.manual_seed(3); torch.cuda.manual_seed(3)
    h.train()
    tol = 2e-4 if mode == "f32" else 1e-2
    assert len(h.logger.updates) == 3 * U
    worst = 0.0
    for u, (x, y) in enumerate(zip(a.logger.updates, h.logger.updates)):
        assert sorted(x) == sorted(util.STAT_KEYS) and np.isfinite(list(x.values())).all()
        for k in util.STAT_KEYS:
            worst = max(worst, abs(x[k] - y[k]) / max(1.0, abs(y[k])))
    print("\n[wide train loop %s] resident vs host buffer: worst info deviation %.2e (bound %.0e)" % (mode, worst, tol))
    util.record("wide/train_loop/%s/worst_info_resident_vs_host" % mode, worst)
    for u, (x, y) in enumerate(zip(a.logger.updates, h.logger.updates)):
        for k in util.STAT_KEYS:
            assert abs(x[k] - y[k]) <= tol * max(1.0, abs(y[k])), (u, k, x[k], y[k])
    # (b) resume
    b = _loop_agent(case, case["seed"] + 100, device, "device", str(tmp_path / "resumed"), E, T, B, 3,
                    save_train_state=True, resume=(str(tmp_path / "device"), 1))
    assert b.start_epoch == 2 and b.trainer.adam_steps() == (2 * U, 2 * U) and b.total_frames == 2 * E * T
    c = b.collector
    c.env.rs.set_state(snap["env_rs"]); c.env.ob = snap["env_ob"].copy(); c.eval_env.rs.set_state(snap["eval_rs"])
    c.current_ob = snap["ob"].copy()
    b.load_checkpoint(str(tmp_path / "device"), 1, restore_collector=True)  # (the generator states again: building b drew none, but cheap)
    b.train()
    assert [e[0] for e in b.logger.epochs] == [2] and b.trainer.adam_steps() == (3 * U, 3 * U)
    assert a.logger.updates[2 * U:] == b.logger.updates
    rsm._assert_same(rsm._state(a), rsm._state(b))
