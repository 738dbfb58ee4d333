"""-m gpu: REINFORCE (algo.Reinforce, the reference's torchrl/algo/on_policy/reinforce.py) on the HIP engine: one loss
evaluation's gradients and statistics, two updates of every case of tests/reinforce_cases.py against the same-mode restatement,
the reference's own fixtures, the zero critic, graph replays against eager launches, the resident epoch, and PPO / V-MPO / A2C
next to a Reinforce trainer.

The reference arithmetic is reinforce_cases.ReinforceOracle (pinned to the unmodified reference by
tests/golden/make_golden_reinforce.py and tests/test_reinforce_cpu.py). The bounds of test_two_updates are
tests/test_gpu_a2c.py::test_two_updates' (infos 5e-4 / 5e-3 relative to max(1, |x|), every parameter element 2e-5 / 2.2e-4 (u + 1),
the mean 1e-7 / 2e-5 (u + 1); the either-or rule of the 16-bit modes from the second update on, for Training/policy_loss only):
sized as multiples of lr = 1e-4, and an Adam step is bounded by lr whatever eps is. One loss evaluation is held to
tests/test_gpu_parity.py's TOL / REF_DIST against the float64 loss stage."""
import hashlib
import os

import numpy as np
import pytest
import torch

import test_gpu_parity as par
import test_gpu_vmpo as tv
import test_gpu_a2c as ta
import util
import a2c_cases as ac
import reinforce_cases as rc
from reinforce_cases import REINFORCE_CASES, FIXTURE_CASES, INFO_KEYS, LR, updates_of

pytestmark = pytest.mark.gpu

MODES = par.MODES
NAMES = list(REINFORCE_CASES)
EITHER_OR = ("Training/policy_loss",)


class _Coll:
    epoch_frames = 1


def _policy(case, mode, dev):
    os.environ["V4L_COMPUTE"] = mode
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    return rc.seeded_policy(networks, policies, case).to(dev)


def _agent(case, mode, device, **kw):
    from vision4leg_amd.torchrl.algo import Reinforce
    pf = _policy(case, mode, device)
    args = dict(plr=LR, tau=0.95, shuffle=True, entropy_coeff=rc.ENTROPY_COEFF, env=None, replay_buffer=None,
                collector=_Coll(), logger=None, device=device, discount=0.99, num_epochs=1500, batch_size=case["B"], save_dir=None)
    args.update(kw)
    return Reinforce(pf=pf, **args), pf


def _own(vf, pf):
    shared = {id(p) for p in pf.parameters()}
    return {k: p for k, p in vf.named_parameters() if id(p) not in shared}


def test_surface(device):
    """The reference's attribute surface (reinforce.py:19-32,78-82, on_rl_algo.py:18-21,43-48): a policy optimiser with torch's
    default eps and nothing of a critic's or PPO's."""
    import vision4leg_amd.torchrl.networks as networks
    case = REINFORCE_CASES["rf_mlp_odd"]
    agent, pf = _agent(case, "f32", device, gae=True)
    assert agent.sample_key == ["obs", "acts", "advs", "estimate_returns"]
    assert agent.networks == [pf, agent.vf] and agent.snapshot_networks == [("pf", pf)]
    assert networks.is_zero_critic(agent.vf, pf)
    for gone in ("target_pf", "vf_optimizer", "vlr", "clip_para", "opt_epochs", "clipped_value_loss"):
        assert not hasattr(agent, gone), gone
    assert agent.trainer.hp.max_grad_norm == 0.5 and agent.pf_optimizer.param_groups[0]["eps"] == 1e-8
    assert abs(agent.trainer.hp.eps - 1e-8) <= 1e-15
    assert agent.plr == LR and agent.gae is False and agent.tau == 0.95 and agent.optimizer_class is torch.optim.Adam


# ------------------------------------------------------------------------------------------ one loss evaluation
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["rf_mlp_odd", "rf_mlp_tanh", "rf_mlp_odd@513"])
def test_loss_rows(name, mode, device):
    """reinforce_loss_kernel through the trainer's eager entry, nothing stepped: d(policy_loss)/d(mean) rows, d/d(logstd) and the
    10 statistics against the float64 loss stage (reinforce_cases.loss_stage64) on the head rows the forward left in the
    workspace. The policy gets distinct log sigmas (one beyond the clamp for the Normal policy: its gradient is gated to 0) and
    means O(1) first; the head rows are also held to the restatement's forward (par.TOL / par.REF_DIST), so the stage is fed what
    the reference's would be. Gradients: par.TOL["f32"] in f32, par.REF_DIST in the 16-bit modes. Statistics: test_two_updates'
    info bounds.
    "@513" (util.loss_rows_case): the capacity-16 kernel in its 1024-thread block; in f32 with a log sigma below LOG_SIG_MIN
    too (util.loss_rows_both_ends): both ends of the gate exactly 0, and the columns beside that one held to the bound on their
    own (its rows are 1 / sigma^2 = 2.2e4 times theirs and would carry the norm alone)."""
    from vision4leg_amd import _lib
    from vision4leg_amd.engine import HipTrainer
    case = util.loss_rows_case(REINFORCE_CASES, name)
    A, n = case["A"], case["B"]
    tanh = case["kind"].endswith("_tanh")
    agent, pf = _agent(case, mode, device)
    tr = agent.trainer
    both_ends = util.loss_rows_both_ends(name, mode, tanh)
    util.spread_policy_head(pf, util.loss_rows_logstd(A, tanh, both_ends))  # (the last one beyond LOG_SIG_MAX: sigma = e^2, no gradient)
    oracle = rc.oracle_of(pf.state_dict(), case, "f32")
    want_rows = oracle.fwd({k: v for k, v in oracle.pf.items() if k != "logstd"}, rc.batch_tensors(case, 0)[0], case["S"], "f32")
    b = rc.host_batch(case, 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
    lib = _lib.lib()
    with torch.cuda.device(device):
        hip = pf.hip
        hip.ensure_bound()
        st, im = hip.alloc_rollout(n, device)
        hip.ingest(up(b["obs"]), st, im)
        ro = HipTrainer.rollout(st, im, up(b["acts"]).reshape(n, -1), up(b["advs"]).reshape(n), up(b["estimate_returns"]).reshape(n))
        stats = torch.zeros(1, _lib.V4L_STATS, dtype=torch.float32, device=device)
        rstats = torch.zeros(1, _lib.V4L_REINFORCE_STATS, dtype=torch.float32, device=device)
        before = {k: v.detach().clone() for k, v in pf.state_dict().items()}
        tr._pre(n)
        tr.begin(None, stats, LR, LR)
        tr.reinforce_actor_grads(ro, n, rstats)
        torch.cuda.synchronize()
        off = lib.v4l_net_ws_offset(hip.h, n, b"dout")
        rows = tr.ws[off:off + n * 16].view(n, 16).cpu() / lib.v4l_net_grad_scale(hip.h, n)
        off = lib.v4l_net_ws_offset(hip.h, n, b"out")
        head = tr.ws[off:off + n * 16].view(n, 16).cpu().numpy()
        got_ls = hip.grad_view(tr.g_pf, "logstd").cpu().reshape(-1)
        rec = rstats[0].cpu().numpy()
        ppo_rec = tr.stats_cur().cpu().numpy()
    for k, v in pf.state_dict().items():
        assert torch.equal(v, before[k]), k  # nothing stepped
    assert (rows[:, A:] == 0).all()
    tol = par.TOL["f32"] if mode == "f32" else par.REF_DIST[mode]
    assert util.rel_err(head[:, :A], want_rows.detach().numpy()) < tol
    dout, dls, oinfo = rc.loss_stage64(head, pf.state_dict()["logstd"].cpu().numpy().reshape(-1), b["acts"].astype(np.float32),
                                       b["advs"].astype(np.float32).reshape(-1), A, rc.ENTROPY_COEFF, tanh)
    e_rows, e_ls = util.rel_err(rows[:, :A], dout), util.rel_err(got_ls, dls)
    print("\n[%s %s] rel err d(mean) rows %.2e, d(logstd) %.2e" % (name, mode, e_rows, e_ls))
    util.record("reinforce/loss/%s/%s/dmean_rel" % (name, mode), e_rows)
    util.record("reinforce/loss/%s/%s/dlogstd_rel" % (name, mode), e_ls)
    assert e_rows < tol and e_ls < tol, (e_rows, e_ls)
    if not tanh:
        assert got_ls[-1].item() == 0.0 and dls[-1].item() == 0.0
    if both_ends:
        assert got_ls[0].item() == 0.0 and dls[0].item() == 0.0
        assert util.rel_err(rows[:, 1:A], dout[:, 1:]) < tol
    assert len(rec) == 12 and (rec[len(INFO_KEYS):] == 0).all()
    for j, k in enumerate(INFO_KEYS):
        print("   %-22s % .6f % .6f" % (k, rec[j], oinfo[k]))
    for j, k in enumerate(INFO_KEYS):
        assert abs(rec[j] - oinfo[k]) <= (5e-4 if mode == "f32" else 5e-3) * max(1.0, abs(oinfo[k])), (k, rec[j], oinfo[k])
    # the PPO record's slots the REINFORCE launches have a value for; log_std/* and ratio/* stay at the cleared 0
    S = _lib.STAT_KEYS.index
    for k in ("Training/policy_loss", "logprob/mean", "logprob/std", "logprob/max", "logprob/min", "advs/mean", "advs/max", "advs/min"):
        assert ppo_rec[S(k)] == rec[INFO_KEYS.index(k)], k
    # (the PPO record keeps torch's std of the advantages, the REINFORCE record numpy's, as the reference logs it)
    assert abs(ppo_rec[S("advs/std")] * np.sqrt((n - 1) / n) - rec[1]) <= 1e-6 * rec[1]
    for k in ("Training/vf_loss", "grad_norm/vf", "log_std/mean", "log_std/std", "log_std/max", "log_std/min", "ratio/max", "ratio/min"):
        assert ppo_rec[S(k)] == 0.0, k
    assert ppo_rec[_lib.ST_F16_SAT] == 0.0


# ------------------------------------------------------------------------------------------ updates
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_two_updates(name, mode, device):
    """10 infos and every parameter of pf after each Reinforce.update call against the same-mode restatement; the policy's Adam
    step count advances by one per update and the critic's stays 0; nothing saturates in f16."""
    case = REINFORCE_CASES[name]
    agent, pf = _agent(case, mode, device)
    oracle = rc.oracle_of(pf.state_dict(), case, mode)
    ref32 = rc.oracle_of(pf.state_dict(), case, "f32") if mode != "f32" else None
    for u in range(updates_of(case)):
        before = {k: v.detach().cpu().clone() for k, v in pf.state_dict().items()}
        info = agent.update(rc.host_batch(case, u))
        args = rc.batch_tensors(case, u) + (LR,)
        oinfo = oracle.update(*args)
        ginfo = ref32.update(*args) if ref32 is not None else None
        assert list(info) == INFO_KEYS
        print("\n[%s %s] update %d info (hip / restatement%s):" % (name, mode, u, "" if ginfo is None else " / f32 restatement"))
        for k in INFO_KEYS:
            print("   %-22s % .6f % .6f%s" % (k, info[k], oinfo[k], "" if ginfo is None else " % .6f" % ginfo[k]))
        for k in INFO_KEYS:
            tol = (5e-4 if mode == "f32" else 5e-3) * max(1.0, abs(oinfo[k]))
            strict_ok = abs(info[k] - oinfo[k]) <= tol
            if mode != "f32" and u >= 1 and k in EITHER_OR:
                assert strict_ok or abs(info[k] - ginfo[k]) <= 5e-2 * max(1.0, abs(ginfo[k])), (u, k, info[k], oinfo[k], ginfo[k])
                continue
            assert strict_ok, (u, k, info[k], oinfo[k], None if ginfo is None else ginfo[k])
        elem = 2e-5 if mode == "f32" else 2.2e-4 * (u + 1)
        worst, tot, cnt = 0.0, 0.0, 0
        for k, v in pf.state_dict().items():
            dd = (v.detach().cpu() - oracle.pf[k]).abs()
            worst = max(worst, dd.max().item())
            tot += dd.sum().item(); cnt += dd.numel()
        util.record("reinforce/update/%s/%s/u%d/worst_abs_param_vs_oracle" % (name, mode, u), worst)
        util.record("reinforce/update/%s/%s/u%d/mean_abs_param_vs_oracle" % (name, mode, u), tot / cnt)
        util.record("reinforce/update/%s/%s/u%d/max_info_rel_vs_oracle" % (name, mode, u),
                    max(abs(info[k] - oinfo[k]) / max(1.0, abs(oinfo[k])) for k in INFO_KEYS))
        print("   worst |param - restatement| %.3e (bound %.1e), mean %.3e" % (worst, elem, tot / cnt))
        if ref32 is not None:
            far = max((v.detach().cpu() - ref32.pf[k]).abs().max().item() for k, v in pf.state_dict().items())
            print("   worst |param - f32 restatement| %.3e" % far)
        assert worst <= elem, (u, worst)
        assert tot / cnt <= (1e-7 if mode == "f32" else 2e-5 * (u + 1)), (u, tot / cnt)
        assert max((pf.state_dict()[k].cpu() - before[k]).abs().max().item() for k in before) > 5e-5  # the optimiser stepped
        assert (pf.state_dict()["logstd"].cpu() - before["logstd"]).abs().min().item() > 0
        assert agent.trainer.adam_steps() == (u + 1, 0) and agent.training_update_num == u + 1
    assert agent.f16_saturated == 0


@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_against_reference_fixture(name, device):
    """f32 mode against what the unmodified reference logged and stepped to (tests/golden/<name>.npz)."""
    case = REINFORCE_CASES[name]
    gold = util.load_golden(name)
    agent, pf = _agent(case, "f32", device)
    for u in range(2):
        info = agent.update(rc.host_batch(case, u))
        for k, want in zip(INFO_KEYS, gold["u%d/info" % u]):
            assert abs(info[k] - want) <= 5e-4 * max(1.0, abs(want)), (u, k, info[k], want)
        seen = 0
        for k, v in pf.state_dict().items():
            key = "u%d/pf/%s" % (u, k)
            if key in gold.files:
                seen += 1
                assert np.abs(v.detach().cpu().numpy() - gold[key]).max() <= 2e-5, (u, k)
        assert seen >= 4


# ------------------------------------------------------------------------------------------ the zero critic
@pytest.mark.parametrize("name", ["rf_mlp", "rf_loco"])
def test_zero_critic_is_inert(name, device):
    """f16: vf(obs) is exactly 0.0; two updates leave every parameter of the critic's own and the trainer's critic-side Adam
    moments bit-identical; the trunk parameters are pf's own tensors, moved by the policy step."""
    case = REINFORCE_CASES[name]
    agent, pf = _agent(case, "f16", device)
    vf, tr = agent.vf, agent.trainer
    obs = torch.from_numpy(np.ascontiguousarray(util.make_batch(case, update=5, B=64)["obs"], dtype=np.float32)).to(device)
    with torch.cuda.device(device):
        vals = vf(obs)
        torch.cuda.synchronize()
    assert tuple(vals.shape) == (64, 1) and (vals == 0).all()
    own = _own(vf, pf)
    assert own and len(own) < len(list(vf.parameters()))
    before = {k: p.detach().clone() for k, p in own.items()}
    trunk_before = {k: p.detach().clone() for k, p in vf.named_parameters() if k not in own}
    tr._pre(case["B"])
    m0, v0 = tr.m_vf.clone(), tr.v_vf.clone()
    for u in range(2):
        agent.update(rc.host_batch(case, u))
    torch.cuda.synchronize()
    for k, p in own.items():
        assert torch.equal(p.detach(), before[k]), k
    assert torch.equal(tr.m_vf, m0) and torch.equal(tr.v_vf, v0) and not tr.m_vf.any() and not tr.v_vf.any()
    pf_params = {id(p): k for k, p in pf.named_parameters()}
    moved = 0
    for k, p in vf.named_parameters():
        if k not in own:
            assert id(p) in pf_params, k
            moved += int(not torch.equal(p.detach(), trunk_before[k]))
    assert moved > 0
    assert tr.adam_steps() == (2, 0)
    with torch.cuda.device(device):
        assert (vf(obs) == 0).all()


# ------------------------------------------------------------------------------------------ graphs
def _digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def _run_three(case, device, U=3, runs=2):
    """`runs` runs of U updates on the rows of U seeded minibatches, through the shell's _run on a device rollout -> (per run:
    records; parameters, moments), graph counts after each run."""
    from vision4leg_amd.engine import HipTrainer
    agent, pf = _agent(case, "f16", device)
    n = case["B"]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
    bs = [rc.host_batch(case, u) for u in range(U)]
    out, counts = [], []
    with torch.cuda.device(device):
        hip = pf.hip
        hip.ensure_bound()
        st, im = hip.alloc_rollout(U * n, device)
        hip.ingest(up(np.concatenate([b["obs"] for b in bs])), st, im)
        cat = lambda k: up(np.concatenate([b[k] for b in bs]))
        arrays = (cat("acts").reshape(U * n, -1), cat("advs").reshape(-1), cat("estimate_returns").reshape(-1))
        ro = HipTrainer.rollout(st, im, *arrays)
        rowidx = torch.arange(U * n, dtype=torch.int32, device=device).view(U, n).flip(0).contiguous()
        for _ in range(runs):
            infos = agent._run(ro, rowidx, n, U, lambda u: "update %d" % u)
            torch.cuda.synchronize()
            counts.append(agent.trainer.reinforce_graph_counts())
            tr = agent.trainer
            out.append((infos, _digest([v for v in pf.state_dict().values()] + [tr.m_pf, tr.v_pf, tr.m_vf, tr.v_vf])))
    assert agent.trainer.adam_steps() == (U * runs, 0)
    return out, counts


@pytest.mark.parametrize("name", ["rf_mlp", "rf_loco"])
def test_run_equals_eager(name, device, monkeypatch):
    """U = 3 updates twice: the first run of a configuration goes update by update (one eager, the single-update graph, two
    replays), the second is one capture and one replay of the whole run. One replay per update (V4L_EPOCH_GRAPH=0) and eager
    launches (V4L_GRAPH=0) give bit-identical parameters, moments and records."""
    case = REINFORCE_CASES[name]
    monkeypatch.delenv("V4L_GRAPH", raising=False)
    monkeypatch.delenv("V4L_EPOCH_GRAPH", raising=False)
    run, counts = _run_three(case, device)
    print("\n(captures, replays) after each run: %s" % counts)
    assert counts == [(1, 2), (2, 3)]
    assert np.isfinite([v for i in run[1][0] for v in i.values()]).all()
    monkeypatch.setenv("V4L_EPOCH_GRAPH", "0")
    per_update, counts_u = _run_three(case, device)
    assert counts_u == [(1, 2), (1, 5)]
    monkeypatch.delenv("V4L_EPOCH_GRAPH")
    monkeypatch.setenv("V4L_GRAPH", "0")
    eager, counts_e = _run_three(case, device)
    assert counts_e == [(0, 0), (0, 0)]
    for other in (per_update, eager):
        for r in range(2):
            assert run[r][0] == other[r][0], r
            assert run[r][1] == other[r][1], r


# ------------------------------------------------------------------------------------------ resident epoch
def _discount_reward64(rewards, terminals, time_limits, gamma):
    """The reference's discount_reward loop (replay_buffers/on_policy.py:47-71) with time_limit_filter, values = last_value = 0."""
    T = len(rewards)
    R = np.zeros_like(rewards[0])
    out = [None] * T
    for t in reversed(range(T)):
        tl = np.asarray(time_limits[t], dtype=np.float64)
        R = (rewards[t] + (1 - terminals[t]) * gamma * R * (1 - tl)) + tl * 0.0
        out[t] = R
    return np.array(out)


def test_resident_epoch(device, monkeypatch):
    """E = 4, T = 8, B = 16: a VecOnPolicyCollector given networks.ZeroNet(), a DeviceOnPolicyReplayBuffer, one train_one_epoch +
    update_per_epoch. The filed values are exact zeros, advs == estimate_returns == the reference's discounted rewards, U = 2
    updates are logged with the 10 keys, and the same epoch fed through a host OnPolicyReplayBuffer gives the same parameters bit
    for bit."""
    from vision4leg_amd import recipes
    import vision4leg_amd.torchrl.networks as networks
    from vision4leg_amd.torchrl.algo import Reinforce
    from vision4leg_amd.torchrl.collector import VecOnPolicyCollector
    from vision4leg_amd.torchrl.replay_buffers import DeviceOnPolicyReplayBuffer, OnPolicyReplayBuffer
    monkeypatch.delenv("V4L_GRAPH", raising=False)
    monkeypatch.delenv("V4L_EPOCH_GRAPH", raising=False)
    mode = "f16"
    case = dict(REINFORCE_CASES["rf_mlp"], B=16)
    E, T, B, S, A = 4, 8, 16, case["S"], case["A"]
    pf = _policy(case, mode, device)
    buf = DeviceOnPolicyReplayBuffer(max_replay_buffer_size=E * T, env_nums=E, time_limit_filter=True)
    coll = VecOnPolicyCollector(networks.ZeroNet(), env=recipes.ZeroCostVecEnv(E, case, seed=2, p_done=0.2),
                                eval_env=recipes.ZeroCostVecEnv(E, case, seed=3), pf=pf, replay_buffer=buf, device=device,
                                epoch_frames=E * T)
    assert networks.is_zero_critic(coll.vf, pf)
    log = tv._Log()
    common = dict(plr=LR, tau=0.95, shuffle=True, entropy_coeff=rc.ENTROPY_COEFF, env=None, device=device, discount=0.99,
                  num_epochs=10, batch_size=B)
    agent = Reinforce(pf=pf, replay_buffer=buf, collector=coll, logger=log, **common)
    assert agent.vf is coll.vf
    # the twin: equal policy, a host buffer that gets this epoch's transitions
    pf2 = _policy(case, mode, device)
    buf2 = OnPolicyReplayBuffer(max_replay_buffer_size=E * T, env_nums=E, time_limit_filter=True)
    log2 = tv._Log()
    twin = Reinforce(pf=pf2, replay_buffer=buf2, collector=_Coll(), logger=log2, **common)
    for k, v in pf.state_dict().items():
        assert torch.equal(v, pf2.state_dict()[k])
    np.random.seed(3); torch.manual_seed(3); torch.cuda.manual_seed(3)
    coll.train_one_epoch()
    state, _, acts, vals, _ = buf.step_arrays(A)
    torch.cuda.synchronize()
    assert vals.numel() == E * T and (vals == 0).all()  # what the rollout step filed
    obs = state[:, :S].detach().cpu().numpy().astype(np.float64).reshape(T, E, S)
    acts_h = acts.detach().cpu().numpy().astype(np.float64).reshape(T, E, A)
    last_next = buf._last_next_obs
    last_next = (last_next.detach().cpu().numpy() if isinstance(last_next, torch.Tensor) else np.asarray(last_next)).reshape(E, -1)
    for t in range(T):
        buf2.add_sample({"obs": obs[t], "next_obs": last_next, "acts": acts_h[t],
                         "values": np.zeros((E, 1)), "rewards": buf._rewards[t], "terminals": buf._terminals[t],
                         "time_limits": buf._time_limits[t]})
    np.random.seed(7)
    agent.update_per_epoch()
    torch.cuda.synchronize()
    _, _, _, advs, rets, vals2, _ = buf.device_rollout()
    assert (vals2 == 0).all() and torch.equal(advs, rets)
    want = _discount_reward64(np.asarray(buf._rewards, dtype=np.float64), np.asarray(buf._terminals, dtype=np.float64),
                              np.asarray(buf._time_limits, dtype=np.float64), 0.99)
    assert np.array_equal(np.asarray(buf._advs), want.reshape(np.shape(buf._advs)))
    assert np.array_equal(np.asarray(buf._estimate_returns), np.asarray(buf._advs))
    assert np.array_equal(advs.cpu().numpy(), want.reshape(-1).astype(np.float32))
    U = T * E // B
    assert len(log.updates) == U == 2 and all(list(i) == INFO_KEYS for i in log.updates)
    assert agent.training_update_num == U and agent.trainer.adam_steps() == (U, 0) and agent.f16_saturated == 0
    np.random.seed(7)
    twin.update_per_epoch()
    torch.cuda.synchronize()
    assert np.array_equal(buf2._advs, np.asarray(buf._advs)) and log2.updates == log.updates
    for k, v in pf.state_dict().items():
        assert torch.equal(v, pf2.state_dict()[k]), k
    assert any(not torch.equal(v, w) for v, w in zip(pf.state_dict().values(), _policy(case, mode, device).state_dict().values()))


# ------------------------------------------------------------------------------------------ the other learners beside it
def test_others_untouched(device):
    """f16: two updates of a PPO, a V-MPO and an A2C agent on their existing cases give the same bits (sha256 over parameters and
    Adam moments) whether or not a Reinforce trainer was built and run on the same device in between. The digests are recorded
    (util.record: their first 48 bits) so that two commits' values can be compared by hand."""
    from vision4leg_amd.torchrl.algo import PPO
    mode = "f16"

    def other_updates():
        out = {}
        for tag, case, make, batch in (
                ("ppo", util.CASES["mlp_s93"], lambda c: tv._agent(c, mode, device, cls=PPO, clip_para=0.2),
                 lambda c, u: {k: util.make_batch(c, update=u)[k] for k in tv.BATCH_KEYS}),
                ("vmpo", tv.VMPO_CASES["vmpo_mlp"], lambda c: tv._agent(c, mode, device),
                 lambda c, u: {k: util.make_batch(c, update=u)[k] for k in tv.BATCH_KEYS}),
                ("a2c", ac.A2C_CASES["a2c_mlp"], lambda c: ta._agent(c, mode, device), ac.host_batch)):
            agent, pf, vf = make(case)
            if tag != "a2c":
                agent.trainer.sync_target()
            for u in range(2):
                agent.update(batch(case, u))
            torch.cuda.synchronize()
            tr = agent.trainer
            out[tag] = _digest(list(pf.state_dict().values()) + list(vf.state_dict().values()) + [tr.m_pf, tr.v_pf, tr.m_vf, tr.v_vf])
        return out
    first = other_updates()
    case = REINFORCE_CASES["rf_mlp"]
    agent, _ = _agent(case, mode, device)
    for u in range(2):
        agent.update(rc.host_batch(case, u))
    second = other_updates()
    for tag in first:
        print("   %s sha256 %s" % (tag, first[tag]))
        util.record("reinforce/others/%s/sha256_first48bits" % tag, int(first[tag][:12], 16))
        assert first[tag] == second[tag], tag
    del agent
