"""-m gpu: A2C (algo.A2C, the reference's torchrl/algo/on_policy/a2c.py) on the HIP engine for state-MLP nets: one loss
evaluation's gradients and statistics, two updates of every case of tests/a2c_cases.py against the same-mode restatement, the
reference's own fixtures, the resident epoch against update(batch) with its graph counts, and PPO / V-MPO next to an A2C trainer.

The reference arithmetic is a2c_cases.A2COracle (pinned to the unmodified reference by tests/golden/make_golden_a2c.py and
tests/test_a2c_cpu.py). The bounds of test_two_updates are tests/test_gpu_vmpo.py::test_two_updates' (infos 5e-4 / 5e-3 relative to
max(1, |x|), every parameter element 2e-5 / 2.2e-4 (u + 1), the mean 1e-7 / 2e-5 (u + 1); the either-or rule of the 16-bit
modes from the second update on, for Training/policy_loss only): the project's bounds for the same forward, backward and Adam
arithmetic. One loss evaluation is held to tests/test_gpu_parity.py's TOL / REF_DIST, as V-MPO's."""
import numpy as np
import pytest
import torch

import test_gpu_parity as par
import test_gpu_vmpo as tv
import util
import a2c_cases as ac
from a2c_cases import A2C_CASES, FIXTURE_CASES, INFO_KEYS, LR, updates_of

pytestmark = pytest.mark.gpu

MODES = par.MODES
NAMES = list(A2C_CASES)
EITHER_OR = ("Training/policy_loss",)


class _Coll:
    epoch_frames = 1


def _build(case, mode, dev):
    import os
    os.environ["V4L_COMPUTE"] = mode
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    pf, vf = ac.seeded_nets(networks, policies, case)
    return pf.to(dev), vf.to(dev)


def _agent(case, mode, device, **kw):
    from vision4leg_amd.torchrl.algo import A2C
    pf, vf = _build(case, mode, device)
    args = dict(plr=LR, vlr=LR, tau=0.95, shuffle=True, entropy_coeff=ac.ENTROPY_COEFF, env=None, replay_buffer=None,
                collector=_Coll(), logger=None, device=device, discount=0.99, num_epochs=1500, batch_size=case["B"], save_dir=None)
    args.update(kw)
    return A2C(pf=pf, vf=vf, **args), pf, vf


def _oracle(pf, vf, case, mode):
    return ac.oracle_of(pf.state_dict(), vf.state_dict(), case, mode)


def test_surface(device):
    """The reference's attribute surface (a2c.py:22-44, on_rl_algo.py:18-21,43-48): no target_pf, no PPO-only attributes."""
    case = A2C_CASES["a2c_mlp_odd"]
    agent, pf, vf = _agent(case, "f32", device)
    assert agent.sample_key == ["obs", "acts", "advs", "estimate_returns"]
    assert agent.networks == [pf, vf] and agent.snapshot_networks == [("pf", pf), ("vf", vf)]
    for gone in ("target_pf", "clip_para", "opt_epochs", "clipped_value_loss"):
        assert not hasattr(agent, gone), gone
    assert agent.trainer.hp.max_grad_norm == 0.5 and agent.pf_optimizer.param_groups[0]["eps"] == 1e-5
    assert agent.plr == LR and agent.vlr == LR and agent.gae is True and agent.tau == 0.95


# ------------------------------------------------------------------------------------------ one loss evaluation
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["a2c_mlp_odd", "a2c_mlp_tanh", "a2c_mlp_odd@513"])
def test_loss_rows(name, mode, device):
    """a2c_critic_loss_kernel and a2c_loss_kernel through the trainer's eager phases, nothing stepped: d(vf_loss)/d(value) rows,
    d(policy_loss)/d(mean) rows, d/d(logstd) and the 12 statistics against autograd on the restatement. The policy gets distinct
    log sigmas (one beyond the clamp for the Normal policy: its gradient is gated to 0) and means O(1) first.
    Gradients: f32 par.TOL; 16-bit modes: the rows are linear in the head output, whose distance to the fp32 value is capped by
    par.REF_DIST. Statistics: test_two_updates' info bounds.
    "@513" (util.loss_rows_case): the capacity-16 kernels in their 1024-thread block; in f32 with a log sigma below LOG_SIG_MIN
    too (util.loss_rows_both_ends): both ends of the gate exactly 0, and the columns beside that one held to the bound on their
    own (its rows are 1 / sigma^2 = 2.2e4 times theirs and would carry the norm alone)."""
    from vision4leg_amd import _lib
    from vision4leg_amd.engine import HipTrainer
    case = util.loss_rows_case(A2C_CASES, name)
    A, n = case["A"], case["B"]
    tanh = case["kind"].endswith("_tanh")
    agent, pf, vf = _agent(case, mode, device)
    tr = agent.trainer
    both_ends = util.loss_rows_both_ends(name, mode, tanh)
    util.spread_policy_head(pf, util.loss_rows_logstd(A, tanh, both_ends))  # (the last one beyond LOG_SIG_MAX: sigma = e^2, no gradient)
    oracle = _oracle(pf, vf, case, mode)
    dout, dls, dval, oinfo = oracle.loss_grads(*ac.batch_tensors(case, 0))
    b = ac.host_batch(case, 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
    lib = _lib.lib()
    with torch.cuda.device(device):
        hip = pf.hip
        hip.ensure_bound()
        st, im = hip.alloc_rollout(n, device)
        hip.ingest(up(b["obs"]), st, im)
        ro = HipTrainer.rollout(st, im, up(b["acts"]).reshape(n, -1), up(b["advs"]).reshape(n), up(b["estimate_returns"]).reshape(n))
        stats = torch.zeros(1, _lib.V4L_STATS, dtype=torch.float32, device=device)
        astats = torch.zeros(1, _lib.V4L_A2C_STATS, dtype=torch.float32, device=device)
        tr._pre(n)
        tr.begin(None, stats, LR, LR)
        tr.a2c_critic_grads(ro, n, astats)
        torch.cuda.synchronize()
        off = lib.v4l_net_ws_offset(vf.hip.h, n, b"dout")
        vrows = tr.ws[off:off + n * 16].view(n, 16).cpu() / lib.v4l_net_grad_scale(vf.hip.h, n)
        tr.a2c_actor_grads(ro, n, astats)
        torch.cuda.synchronize()
        off = lib.v4l_net_ws_offset(hip.h, n, b"dout")
        rows = tr.ws[off:off + n * 16].view(n, 16).cpu() / lib.v4l_net_grad_scale(hip.h, n)
        got_ls = hip.grad_view(tr.g_pf, "logstd").cpu().reshape(-1)
        rec = astats[0].cpu().numpy()
        ppo_rec = tr.stats_cur().cpu().numpy()
    assert (rows[:, A:] == 0).all() and (vrows[:, 1:] == 0).all()
    tol = par.TOL["f32"] if mode == "f32" else par.REF_DIST[mode]
    e_rows, e_ls, e_val = util.rel_err(rows[:, :A], dout), util.rel_err(got_ls, dls), util.rel_err(vrows[:, :1], dval)
    print("\n[%s %s] rel err d(mean) rows %.2e, d(logstd) %.2e, d(value) rows %.2e" % (name, mode, e_rows, e_ls, e_val))
    util.record("a2c/loss/%s/%s/dmean_rel" % (name, mode), e_rows)
    util.record("a2c/loss/%s/%s/dlogstd_rel" % (name, mode), e_ls)
    util.record("a2c/loss/%s/%s/dvalue_rel" % (name, mode), e_val)
    assert e_rows < tol and e_ls < tol and e_val < tol, (e_rows, e_ls, e_val)
    if not tanh:
        assert got_ls[-1].item() == 0.0 and dls[-1].item() == 0.0
    if both_ends:
        assert got_ls[0].item() == 0.0 and dls[0].item() == 0.0
        assert util.rel_err(rows[:, 1:A], dout[:, 1:]) < tol
    assert (rec[len(INFO_KEYS):] == 0).all()
    for j, k in enumerate(INFO_KEYS):
        print("   %-22s % .6f % .6f" % (k, rec[j], oinfo[k]))
    for j, k in enumerate(INFO_KEYS):
        assert abs(rec[j] - oinfo[k]) <= (5e-4 if mode == "f32" else 5e-3) * max(1.0, abs(oinfo[k])), (k, rec[j], oinfo[k])
    # the PPO record's slots the A2C launches have a value for; the other policy slots stay at the cleared 0
    S = _lib.STAT_KEYS.index
    assert ppo_rec[S("Training/vf_loss")] == rec[1] and ppo_rec[S("Training/policy_loss")] == rec[0] and ppo_rec[S("logprob/mean")] == rec[11]
    for k in ("logprob/std", "logprob/max", "logprob/min", "log_std/mean", "log_std/std", "log_std/max", "log_std/min", "ratio/max", "ratio/min"):
        assert ppo_rec[S(k)] == 0.0, k
    assert ppo_rec[_lib.ST_F16_SAT] == 0.0


# ------------------------------------------------------------------------------------------ updates
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_two_updates(name, mode, device):
    """12 infos and every parameter of pf and vf after each A2C.update call against the same-mode restatement; both Adam step
    counts advance by one per update; nothing saturates in f16."""
    case = A2C_CASES[name]
    agent, pf, vf = _agent(case, mode, device)
    oracle = _oracle(pf, vf, case, mode)
    ref32 = _oracle(pf, vf, case, "f32") if mode != "f32" else None
    for u in range(updates_of(case)):
        before = {k: v.detach().cpu().clone() for k, v in pf.state_dict().items()}
        info = agent.update(ac.host_batch(case, u))
        args = ac.batch_tensors(case, u) + (LR, LR)
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
        for tag, net, onet in (("pf", pf, oracle.pf), ("vf", vf, oracle.vf)):
            for k, v in net.state_dict().items():
                dd = (v.detach().cpu() - onet[k]).abs()
                worst = max(worst, dd.max().item())
                tot += dd.sum().item(); cnt += dd.numel()
        util.record("a2c/update/%s/%s/u%d/worst_abs_param_vs_oracle" % (name, mode, u), worst)
        util.record("a2c/update/%s/%s/u%d/mean_abs_param_vs_oracle" % (name, mode, u), tot / cnt)
        util.record("a2c/update/%s/%s/u%d/max_info_rel_vs_oracle" % (name, mode, u),
                    max(abs(info[k] - oinfo[k]) / max(1.0, abs(oinfo[k])) for k in INFO_KEYS))
        print("   worst |param - restatement| %.3e (bound %.1e), mean %.3e" % (worst, elem, tot / cnt))
        if ref32 is not None:
            far = max((v.detach().cpu() - ref32.pf[k]).abs().max().item() for k, v in pf.state_dict().items())
            far = max(far, max((v.detach().cpu() - ref32.vf[k]).abs().max().item() for k, v in vf.state_dict().items()))
            print("   worst |param - f32 restatement| %.3e" % far)
        assert worst <= elem, (u, worst)
        assert tot / cnt <= (1e-7 if mode == "f32" else 2e-5 * (u + 1))
        assert max((pf.state_dict()[k].cpu() - before[k]).abs().max().item() for k in before) > 5e-5  # the optimiser stepped
        assert (pf.state_dict()["logstd"].cpu() - before["logstd"]).abs().min().item() > 0
        assert agent.trainer.adam_steps() == (u + 1, u + 1) and agent.training_update_num == u + 1
    assert agent.f16_saturated == 0


@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_against_reference_fixture(name, device):
    """f32 mode against what the unmodified reference logged and stepped to (tests/golden/<name>.npz)."""
    case = A2C_CASES[name]
    gold = util.load_golden(name)
    agent, pf, vf = _agent(case, "f32", device)
    for u in range(2):
        info = agent.update(ac.host_batch(case, u))
        for k, want in zip(INFO_KEYS, gold["u%d/info" % u]):
            assert abs(info[k] - want) <= 5e-4 * max(1.0, abs(want)), (u, k, info[k], want)
        seen = 0
        for tag, net in (("pf", pf), ("vf", vf)):
            for k, v in net.state_dict().items():
                key = "u%d/%s/%s" % (u, tag, k)
                if key in gold.files:
                    seen += 1
                    assert np.abs(v.detach().cpu().numpy() - gold[key]).max() <= 2e-5, (u, tag, k)
        assert seen >= 4


def test_optimizer_class_carries_over(device):
    """optimizer_class / optimizer_kwargs reach both optimisers: "AdamW" with weight decay against the restatement on
    torch.optim.AdamW (one update, f32); the plain-Adam restatement is further away."""
    case = A2C_CASES["a2c_mlp_odd"]
    agent, pf, vf = _agent(case, "f32", device, optimizer_class="AdamW", optimizer_kwargs=dict(weight_decay=1.0))
    oracle = ac.oracle_of(pf.state_dict(), vf.state_dict(), case, "f32", optimizer_class=torch.optim.AdamW,
                          optimizer_kwargs=dict(weight_decay=1.0))
    plain = _oracle(pf, vf, case, "f32")
    assert agent.optimizer_class is torch.optim.AdamW
    agent.update(ac.host_batch(case, 0))
    oracle.update(*ac.batch_tensors(case, 0), LR, LR)
    plain.update(*ac.batch_tensors(case, 0), LR, LR)
    near = far = 0.0
    for net, onet, pnet in ((pf, oracle.pf, plain.pf), (vf, oracle.vf, plain.vf)):
        for k, v in net.state_dict().items():
            near = max(near, (v.detach().cpu() - onet[k]).abs().max().item())
            far = max(far, (v.detach().cpu() - pnet[k]).abs().max().item())
    print("\nworst |param - AdamW restatement| %.2e, - Adam restatement %.2e" % (near, far))
    assert near <= 2e-5 and far > near


# ------------------------------------------------------------------------------------------ resident epoch
def _epoch_stack(device, mode="f16"):
    from vision4leg_amd import recipes
    from vision4leg_amd.torchrl.algo import A2C
    from vision4leg_amd.torchrl.collector import VecOnPolicyCollector
    from vision4leg_amd.torchrl.replay_buffers import DeviceOnPolicyReplayBuffer
    case = dict(A2C_CASES["a2c_mlp"], B=32)
    E, T, B = 4, 32, 32  # T * E = 4 * B: four updates in the epoch's one pass
    pf, vf = _build(case, mode, device)
    buf = DeviceOnPolicyReplayBuffer(max_replay_buffer_size=E * T, env_nums=E, time_limit_filter=True)
    coll = VecOnPolicyCollector(vf, env=recipes.ZeroCostVecEnv(E, case, seed=2, p_done=0.1), eval_env=recipes.ZeroCostVecEnv(E, case, seed=3),
                                pf=pf, replay_buffer=buf, device=device, epoch_frames=E * T)
    log = tv._Log()
    agent = A2C(pf=pf, vf=vf, plr=LR, vlr=LR, tau=0.95, shuffle=True, entropy_coeff=ac.ENTROPY_COEFF, env=None,
                replay_buffer=buf, collector=coll, logger=log, device=device, discount=0.99, num_epochs=10, batch_size=B)
    return case, agent, coll, buf, log, pf, vf


def _epochs(device, count, twin=False):
    """`count` epochs of collect + update_per_epoch. twin: a second agent on equal nets gets every minibatch of every epoch, the
    same rows, through update(batch). -> (agent, counts after each epoch, infos, params, twin infos, twin params)."""
    case, agent, coll, buf, log, pf, vf = _epoch_stack(device)
    S = case["S"]
    other = _agent(case, "f16", device) if twin else None
    if twin:
        for k, v in pf.state_dict().items():
            assert torch.equal(v, other[1].state_dict()[k])
    np.random.seed(3); torch.manual_seed(3); torch.cuda.manual_seed(3)
    picked, inner = [], buf.one_iteration

    def one_iteration(*a, **kw):
        for batch in inner(*a, **kw):
            picked.append(np.array(batch["rowidx"], copy=True))
            yield batch
    buf.one_iteration = one_iteration
    counts, twin_infos = [], []
    for e in range(count):
        coll.train_one_epoch()
        if e == 0:
            # the pair shares no parameter: the fused rollout step must have run the critic's OWN base (a pass through the
            # policy's base would be off by the values' own size)
            state, _, _, vals, _ = buf.step_arrays(case["A"])  # (what the rollout step filed; GAE has not run yet)
            want = vf(state[:, :S].contiguous()).reshape(-1)
            assert (vals - want).abs().max().item() <= 2e-2 * want.abs().max().item(), ((vals - want).abs().max().item(), want.abs().max().item())
        del picked[:]
        agent.update_per_epoch()
        torch.cuda.synchronize()
        counts.append(agent.trainer.a2c_graph_counts())
        assert len(picked) == 4
        if twin:
            state, _, acts, advs, rets, _, _ = buf.device_rollout()
            for rows in picked:
                idx = torch.tensor(rows, dtype=torch.long, device=device)
                host = lambda t: t[idx].detach().cpu().numpy()
                twin_infos.append(other[0].update({"obs": host(state)[:, :S], "acts": host(acts), "advs": host(advs).reshape(-1, 1),
                                                   "estimate_returns": host(rets).reshape(-1, 1)}))
    params = lambda a, b: {tag + k: v.detach().cpu().clone() for tag, net in (("pf/", a), ("vf/", b)) for k, v in net.state_dict().items()}
    return agent, counts, log.updates, params(pf, vf), twin_infos, (params(other[1], other[2]) if twin else None)


def test_resident_epoch(device, monkeypatch):
    """update_per_epoch on a DeviceOnPolicyReplayBuffer (E = 4, T = 32, batch 32: T * E = 4 * B, four updates, records read back
    once) gives the bits of the same rows fed one by one through update(batch). Graph counts, by v4l_trainer_update_run's rules:
    the first epoch of a configuration runs update by update (one eager, the single-update graph, three replays), the second
    epoch captures the run and replays it once, a third is one replay and no capture. V4L_EPOCH_GRAPH=0 (one replay per update)
    and V4L_GRAPH=0 (eager, no graph at all) give the same bits."""
    monkeypatch.delenv("V4L_GRAPH", raising=False)
    monkeypatch.delenv("V4L_EPOCH_GRAPH", raising=False)
    agent, counts, infos, params, twin_infos, twin_params = _epochs(device, 3, twin=True)
    assert agent.use_graph and len(infos) == 12 and agent.training_update_num == 12 and all(list(i) == INFO_KEYS for i in infos)
    assert agent.trainer.adam_steps() == (12, 12) and agent.f16_saturated == 0
    print("\n(captures, replays) after each epoch: %s" % counts)
    assert counts == [(1, 3), (2, 4), (2, 5)]
    assert infos == twin_infos
    for k in params:
        assert torch.equal(params[k], twin_params[k]), k
    assert np.isfinite([v for i in infos for v in i.values()]).all()
    monkeypatch.setenv("V4L_EPOCH_GRAPH", "0")
    _, counts_u, infos_u, params_u, _, _ = _epochs(device, 3)
    assert counts_u == [(1, 3), (1, 7), (1, 11)]
    monkeypatch.delenv("V4L_EPOCH_GRAPH")
    monkeypatch.setenv("V4L_GRAPH", "0")
    eager, counts_e, infos_e, params_e, _, _ = _epochs(device, 3)
    assert not eager.use_graph and counts_e == [(0, 0)] * 3
    for other_infos, other_params in ((infos_u, params_u), (infos_e, params_e)):
        assert infos == other_infos
        for k in params:
            assert torch.equal(params[k], other_params[k]), k


def test_tripwire(device):
    """A NaN advantage reaches the PPO record's slots the A2C launches fill: _check_update_records raises."""
    case = A2C_CASES["a2c_mlp_odd"]
    agent, pf, vf = _agent(case, "f32", device)
    b = ac.host_batch(case, 0)
    b["advs"] = b["advs"].copy()
    b["advs"][3, 0] = np.nan
    with pytest.raises(FloatingPointError, match="non-finite training statistics"):
        agent.update(b)


# ------------------------------------------------------------------------------------------ PPO and V-MPO beside it
def test_ppo_and_vmpo_untouched(device):
    """A PPO update and a V-MPO update give identical bits whether or not an A2C agent was built and run on the same device in
    the process."""
    from vision4leg_amd.torchrl.algo import PPO
    mode = "f16"

    def other_updates():
        out = {}
        for tag, case, kw in (("ppo", util.CASES["mlp_s93"], dict(cls=PPO, clip_para=0.2)), ("vmpo", tv.VMPO_CASES["vmpo_mlp"], {})):
            agent, pf, vf = tv._agent(case, mode, device, **kw)
            agent.trainer.sync_target()
            b = util.make_batch(case, update=0)
            out[tag] = (agent.update({k: b[k] for k in tv.BATCH_KEYS}),
                        {t + k: v.detach().cpu().clone() for t, net in (("pf/", pf), ("vf/", vf)) for k, v in net.state_dict().items()})
        return out
    first = other_updates()
    case = A2C_CASES["a2c_mlp"]
    agent, _, _ = _agent(case, mode, device)
    for u in range(2):
        agent.update(ac.host_batch(case, u))
    second = other_updates()
    for tag in first:
        assert first[tag][0] == second[tag][0], tag
        for k in first[tag][1]:
            assert torch.equal(first[tag][1][k], second[tag][1][k]), (tag, k)
    del agent
