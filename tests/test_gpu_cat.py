"""-m gpu: the discrete policy (policies.CategoricalDisPolicy, the reference's torchrl/policies/discrete_policies.py:127-172) on the
HIP engine under algo.A2C and algo.Reinforce: the categorical head and the sampling kernel, one loss evaluation's d(out) rows
and statistics, two updates of every case of tests/cat_cases.py against the same-mode restatement and the reference's own
fixtures, graph replays against eager launches, the launch count against the Gaussian learners', the rollout step, and the
training loop over a discrete vec env with the resident and the host buffer.

The reference arithmetic is cat_cases.CatOracle / CatReinforceOracle (pinned to the unmodified reference by
tests/golden/make_golden_cat.py and tests/test_cat_cpu.py). No bound here is new: the forward is held to tests/test_gpu_parity.py's
f32 gate and, in the 16-bit modes, to the envelope rule tests/test_gpu_tact.py::test_forward_and_gauss_head imports; one loss
evaluation to par.TOL / par.REF_DIST and the updates to the statements of tests/test_gpu_a2c.py::test_two_updates (infos 5e-4 /
5e-3 relative to max(1, |x|), every parameter element 2e-5 / 2.2e-4 (u + 1), the mean 1e-7 / 2e-5 (u + 1), the either-or rule of
the 16-bit modes from the second update on for Training/policy_loss only); the training loop to
tests/test_gpu_wide_actions.py::test_train_loop_buffers_and_resume's tolerance.

What the head adds to a forward distance is propagated, not measured: with dz the largest distance between two sets of logits,
|d log p_j| <= 2 dz (log-softmax is 2-Lipschitz in the max norm), |d p_j| <= 2 dz p_j <= 2 dz and, to first order,
|d H| <= 2 dz sum_j p_j (|log p_j| + 1) <= 2 dz (H + 1); the tests allow twice the first-order entropy term."""
import collections
import hashlib
import os

import numpy as np
import pytest
import torch

import test_gpu_parity as par
import test_gpu_resume as rsm
import test_gpu_update_route as route
import test_gpu_wide_actions as wide
import util
import a2c_cases as ac
import reinforce_cases as rc
import cat_cases as cc
from cat_cases import CAT_CASES, LR, updates_of
from oracle import ppo_oracle as orc

pytestmark = pytest.mark.gpu

MODES = par.MODES
NAMES = list(CAT_CASES)
LEARNERS = ("a2c", "rf")
EITHER_OR = ("Training/policy_loss",)
EPS32 = float(np.finfo(np.float32).eps)


class _Coll:
    epoch_frames = 1


def _build(case, mode, dev):
    os.environ["V4L_COMPUTE"] = mode
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    pf, vf = cc.seeded_nets(networks, policies, case)
    return pf.to(dev), vf.to(dev)


def _agent(learner, case, mode, device, **kw):
    """-> (agent, pf, vf): algo.A2C on the case's pair, or algo.Reinforce on its policy (vf = the agent's zero critic)."""
    from vision4leg_amd.torchrl.algo import A2C, Reinforce
    pf, vf = _build(case, mode, device)
    args = dict(plr=LR, tau=0.95, shuffle=True, entropy_coeff=cc.ENTROPY_COEFF, env=None, replay_buffer=None, collector=_Coll(),
                logger=None, device=device, discount=0.99, num_epochs=1500, batch_size=case["B"], save_dir=None)
    args.update(kw)
    if learner == "a2c":
        return A2C(pf=pf, vf=vf, vlr=LR, **args), pf, vf
    agent = Reinforce(pf=pf, **args)
    return agent, pf, agent.vf


def _oracle(learner, pf, vf, case, mode):
    if learner == "a2c":
        return cc.a2c_oracle_of(pf.state_dict(), vf.state_dict(), case, mode)
    return cc.rf_oracle_of(pf.state_dict(), case, mode)


def _oracle_update(learner, oracle, case, u):
    args = cc.batch_tensors(case, u)
    return oracle.update(*args, LR, LR) if learner == "a2c" else oracle.update(*args, LR)


def _info_keys(learner):
    return cc.A2C_INFO_KEYS if learner == "a2c" else cc.RF_INFO_KEYS


def _up(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)


def _sd_cpu(net):
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


# ------------------------------------------------------------------------------------------ head
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_head(name, mode, device):
    """v4l_cat_head and the module's forward / update. The logits against the same-mode restatement (f32 gate / the
    restatement's own envelope); probabilities, log-prob and entropy against the restatement within what that logits distance
    propagates to (module docstring), and against float64 on the engine's OWN logits to fp32 rounding; cat_mlp's mean entropy
    and log-prob against what the reference logged at its first update (the fixture: par.TOL f32 / par.REF_DIST)."""
    case = CAT_CASES[name]
    K, n = case["K"], case["B"]
    pf, vf = _build(case, mode, device)
    obs, acts, _, _ = cc.batch_tensors(case, 0)
    with torch.cuda.device(device):
        probs = pf(obs.to(device))
        up = pf.update(obs.to(device), acts.to(device))
        hip = pf.hip
        st, im, _ = hip.stage(obs.to(device))
        out = hip.forward(st, im, n)
        assert bool((out[:, K:] == 0).all())
        logits = out[:, :K].cpu().clone()
        raw = hip.cat_head(out, n, acts.to(device))
        torch.cuda.synchronize()
    assert tuple(probs.shape) == (n, K) and tuple(up["log_prob"].shape) == (n, 1) and tuple(up["ent"].shape) == (n,)
    assert isinstance(up["dis"], torch.distributions.Categorical) and list(up) == ["dis", "log_prob", "ent"]
    assert torch.equal(raw[0], probs) and torch.equal(raw[1], up["ent"]) and torch.equal(raw[2], up["log_prob"].view(n))
    params = {k: v.detach().cpu() for k, v in pf.state_dict().items()}
    with torch.no_grad():
        ologits = orc.FORWARDS[case["kind"]](params, obs, case["S"], mode)
        op, olp, oent = cc.head(ologits, acts)
        p64, lp64, ent64 = cc.head(logits.double(), acts)
    ez = util.rel_err(logits, ologits)
    print("\n[%s %s] logits rel err vs %s-restatement %.2e" % (name, mode, mode, ez))
    util.record("cat/head/%s/%s/logits_vs_oracle" % (name, mode), ez)
    if mode == "f32":
        assert ez < par.TOL[mode], ez
    else:
        env = wide._forward_envelope("cat/" + name + "/pf", mode, params, obs, case)
        assert ez <= max(par.ENV_FACTOR * env, par.ENV_FLOOR), (ez, env)
    dz = (logits - ologits).abs().max().item()
    p, lp, ent = probs.cpu(), up["log_prob"].cpu(), up["ent"].cpu()
    assert (p - op).abs().max().item() <= 2 * dz + 4 * EPS32
    assert (lp - olp).abs().max().item() <= 2 * dz + 1e-5
    assert ((ent - oent).abs() <= 4 * dz * (oent + 1.0) + 1e-5).all()
    # the kernel's own arithmetic, on the logits it read: fp32 log-softmax by max-subtraction
    assert torch.allclose(p.double(), p64, rtol=1e-5, atol=1e-7) and torch.allclose(lp.double(), lp64, rtol=1e-5, atol=1e-5)
    assert torch.allclose(ent.double(), ent64, rtol=1e-5, atol=1e-5)
    assert torch.allclose(p.sum(1), torch.ones(n), atol=1e-5) and bool((p > 0).all())
    assert cc.P_MAX_RANGE[0] <= p.max().item() and ent.mean().item() < 0.9 * np.log(K)  # a sharpened head, not the uniform one
    if name == cc.FIXTURE_CASE:
        gold = util.load_golden(cc.FIXTURES["a2c"])["u0/info"]
        cap = par.TOL["f32"] if mode == "f32" else par.REF_DIST[mode]
        for key, got in (("ent", ent.mean().item()), ("log_prob", lp.mean().item())):
            want = gold[cc.A2C_INFO_KEYS.index(key)]
            assert abs(got - want) <= cap * max(1.0, abs(want)), (key, got, want)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_sample(name, mode, device):
    """v4l_cat_sample on the case's 4096 uniforms equals the numpy inverse CDF (float64 running sums of the fp32 probabilities)
    on every row outside the 1e-6 boundary band, which holds at most 1 % of the rows (tests/test_cat_cpu.py); its
    deterministic output is the argmax. explore() draws torch.rand on the device's generator and returns int64 indices with
    their log-probs; eval_act is the argmax as numpy."""
    from vision4leg_amd import engine
    case = CAT_CASES[name]
    K, n = case["K"], case["B"]
    pf, vf = _build(case, mode, device)
    obs = cc.batch_tensors(case, 0)[0].to(device)
    u = cc.uniforms(case)
    with torch.cuda.device(device):
        probs = pf(obs)
        rows = probs[torch.arange(len(u), device=device) % n].contiguous()
        idx = engine.cat_sample(rows, torch.from_numpy(u).to(device)).cpu().numpy()
        det = engine.cat_sample(rows, deterministic=True).cpu().numpy()
        torch.manual_seed(5)
        ex = pf.explore(obs, return_log_probs=True)
        torch.manual_seed(5)
        drawn = torch.rand(n, dtype=torch.float32, device=device).cpu().numpy()
        ev = pf.eval_act(obs)
        torch.cuda.synchronize()
    rows = rows.cpu().numpy()
    want, dist = cc.inverse_cdf(rows, u)
    clear = dist > 1e-6
    print("\n[%s %s] %d of %d rows inside the boundary band" % (name, mode, int((~clear).sum()), len(u)))
    assert clear.mean() >= 0.99 and idx.dtype == np.int64
    assert (idx[clear] == want[clear]).all() and idx.min() >= 0 and idx.max() < K
    assert (det == rows.argmax(axis=1)).all()
    assert list(ex) == ["dis", "action", "log_prob"] and ex["action"].dtype == torch.int64 and tuple(ex["action"].shape) == (n,)
    assert torch.equal(ex["dis"], probs)
    a = ex["action"].cpu().numpy()
    w2, d2 = cc.inverse_cdf(probs.cpu().numpy(), drawn)
    assert (a[d2 > 1e-6] == w2[d2 > 1e-6]).all()
    picked = probs.cpu().numpy()[np.arange(n), a].astype(np.float64)
    assert np.abs(ex["log_prob"].cpu().numpy() - np.log(picked)).max() <= 1e-5
    assert isinstance(ev, np.ndarray) and ev.shape == (n,) and (ev == probs.cpu().numpy().argmax(axis=1)).all()


def test_setter_refuses_a_bound_net(device):
    """The one refusal of v4l_net_set_categorical that needs a device (tests/test_cat_cpu.py has the others)."""
    from vision4leg_amd import _lib
    pf, _ = _build(CAT_CASES["cat_mlp_k2"], "f32", device)
    l = _lib.lib()
    with torch.cuda.device(device):
        pf.hip.ensure_bound()
    assert l.v4l_net_set_categorical(pf.hip.h, 0) != 0 and "bound already" in l.v4l_last_error().decode()


# ------------------------------------------------------------------------------------------ one loss evaluation
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("learner", LEARNERS)
def test_loss_grads(learner, name, mode, device):
    """a2c_cat_loss_kernel / reinforce_cat_loss_kernel through the trainer's eager phases, nothing stepped: the d(out) rows
    against autograd on the restatement (f32 par.TOL, 16-bit par.REF_DIST: tests/test_gpu_a2c.py::test_loss_rows' bounds), the
    padded columns K .. 15 exactly zero, the statistics to test_two_updates' info bounds; the A2C record's std/* slots and every
    slot past the keys stay as cleared."""
    from vision4leg_amd import _lib
    from vision4leg_amd.engine import HipTrainer
    case = CAT_CASES[name]
    K, n = case["K"], case["B"]
    agent, pf, vf = _agent(learner, case, mode, device)
    tr = agent.trainer
    oracle = _oracle(learner, pf, vf, case, mode)
    got = oracle.loss_grads(*cc.batch_tensors(case, 0))
    dout, oinfo = got[0], got[-1]
    b = cc.host_batch(case, 0)
    lib = _lib.lib()
    with torch.cuda.device(device):
        hip = pf.hip
        hip.ensure_bound()
        st, im = hip.alloc_rollout(n, device)
        hip.ingest(_up(b["obs"], device), st, im)
        ro = HipTrainer.rollout(st, im, _up(b["acts"], device).reshape(n, 1), _up(b["advs"], device).reshape(n),
                                _up(b["estimate_returns"], device).reshape(n))
        stats = torch.zeros(1, _lib.V4L_STATS, dtype=torch.float32, device=device)
        tr._pre(n)
        tr.begin(None, stats, LR, LR)
        if learner == "a2c":
            second = torch.zeros(1, _lib.V4L_A2C_STATS, dtype=torch.float32, device=device)
            tr.a2c_critic_grads(ro, n, second)
            tr.a2c_actor_grads(ro, n, second)
            rec_keys = _lib.A2C_INFO_KEYS
        else:
            second = torch.zeros(1, _lib.V4L_REINFORCE_STATS, dtype=torch.float32, device=device)
            tr.reinforce_actor_grads(ro, n, second)
            rec_keys = _lib.REINFORCE_INFO_KEYS
        torch.cuda.synchronize()
        off = lib.v4l_net_ws_offset(hip.h, n, b"dout")
        rows = tr.ws[off:off + n * 16].view(n, 16).cpu() / lib.v4l_net_grad_scale(hip.h, n)
        rec = second[0].cpu().numpy()
        ppo_rec = tr.stats_cur().cpu().numpy()
    assert (rows[:, K:] == 0).all()
    tol = par.TOL["f32"] if mode == "f32" else par.REF_DIST[mode]
    e_rows = util.rel_err(rows[:, :K], dout)
    print("\n[%s %s %s] rel err d(out) rows %.2e (bound %.1e)" % (learner, name, mode, e_rows, tol))
    util.record("cat/loss/%s/%s/%s/dout_rel" % (learner, name, mode), e_rows)
    assert e_rows < tol, e_rows
    assert abs(rows[:, :K].sum(1)).max().item() <= 1e-6 * max(1.0, rows.abs().max().item())  # a softmax gradient row sums to 0
    for j, k in enumerate(rec_keys):
        if k in oinfo:
            print("   %-22s % .6f % .6f" % (k, rec[j], oinfo[k]))
            assert abs(rec[j] - oinfo[k]) <= (5e-4 if mode == "f32" else 5e-3) * max(1.0, abs(oinfo[k])), (k, rec[j], oinfo[k])
        else:
            assert k.startswith("std/") and rec[j] == 0.0, k
    assert set(oinfo) <= set(rec_keys) and (rec[len(rec_keys):] == 0).all()
    S = _lib.STAT_KEYS.index
    assert ppo_rec[S("Training/policy_loss")] == rec[rec_keys.index("Training/policy_loss")]
    for k in ("log_std/mean", "log_std/std", "log_std/max", "log_std/min", "ratio/max", "ratio/min"):
        assert ppo_rec[S(k)] == 0.0, k
    assert ppo_rec[_lib.ST_F16_SAT] == 0.0


# ------------------------------------------------------------------------------------------ updates
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("learner", LEARNERS)
def test_two_updates(learner, name, mode, device):
    """tests/test_gpu_a2c.py::test_two_updates' statements (and its REINFORCE twin's) for the categorical policy: the infos (8 of
    A2C's, Reinforce's 10) and every parameter after each update against the same-mode restatement; under Reinforce the zero
    critic's own parameters keep their bits and its Adam count stays 0; nothing saturates in f16."""
    case = CAT_CASES[name]
    keys = _info_keys(learner)
    agent, pf, vf = _agent(learner, case, mode, device)
    oracle = _oracle(learner, pf, vf, case, mode)
    ref32 = _oracle(learner, pf, vf, case, "f32") if mode != "f32" else None
    shared = {id(p) for p in pf.parameters()}
    own_vf = {k: p.detach().clone() for k, p in vf.named_parameters() if id(p) not in shared}
    nets = (("pf", pf, oracle.pf),) + ((("vf", vf, oracle.vf),) if learner == "a2c" else ())
    for u in range(updates_of(case)):
        before = _sd_cpu(pf)
        info = agent.update(cc.host_batch(case, u))
        oinfo = _oracle_update(learner, oracle, case, u)
        ginfo = _oracle_update(learner, ref32, case, u) if ref32 is not None else None
        assert list(info) == keys
        print("\n[%s %s %s] update %d info (hip / restatement%s):" % (learner, name, mode, u, "" if ginfo is None else " / f32 restatement"))
        for k in keys:
            print("   %-22s % .6f % .6f%s" % (k, info[k], oinfo[k], "" if ginfo is None else " % .6f" % ginfo[k]))
        for k in keys:
            tol = (5e-4 if mode == "f32" else 5e-3) * max(1.0, abs(oinfo[k]))
            strict_ok = abs(info[k] - oinfo[k]) <= tol
            if mode != "f32" and u >= 1 and k in EITHER_OR:
                assert strict_ok or abs(info[k] - ginfo[k]) <= 5e-2 * max(1.0, abs(ginfo[k])), (u, k, info[k], oinfo[k], ginfo[k])
                continue
            assert strict_ok, (u, k, info[k], oinfo[k], None if ginfo is None else ginfo[k])
        elem = 2e-5 if mode == "f32" else 2.2e-4 * (u + 1)
        worst, tot, cnt = 0.0, 0.0, 0
        for tag, net, onet in nets:
            for k, v in net.state_dict().items():
                dd = (v.detach().cpu() - onet[k]).abs()
                worst = max(worst, dd.max().item())
                tot += dd.sum().item(); cnt += dd.numel()
        util.record("cat/update/%s/%s/%s/u%d/worst_abs_param_vs_oracle" % (learner, name, mode, u), worst)
        util.record("cat/update/%s/%s/%s/u%d/mean_abs_param_vs_oracle" % (learner, name, mode, u), tot / cnt)
        print("   worst |param - restatement| %.3e (bound %.1e), mean %.3e" % (worst, elem, tot / cnt))
        assert worst <= elem, (u, worst)
        assert tot / cnt <= (1e-7 if mode == "f32" else 2e-5 * (u + 1))
        assert max((pf.state_dict()[k].cpu() - before[k]).abs().max().item() for k in before) > 5e-5  # the optimiser stepped
        assert agent.trainer.adam_steps() == ((u + 1, u + 1) if learner == "a2c" else (u + 1, 0))
        assert agent.training_update_num == u + 1
    if learner == "rf":
        assert own_vf and all(torch.equal(p.detach(), own_vf[k]) for k, p in vf.named_parameters() if k in own_vf)
        assert not agent.trainer.m_vf.any() and not agent.trainer.v_vf.any()
    assert agent.f16_saturated == 0


@pytest.mark.parametrize("learner", LEARNERS)
def test_against_reference_fixture(learner, device):
    """f32 mode against what the unmodified reference logged and stepped to (tests/golden/a2c_cat_mlp.npz, rf_cat_mlp.npz):
    tests/test_gpu_a2c.py::test_against_reference_fixture's bounds."""
    case = CAT_CASES[cc.FIXTURE_CASE]
    gold = util.load_golden(cc.FIXTURES[learner])
    keys = _info_keys(learner)
    agent, pf, vf = _agent(learner, case, "f32", device)
    for u in range(2):
        info = agent.update(cc.host_batch(case, u))
        assert list(info) == keys
        for k, want in zip(keys, gold["u%d/info" % u]):
            assert abs(info[k] - want) <= 5e-4 * max(1.0, abs(want)), (u, k, info[k], want)
        seen = 0
        for tag, net in (("pf", pf),) + ((("vf", vf),) if learner == "a2c" else ()):
            for k, v in net.state_dict().items():
                key = "u%d/%s/%s" % (u, tag, k)
                if key in gold.files:
                    seen += 1
                    assert np.abs(v.detach().cpu().numpy() - gold[key]).max() <= 2e-5, (u, tag, k)
        assert seen >= (4 if learner == "a2c" else 2)


# ------------------------------------------------------------------------------------------ graphs and launches
def _digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def _run_three(learner, case, device, U=3, runs=2):
    """tests/test_gpu_reinforce.py::_run_three for either learner: `runs` runs of U updates on the rows of U seeded minibatches
    through the shell's _run on a device rollout -> (per run: infos, digest of parameters and moments), graph counts per run."""
    from vision4leg_amd.engine import HipTrainer
    agent, pf, vf = _agent(learner, case, "f16", device)
    n = case["B"]
    bs = [cc.host_batch(case, u) for u in range(U)]
    out, counts = [], []
    with torch.cuda.device(device):
        hip = pf.hip
        hip.ensure_bound()
        st, im = hip.alloc_rollout(U * n, device)
        hip.ingest(_up(np.concatenate([b["obs"] for b in bs]), device), st, im)
        cat = lambda k: _up(np.concatenate([b[k] for b in bs]), device)
        ro = HipTrainer.rollout(st, im, cat("acts").reshape(U * n, 1), cat("advs").reshape(-1), cat("estimate_returns").reshape(-1))
        rowidx = torch.arange(U * n, dtype=torch.int32, device=device).view(U, n).flip(0).contiguous()
        tr = agent.trainer
        for _ in range(runs):
            infos = agent._run(ro, rowidx, n, U, lambda u: "update %d" % u)
            torch.cuda.synchronize()
            counts.append(tr.a2c_graph_counts() if learner == "a2c" else tr.reinforce_graph_counts())
            out.append((infos, _digest(list(pf.state_dict().values()) + list(vf.state_dict().values())
                                       + [tr.m_pf, tr.v_pf, tr.m_vf, tr.v_vf])))
    return out, counts


@pytest.mark.parametrize("learner", LEARNERS)
def test_run_equals_eager(learner, device, monkeypatch):
    """U = 3 updates twice (f16, cat_mlp): the graphed epoch (V4L_EPOCH_GRAPH default: the second run is one capture and one
    replay of the whole run), one replay per update (V4L_EPOCH_GRAPH=0) and eager launches (V4L_GRAPH=0) give bit-identical
    parameters, moments and records: the categorical loss kernels reduce in a fixed order, without float atomics."""
    case = CAT_CASES["cat_mlp"]
    monkeypatch.delenv("V4L_GRAPH", raising=False)
    monkeypatch.delenv("V4L_EPOCH_GRAPH", raising=False)
    run, counts = _run_three(learner, case, device)
    print("\n(captures, replays) after each run: %s" % counts)
    assert counts == [(1, 2), (2, 3)]
    assert np.isfinite([v for i in run[1][0] for v in i.values()]).all() and all(list(i) == _info_keys(learner) for i in run[1][0])
    monkeypatch.setenv("V4L_EPOCH_GRAPH", "0")
    per_update, counts_u = _run_three(learner, case, device)
    assert counts_u == [(1, 2), (1, 5)]
    monkeypatch.delenv("V4L_EPOCH_GRAPH")
    monkeypatch.setenv("V4L_GRAPH", "0")
    eager, counts_e = _run_three(learner, case, device)
    assert counts_e == [(0, 0), (0, 0)]
    for other in (per_update, eager):
        for r in range(2):
            assert run[r][0] == other[r][0], r
            assert run[r][1] == other[r][1], r


def _gauss_agent(learner, mode, device):
    """The Gaussian learner on the net of cat_mlp (S = 93, six head columns, [256, 256] / [256, 256]): a2c_cases' a2c_mlp pair,
    reinforce_cases' rf_mlp policy."""
    import test_gpu_a2c as ta
    import test_gpu_reinforce as trf
    if learner == "a2c":
        case = ac.A2C_CASES["a2c_mlp"]
        return ta._agent(case, mode, device)[0], [ac.host_batch(case, u) for u in range(2)]
    case = rc.REINFORCE_CASES["rf_mlp"]
    return trf._agent(case, mode, device)[0], [rc.host_batch(case, u) for u in range(2)]


@pytest.mark.parametrize("learner", LEARNERS)
def test_launch_count_is_the_gaussian_learners(learner, device):
    """One update of the categorical learner launches what the Gaussian learner launches for the same net: the same labels with
    the same call counts, read from the library's profiler for both (no literal): the categorical loss takes the Gaussian loss's
    launch position and adds none."""
    case = CAT_CASES["cat_mlp"]
    g = ac.A2C_CASES["a2c_mlp"] if learner == "a2c" else rc.REINFORCE_CASES["rf_mlp"]
    assert (g["S"], g["A"], g["enc"], g["head"], g["B"]) == (case["S"], case["K"], case["enc"], case["head"], case["B"])

    def profile(agent, batches):
        agent.update(batches[0])
        return route._profiled(lambda: agent.update(batches[1]))

    def both():
        gauss = profile(*_gauss_agent(learner, "f16", device))
        agent = _agent(learner, case, "f16", device)[0]
        return gauss, profile(agent, [cc.host_batch(case, u) for u in range(2)])
    gauss, cat = route._with_env("f16", {}, both)
    calls = lambda rows: sum(r[1] for r in rows)
    print("\n[%s] launches per update: Gaussian %d, categorical %d" % (learner, calls(gauss), calls(cat)))
    assert calls(cat) == calls(gauss) > 0
    assert [r[:2] for r in cat] == [r[:2] for r in gauss]


# ------------------------------------------------------------------------------------------ rollout step
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("E", [1, 17, 65])
@pytest.mark.parametrize("learner", LEARNERS)
def test_rollout_step(learner, E, mode, device):
    """RolloutActor.step on the A2C pair (no common parameter) and on the Reinforce pair (zero_critic(pf): a shared trunk, which
    for a Gaussian policy of this geometry picks a fused state-MLP route): both report GENERAL. Two sampled steps and a
    deterministic one. The step's action equals explore()'s under the same seed and both equal the numpy inverse CDF of the
    uniforms the kernel consumed (actor.eps), on every row whose uniform is further than `band` from a boundary; value and the
    filed log pi_old against vf(ob) and pf.update(ob, action); filing; the deterministic step and eval_act are the argmax.
    tol: tests/test_gpu_sd.py::test_rollout_step's rule for two routes' head outputs (1e-5 f32, 4e-3 16-bit, of max(1, |x|));
    band = 2 tol max(1, |logits|): a logits distance dz moves a running sum of probabilities by at most 2 dz."""
    from vision4leg_amd.torchrl.policies import RolloutActor
    import vision4leg_amd.torchrl.networks as networks
    case = CAT_CASES["cat_mlp"]
    K = case["K"]
    pf, vf = _build(case, mode, device)
    if learner == "rf":
        vf = networks.zero_critic(pf)
    T = 3
    with torch.cuda.device(device):
        net = pf.hip
        net.ensure_bound()
        slots = (T + 1) * E
        state, image = net.alloc_rollout(slots, device)
        SENT = -7.0
        acts = torch.full((slots, 1), SENT, device=device)
        vals, logp = torch.full((slots,), SENT, device=device), torch.full((slots,), SENT, device=device)
        obs = torch.tensor(util.obs_rows(np.random.RandomState(3), T * E, case), dtype=torch.float32, device=device)
        ra = RolloutActor(pf, vf, E)
        actor = ra._actor
        assert actor.shared_encoder == (learner == "rf") and tuple(actor.eps.shape) == (E, 1)
        assert actor.route() == "GENERAL" and sorted(actor._out) == ["action", "ent", "value"]
        actor.attach((state, image, acts, vals, logp))
        actor.seek(0)
        tol = 1e-5 if mode == "f32" else 4e-3
        checked = 0
        for s in range(T):
            det = s == T - 1
            ob = obs[s * E:(s + 1) * E]
            sl = slice(s * E, (s + 1) * E)
            torch.manual_seed(100 + s)
            actor.step(ob, deterministic=det)
            torch.cuda.synchronize()
            out = {k: v.clone() for k, v in actor._out.items()}
            u = actor.eps.clone().view(E).cpu().numpy()
            assert bool((u == -1).all()) == det and (det or ((u >= 0).all() and (u < 1).all()))
            torch.manual_seed(100 + s)
            ex = pf.explore(ob, return_log_probs=True)
            sep_value = vf(ob).view(E)
            up = pf.update(ob, acts[sl].view(E))
            st_, im_, _ = net.stage(ob)
            zmax = max(1.0, net.forward(st_, im_, E)[:, :K].abs().max().item())
            torch.cuda.synchronize()
            action = out["action"].view(E).cpu().numpy()
            assert tuple(out["action"].shape) == (E, 1) and (action == np.round(action)).all() and action.min() >= 0 and action.max() < K
            probs = ex["dis"].cpu().numpy()
            if det:
                top2 = np.sort(probs, axis=1)[:, -2:]
                sure = (top2[:, 1] - top2[:, 0]) > 4 * tol * zmax
                assert (action[sure] == probs.argmax(axis=1)[sure]).all() and (action[sure] == pf.eval_act(ob)[sure]).all()
            else:
                want, dist = cc.inverse_cdf(probs, u)
                clear = dist > 2 * tol * zmax
                checked += int(clear.sum())
                assert (action[clear] == want[clear]).all() and (ex["action"].cpu().numpy()[clear] == want[clear]).all()
            assert (out["value"].view(E) - sep_value).abs().max().item() <= tol * max(1.0, sep_value.abs().max().item())
            if learner == "rf":
                assert bool((out["value"] == 0).all())
            assert (logp[sl] - up["log_prob"].view(E)).abs().max().item() <= 2 * tol * zmax + 1e-5
            assert (out["ent"].view(E) - up["ent"]).abs().max().item() <= 4 * tol * zmax * (up["ent"].max().item() + 1.0) + 1e-5
            # filing: this step's slots hold what the step returned, the later ones the sentinel
            assert torch.equal(acts[sl], out["action"]) and torch.equal(vals[sl], out["value"].view(E)) and bool((logp[sl] != SENT).all())
            assert bool((acts[(s + 1) * E:] == SENT).all()) and bool((vals[(s + 1) * E:] == SENT).all()) and bool((logp[(s + 1) * E:] == SENT).all())
        assert checked >= (T - 1) * E * 0.5
        if E == 1:
            a1 = RolloutActor(pf, vf, 1).eval_act(obs[:1])
            assert a1.shape == (1,) and int(a1[0]) == int(pf.eval_act(obs[:1])[0])


# ------------------------------------------------------------------------------------------ training loop
class DiscreteFakeVecEnv:
    """A deterministic vec env with a discrete action space (action_space.n = K) in the reference's vec-env protocol
    (tests/util.FakeVecEnv's): it checks every action array it is handed (int64 [E] in [0, K)) and its rewards and next
    observations depend on the actions, so a collector that feeds other actions diverges."""

    Space = collections.namedtuple("Space", "n")

    def __init__(self, E, S, K, seed=0, p_done=0.1):
        self.env_nums, self.S, self.K = E, S, K
        self.rs = np.random.RandomState(seed)
        self.action_space = self.Space(K)
        self.p_done, self.training, self.closed, self._reward_scale = p_done, True, False, 1
        self.log = []

    def _rows(self, n):
        return np.clip(self.rs.randn(n, self.S), -10, 10)

    def train(self):
        self.training = True

    def eval(self):
        self.training = False

    def reset(self):
        self.ob = self._rows(self.env_nums)
        return self.ob.copy()

    def step(self, acts):
        assert isinstance(acts, np.ndarray) and acts.dtype == np.int64 and acts.shape == (self.env_nums,), (type(acts), getattr(acts, "dtype", None), np.shape(acts))
        assert acts.min() >= 0 and acts.max() < self.K
        self.log.append(acts.copy())
        self.ob = self._rows(self.env_nums)
        self.ob[:, 0] += 0.5 * (acts % 3 - 1)
        rewards = (acts % 3 - 1.0).reshape(-1, 1) + self.rs.randn(self.env_nums, 1)
        dones = self.rs.rand(self.env_nums, 1) < self.p_done
        return self.ob.copy(), rewards, dones, {"time_limit": self.rs.rand(self.env_nums) < 0.05}

    def partial_reset(self, mask):
        mask = np.asarray(mask, dtype=bool).reshape(-1)
        self.ob[mask] = self._rows(int(mask.sum()))
        return self.ob.copy()

    def close(self):
        self.closed = True


LOOP_CASE = dict(CAT_CASES["cat_mlp_k16"], B=32)


def _loop_agent(learner, device, buffer, save_dir, E, T, B, num_epochs):
    from vision4leg_amd.torchrl.algo import A2C, Reinforce
    from vision4leg_amd.torchrl.collector import VecOnPolicyCollector
    import vision4leg_amd.torchrl.networks as networks
    from vision4leg_amd.torchrl.replay_buffers import DeviceOnPolicyReplayBuffer, OnPolicyReplayBuffer
    case = LOOP_CASE
    pf, vf = _build(case, "f16", device)
    env = DiscreteFakeVecEnv(E, case["S"], case["K"], seed=9, p_done=0.12)
    eval_env = DiscreteFakeVecEnv(E, case["S"], case["K"], seed=1, p_done=0.3)
    cls = DeviceOnPolicyReplayBuffer if buffer == "device" else OnPolicyReplayBuffer
    buf = cls(max_replay_buffer_size=E * T, env_nums=E, time_limit_filter=True)
    coll = VecOnPolicyCollector(vf if learner == "a2c" else networks.ZeroNet(), env=env, eval_env=eval_env, pf=pf, replay_buffer=buf,
                                device=device, epoch_frames=E * T)
    assert coll.fast_path == (buffer == "device") and coll.continuous is False
    args = dict(plr=LR, tau=0.95, shuffle=True, entropy_coeff=cc.ENTROPY_COEFF, env=None, replay_buffer=buf, collector=coll,
                logger=rsm._Log(), device=device, discount=0.99, num_epochs=num_epochs, batch_size=B, save_interval=1, eval_interval=1,
                save_dir=save_dir)
    agent = A2C(pf=pf, vf=vf, vlr=LR, **args) if learner == "a2c" else Reinforce(pf=pf, **args)
    return agent, pf, env, eval_env


@pytest.mark.parametrize("learner", LEARNERS)
def test_train_loop_buffers(learner, device, tmp_path, monkeypatch):
    """train() over a discrete vec env (action_space.n = 16, E = 4), T = 16, B = 32, two epochs, f16, with the resident buffer
    (the rollout step files [E][1] action rows) and with the host buffer (the reference's protocol, [E] actions per step): the
    update infos agree to tests/test_gpu_wide_actions.py::test_train_loop_buffers_and_resume's tolerance; the env only ever
    sees int64 actions in [0, K) (it asserts so per step), the same ones on both paths; eval_one_epoch runs; the saved
    model_pf_*.pth loads with strict=True into a plain torch.nn.Sequential whose softmax is the engine's probabilities within
    the f16 forward cap (par.REF_DIST)."""
    monkeypatch.setenv("V4L_COMPUTE", "f16")
    E, T, B = 4, 16, 32
    U = E * T // B
    runs = {}
    for buffer in ("device", "host"):
        np.random.seed(3); torch.manual_seed(3); torch.cuda.manual_seed(3)
        agent, pf, env, eval_env = _loop_agent(learner, device, buffer, str(tmp_path / buffer), E, T, B, 2)
        np.random.seed(3); torch.manual_seed(3); torch.cuda.manual_seed(3)
        agent.train()
        runs[buffer] = (agent, pf, env, eval_env)
        assert len(agent.logger.updates) == 2 * U and len(agent.logger.epochs) == 2 and agent.f16_saturated == 0
        assert len(env.log) == 2 * T and len(eval_env.log) > 0 and env.closed
        assert agent.trainer.adam_steps() == ((2 * U, 2 * U) if learner == "a2c" else (2 * U, 0))
    a, h = runs["device"][0], runs["host"][0]
    buf = h.replay_buffer
    assert tuple(buf._acts.shape) == (T, E) and tuple(a.replay_buffer._acts_dev.shape) == (T * E, 1)
    assert (buf._acts == np.round(buf._acts)).all() and a.replay_buffer._acts_dev.min().item() >= 0
    tol, keys, worst = 1e-2, _info_keys(learner), 0.0
    for u, (x, y) in enumerate(zip(a.logger.updates, h.logger.updates)):
        assert list(x) == list(y) == keys and np.isfinite(list(x.values())).all()
        for k in keys:
            worst = max(worst, abs(x[k] - y[k]) / max(1.0, abs(y[k])))
    print("\n[cat train loop %s] resident vs host buffer: worst info deviation %.2e (bound %.0e)" % (learner, worst, tol))
    util.record("cat/train_loop/%s/worst_info_resident_vs_host" % learner, worst)
    assert worst <= tol, worst
    assert all((x == y).all() for x, y in zip(runs["device"][2].log, runs["host"][2].log))
    # the checkpoint: networks.Net's keys, loadable by a plain Sequential of the same tree
    pf = runs["device"][1]
    sd = torch.load(os.path.join(str(tmp_path / "device"), "model_pf_finish.pth"), map_location="cpu")
    case = LOOP_CASE
    L, R = torch.nn.Linear, torch.nn.ReLU
    (h1, h2), (a1,) = case["enc"], case["head"]
    plain = torch.nn.Sequential(collections.OrderedDict(
        base=torch.nn.Sequential(collections.OrderedDict(seq_fcs=torch.nn.Sequential(L(case["S"], h1), R(), L(h1, h2), R()))),
        seq_append_fcs=torch.nn.Sequential(L(h2, a1), R(), L(a1, case["K"]))))
    plain.load_state_dict(sd, strict=True)
    obs = torch.tensor(util.obs_rows(np.random.RandomState(4), 33, case), dtype=torch.float32)
    with torch.no_grad():
        want = torch.softmax(plain(obs), dim=-1)
    with torch.cuda.device(device):
        got = pf(obs.to(device)).cpu()
    err = util.rel_err(got, want)
    print("   engine probabilities vs the loaded Sequential's softmax: rel err %.2e" % err)
    assert err < par.REF_DIST["f16"], err
