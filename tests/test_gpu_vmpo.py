"""-m gpu: V-MPO (algo.VMPO, the reference's torchrl/algo/on_policy/v_mpo.py) on the HIP engine: the on-device row selection,
one loss evaluation's gradients, two updates of every case of tests/vmpo_cases.py against the same-mode restatement, the
reference's own fixtures, the resident epoch against update(batch), and PPO next to a V-MPO trainer.

The reference arithmetic is vmpo_cases.VMPOOracle (pinned to the unmodified reference by tests/golden/make_golden_vmpo.py and
tests/test_vmpo_cpu.py). The bounds are tests/test_gpu_tact.py::test_two_updates' (infos 5e-4 / 5e-3 relative to max(1, |x|),
every parameter element 2e-5 / 2.2e-4 (u + 1), the mean 1e-7 / 2e-5 (u + 1); the either-or rule of the 16-bit modes from the
second update on for the scalars a moved rounding decision reaches: here grad_norm/pf and Training/policy_loss) and
tests/test_gpu_parity.py's TOL / REF_DIST. eta and alpha are parameters stepped by Adam at lr = 1e-4: held to the element bound
and to par.TOL."""
import os

import numpy as np
import pytest
import torch

import test_gpu_parity as par
import test_gpu_update_route as route
import util
from vmpo_cases import FIXTURE_CASES, INFO_KEYS, LR, VMPO_CASES, VMPOOracle, batch_tensors, updates_of

pytestmark = pytest.mark.gpu

MODES = par.MODES
NAMES = list(VMPO_CASES)
BATCH_KEYS = ("obs", "acts", "advs", "estimate_returns", "values")
EITHER_OR = ("grad_norm/pf", "Training/policy_loss")


class _Coll:
    epoch_frames = 1


def _agent(case, mode, device, cls=None, **kw):
    from vision4leg_amd.torchrl.algo import VMPO
    pf, vf = par._build(case, mode, device)
    args = dict(plr=LR, vlr=LR, opt_epochs=3, tau=0.95, shuffle=True, entropy_coeff=0.005, env=None, replay_buffer=None,
                collector=_Coll(), logger=None, device=device, discount=0.99, num_epochs=1500, batch_size=case["B"], save_dir=None)
    args.update(kw)
    return (cls or VMPO)(pf=pf, vf=vf, **args), pf, vf


def _oracle(pf, vf, case, mode):
    opf, ovf = par._oracle_params(pf, vf, case["kind"])
    oracle = VMPOOracle(case["kind"], opf, ovf, {k: v.clone() for k, v in opf.items()}, case["S"], mode)
    oracle.sync_target()
    return oracle


# ------------------------------------------------------------------------------------------ selection
def _select_inputs(n):
    rs = np.random.RandomState(100 + n)
    plain = rs.randn(3 * n).astype(np.float32)
    ties = (np.round(rs.randn(3 * n) * 2) / 2).astype(np.float32)  # a handful of distinct values: ties everywhere
    ties[::7] = 0.0
    ties[3::11] = -0.0
    nan = rs.randn(3 * n).astype(np.float32)
    slots = rs.permutation(3 * n)[:n].astype(np.int32)
    return {"plain": plain, "ties": ties, "nan": nan}, slots


@pytest.mark.parametrize("n", [1, 2, 23, 64, 65, 257, 1024])
def test_select(n, device):
    """v4l_vmpo_select == np.argsort(-adv, kind="stable")[:m] mapped through rowidx, with and without rowidx; ties go to the
    earlier row; one NaN: still a permutation of valid slots, the NaN row last or absent."""
    from vision4leg_amd import engine
    m = (n + 1) // 2
    inputs, slots = _select_inputs(n)
    for tag, base in inputs.items():
        for rowidx in (None, slots):
            adv = base.copy()
            rows = np.arange(n, dtype=np.int32) if rowidx is None else rowidx
            nan_slot = None
            if tag == "nan":
                nan_slot = int(rows[n // 3])
                adv[nan_slot] = np.nan
            if tag == "ties" and n >= 2:  # and one at the very top, first and last row: the first row must lead
                adv[rows[0]] = adv[rows[-1]] = np.float32(9.0)
            want = rows[np.argsort(-adv[rows], kind="stable")[:m]]
            got = engine.vmpo_select(torch.tensor(adv, device=device), None if rowidx is None else torch.tensor(rowidx, device=device),
                                     n).cpu().numpy()
            assert got.shape == (m,) and len(set(got.tolist())) == m and set(got.tolist()) <= set(rows.tolist()), (tag, got)
            assert np.array_equal(got, want), (tag, rowidx is not None, got, want)
            if nan_slot is not None:
                assert nan_slot not in got[:-1].tolist() and (nan_slot != got[-1] or m == n)
            if tag == "ties" and n >= 2:
                assert len(np.unique(adv[rows])) < n and got[0] == rows[0] and (m < 2 or n == 2 or got[1] == rows[-1])


# ------------------------------------------------------------------------------------------ one loss evaluation
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["vmpo_mlp_odd", "vmpo_mlp_tanh"])
def test_loss_rows(name, mode, device):
    """vmpo_loss_kernel through the trainer with eta / alpha frozen (v4l_vmpo_hyper.lr_scale = 0) and the critic at vlr = 0 (its
    Adam step then moves nothing, so the policy's pass sees the parameters the restatement is given): d(loss)/d(mean) rows,
    d(loss)/d(logstd), d(eta), d(alpha) against autograd on the restatement. The policy is moved away from its target first
    (distinct log sigmas, one beyond the clamp: its gradient is gated to 0; means O(1)), so the KL terms are not zero.
    f32: par.TOL; 16-bit modes: the gradient rows are linear in the head output, whose distance to the fp32 value is capped by
    par.REF_DIST."""
    from vision4leg_amd import _lib
    case = VMPO_CASES[name]
    A, B = case["A"], case["B"]
    m = (B + 1) // 2
    tanh = case["kind"].endswith("_tanh")
    agent, pf, vf = _agent(case, mode, device, vlr=0.0)
    tr = agent.trainer
    tr.sync_target()
    target = {k: v.detach().cpu().clone() for k, v in pf.state_dict().items()}
    logstd = np.linspace(-1.0, 0.0 if tanh else 0.5, A).astype(np.float32)
    if not tanh:
        logstd[-1] = 2.5  # beyond LOG_SIG_MAX: sigma = e^2, no gradient
    util.spread_policy_head(pf, logstd)
    tr.vmpo_init(0.02, 0.1, lr_scale=0.0)
    opf, ovf = par._oracle_params(pf, vf, case["kind"])
    oracle = VMPOOracle(case["kind"], opf, ovf, target, case["S"], mode)
    obs, acts, advs, _, _ = batch_tensors(case, 0)
    dout, dls, deta, dalpha, idx = oracle.loss_grads(obs, acts, advs)
    b = util.make_batch(case, update=0)
    agent.update({k: b[k] for k in BATCH_KEYS})
    torch.cuda.synchronize()
    assert np.array_equal(tr.vmpo_selected(B).cpu().numpy(), idx.numpy())
    hip = pf.hip
    off = _lib.lib().v4l_net_ws_offset(hip.h, m, b"dout")
    gscale = _lib.lib().v4l_net_grad_scale(hip.h, m)
    rows = tr.ws[off:off + m * 16].view(m, 16).cpu() / gscale
    assert (rows[:, A:] == 0).all()
    tol = par.TOL["f32"] if mode == "f32" else par.REF_DIST[mode]
    e_rows = util.rel_err(rows[:, :A], dout)
    e_ls = util.rel_err(hip.grad_view(tr.g_pf, "logstd").cpu().reshape(-1), dls.reshape(-1))
    rec = tr.vmpo_record().cpu().numpy()
    print("\n[%s %s] rel err d(mean) rows %.2e, d(logstd) %.2e; d(eta) % .6f / % .6f, d(alpha) % .6f / % .6f"
          % (name, mode, e_rows, e_ls, rec[7], deta, rec[8], dalpha))
    assert e_rows < tol and e_ls < tol, (e_rows, e_ls)
    if not tanh:
        assert hip.grad_view(tr.g_pf, "logstd").cpu().reshape(-1)[-1].item() == 0.0 and dls.reshape(-1)[-1].item() == 0.0
    assert abs(rec[7] - deta) <= par.TOL[mode] * max(1.0, abs(deta)) and abs(rec[8] - dalpha) <= par.TOL[mode] * max(1.0, abs(dalpha))
    state = tr.vmpo_state()
    assert state[0] == 1.0 and state[1] == float(np.float32(0.1)) and state[2:] == [0.0] * 5  # frozen
    assert agent.f16_saturated == 0


# ------------------------------------------------------------------------------------------ updates
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_two_updates(name, mode, device):
    """19 infos, eta, alpha and every parameter of pf and vf after each VMPO.update call against the same-mode restatement."""
    case = VMPO_CASES[name]
    agent, pf, vf = _agent(case, mode, device)
    oracle = _oracle(pf, vf, case, mode)
    ref32 = _oracle(pf, vf, case, "f32") if mode != "f32" else None
    agent.trainer.sync_target()
    assert agent.param_optimizer.param_groups[0]["lr"] == LR and agent.eta.item() == 1.0
    for u in range(updates_of(case)):
        b = util.make_batch(case, update=u)
        before = {k: v.detach().cpu().clone() for k, v in pf.state_dict().items()}
        info = agent.update({k: b[k] for k in BATCH_KEYS})
        args = batch_tensors(case, u) + (LR, LR)
        oinfo = oracle.update(*args)
        ginfo = ref32.update(*args) if ref32 is not None else None
        assert list(info) == INFO_KEYS
        print("\n[%s %s] update %d info (hip / restatement):" % (name, mode, u))
        for k in INFO_KEYS:
            print("   %-22s % .6f % .6f" % (k, info[k], oinfo[k]))
        for k in INFO_KEYS:
            tol = (5e-4 if mode == "f32" else 5e-3) * max(1.0, abs(oinfo[k]))
            strict_ok = abs(info[k] - oinfo[k]) <= tol
            if mode != "f32" and u >= 1 and k in EITHER_OR:
                assert strict_ok or abs(info[k] - ginfo[k]) <= 5e-2 * max(1.0, abs(ginfo[k])), (u, k, info[k], oinfo[k], ginfo[k])
                continue
            assert strict_ok, (u, k, info[k], oinfo[k])
        elem = 2e-5 if mode == "f32" else 2.2e-4 * (u + 1)
        for tag, got, want in (("eta", agent.eta.item(), oracle.eta.item()), ("alpha", agent.alpha.item(), oracle.alpha.item())):
            assert abs(got - want) <= min(elem, par.TOL[mode] * max(1.0, abs(want))), (u, tag, got, want)
            assert info["Training/" + tag] == got
        worst, tot, cnt = 0.0, 0.0, 0
        for tag, net, onet in (("pf", pf, oracle.pf), ("vf", vf, oracle.vf)):
            for k, v in net.state_dict().items():
                dd = (v.detach().cpu() - onet[k]).abs()
                worst = max(worst, dd.max().item())
                tot += dd.sum().item(); cnt += dd.numel()
                assert dd.max().item() <= elem, (u, tag, k, dd.max().item())
        util.record("vmpo/update/%s/%s/u%d/worst_abs_param_vs_oracle" % (name, mode, u), worst)
        util.record("vmpo/update/%s/%s/u%d/max_info_rel_vs_oracle" % (name, mode, u),
                    max(abs(info[k] - oinfo[k]) / max(1.0, abs(oinfo[k])) for k in INFO_KEYS))
        assert tot / cnt <= (1e-7 if mode == "f32" else 2e-5 * (u + 1))
        assert max((pf.state_dict()[k].cpu() - before[k]).abs().max().item() for k in before) > 5e-5  # the optimiser stepped
        assert (pf.state_dict()["logstd"].cpu() - before["logstd"]).abs().min().item() > 0
    assert agent.trainer.vmpo_state()[6] == updates_of(case) and agent.trainer.adam_steps() == (updates_of(case),) * 2
    assert agent.f16_saturated == 0


@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_against_reference_fixture(name, device):
    """f32 mode against what the unmodified reference logged and stepped to (tests/golden/<name>.npz)."""
    case = VMPO_CASES[name]
    gold = util.load_golden(name)
    agent, pf, vf = _agent(case, "f32", device)
    agent.trainer.sync_target()
    for u in range(2):
        b = util.make_batch(case, update=u)
        info = agent.update({k: b[k] for k in BATCH_KEYS})
        for k, want in zip(INFO_KEYS, gold["u%d/info" % u]):
            assert abs(info[k] - want) <= 5e-4 * max(1.0, abs(want)), (u, k, info[k], want)
        assert abs(agent.eta.item() - float(gold["u%d/eta" % u])) <= 2e-5 and abs(agent.alpha.item() - float(gold["u%d/alpha" % u])) <= 2e-5
        seen = 0
        for tag, net in (("pf", pf), ("vf", vf)):
            for k, v in net.state_dict().items():
                key = "u%d/%s/%s" % (u, tag, k)
                if key in gold.files:
                    seen += 1
                    assert np.abs(v.detach().cpu().numpy() - gold[key]).max() <= 2e-5, (u, tag, k)
        assert seen >= 4


# ------------------------------------------------------------------------------------------ resident epoch
class _Log:
    def __init__(self):
        self.updates = []

    def add_update_info(self, info):
        self.updates.append(dict(info))

    def add_epoch_info(self, *a):
        pass


def test_resident_epoch(device):
    """update_per_epoch on a DeviceOnPolicyReplayBuffer (E = 4, T = 16, batch 32, opt_epochs = 2: four updates, records read
    back once) against a twin that gets the same minibatches one by one through update(batch): the same bits."""
    from vision4leg_amd import recipes
    from vision4leg_amd.torchrl.algo import VMPO
    from vision4leg_amd.torchrl.collector import VecOnPolicyCollector
    from vision4leg_amd.torchrl.replay_buffers import DeviceOnPolicyReplayBuffer
    mode = "f16"
    case = dict(VMPO_CASES["vmpo_mlp"], B=32)
    E, T, B, S = 4, 16, 32, case["S"]
    pf, vf = par._build(case, mode, device)
    buf = DeviceOnPolicyReplayBuffer(max_replay_buffer_size=E * T, env_nums=E, time_limit_filter=True)
    coll = VecOnPolicyCollector(vf, env=recipes.ZeroCostVecEnv(E, case, seed=2, p_done=0.1), eval_env=recipes.ZeroCostVecEnv(E, case, seed=3),
                                pf=pf, replay_buffer=buf, device=device, epoch_frames=E * T)
    log = _Log()
    agent = VMPO(pf=pf, vf=vf, plr=LR, vlr=LR, opt_epochs=2, tau=0.95, shuffle=True, entropy_coeff=0.005, env=None,
                 replay_buffer=buf, collector=coll, logger=log, device=device, discount=0.99, num_epochs=10, batch_size=B)
    twin, tpf, tvf = _agent(case, mode, device, opt_epochs=2)
    for k, v in pf.state_dict().items():
        assert torch.equal(v, tpf.state_dict()[k])
    np.random.seed(3); torch.manual_seed(3); torch.cuda.manual_seed(3)
    coll.train_one_epoch()
    picked, inner = [], buf.one_iteration

    def one_iteration(*a, **kw):
        for batch in inner(*a, **kw):
            picked.append(np.array(batch["rowidx"], copy=True))
            yield batch
    buf.one_iteration = one_iteration
    agent.update_per_epoch()
    torch.cuda.synchronize()
    assert len(picked) == 4 and len(log.updates) == 4 and all(list(i) == INFO_KEYS for i in log.updates)
    assert agent.training_update_num == 4 and agent.trainer.vmpo_state()[6] == 4
    state, _, acts, advs, rets, vals, _ = buf.device_rollout()
    twin.trainer.sync_target()
    for u, rows in enumerate(picked):
        idx = torch.tensor(rows, dtype=torch.long, device=device)
        host = lambda t: t[idx].detach().cpu().numpy()
        info = twin.update({"obs": host(state)[:, :S], "acts": host(acts), "advs": host(advs).reshape(-1, 1),
                            "estimate_returns": host(rets).reshape(-1, 1), "values": host(vals).reshape(-1, 1)})
        assert info == log.updates[u], (u, info, log.updates[u])
    for a, b in ((pf, tpf), (vf, tvf)):
        for k, v in a.state_dict().items():
            assert torch.equal(v, b.state_dict()[k]), k
    assert agent.trainer.vmpo_state() == twin.trainer.vmpo_state()
    assert np.isfinite([v for i in log.updates for v in i.values()]).all()


# ------------------------------------------------------------------------------------------ PPO beside it
def test_ppo_untouched(device):
    """After a V-MPO trainer has run in the process, PPO launches what tests/test_gpu_update_route.py pins (mlp_s93's pass, the
    whole PPO update of loco_s84) and an mlp_s93 PPO update gives the bits it gave before."""
    from vision4leg_amd.torchrl.algo import PPO
    mode = "f16"
    case = util.CASES["mlp_s93"]

    def ppo_update():
        agent, pf, vf = _agent(case, mode, device, cls=PPO, clip_para=0.2)
        agent.trainer.sync_target()
        b = util.make_batch(case, update=0)
        info = agent.update({k: b[k] for k in BATCH_KEYS})
        return info, {tag + k: v.detach().cpu().clone() for tag, net in (("pf/", pf), ("vf/", vf)) for k, v in net.state_dict().items()}
    info0, params0 = ppo_update()
    vcase = VMPO_CASES["vmpo_mlp"]
    vagent, _, _ = _agent(vcase, mode, device)
    vagent.trainer.sync_target()
    b = util.make_batch(vcase, update=0)
    vagent.update({k: b[k] for k in BATCH_KEYS})
    info1, params1 = ppo_update()
    assert info0 == info1 and sorted(info1) == sorted(util.STAT_KEYS)
    for k in params0:
        assert torch.equal(params0[k], params1[k]), k
    rows = route.collect("mlp_s93", mode, {}, device)
    assert rows == route.TABLES[route.ROUTES[route._key("mlp_s93", mode, {})]]
    rows = route.collect_update("loco_s84", mode, {}, device)
    assert rows == route.TABLES[route.ROUTES[route._key("loco_s84", mode, {}, what="update")]]
    del vagent
