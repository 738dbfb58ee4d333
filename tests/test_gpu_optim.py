"""-m gpu: weight decay on the HIP engine — PPO(optimizer_class=torch.optim.AdamW / Adam(weight_decay=...)), DESIGN.md 1.

- clip_adam_kernel<WD_COUPLED / WD_DECOUPLED> in isolation: tests/test_gpu_loss_adam.py::test_clip_adam_200_steps_vs_float64 with
  decay (its net, gradients, regimes and learning rates; tests/optim_cases.py holds the float64 restatement, the gate and the
  decay settings, chosen so that — tests/test_optim_cpu.py asserts it — at every compared step the run with decay is >= 50 gates
  away from the run without on >= 90 % of every tensor), a zero-gradient step
  that shows a shared encoder tensor decayed by both optimisers, guarded steps, AdamW(weight_decay=0) == Adam.
- whole PPO.update calls against the unmodified reference's fixtures (tests/golden/make_golden_optim.py) and the oracle stepping
  with the restatement, under tests/test_gpu_parity.py::test_ppo_update's rules; eager and as the epoch's hipGraph.
- train / checkpoint / resume with optimizer_class="AdamW", the exchange with a real torch.optim.AdamW, the refusals."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

import optim_cases as oc
import test_gpu_loss_adam as la
import test_gpu_parity as par
import test_gpu_resume as rsm
import util
from oracle import ppo_oracle as orc

pytestmark = pytest.mark.gpu

MODES = par.MODES
EPS = oc.EPS


def _trainer(case, mode, device, n, wd, decoupled, world=2):
    """la._trainer with decay. world_size 2: every step sums its gradient buffer again (grad_sumsq_kernel, the data-parallel
    phases' norm), as the decay-free test does."""
    from vision4leg_amd.engine import HipTrainer
    pf, vf = par._build(case, mode, device)
    with torch.no_grad():
        pf.state_dict(keep_vars=True)[oc.ISO_ZERO].view(-1)[:7].zero_()
    for net in (pf, vf):
        net.mark_params_changed()
    tpf = copy.deepcopy(pf).to(device)
    tr = HipTrainer(pf.hip, vf.hip, tpf.hip, n, la.CLIP, la.ENT, world_size=world, weight_decay=wd, decoupled=decoupled)
    tr.sync_target()
    return pf, vf, tr


def _iso_setup(mode, device, wd, decoupled):
    assert oc.ISO_CASE == la._dense(7)
    n = 4
    pf, vf, tr = _trainer(oc.ISO_CASE, mode, device, n, wd, decoupled)
    ro, rows, _ = la._inputs(pf, vf, oc.ISO_CASE, n, device, seed=9, tanh=False)
    tp, tv = oc.f64_params(pf, vf)
    P, V = oc.iso_mirrors(pf.hip, vf.hip, tp, tv, wd, decoupled)
    return pf, vf, tr, ro, n, P, V


def _step(tr, ro, n, stats, gp, gv, lr_pf, lr_vf, flags=None):
    """One update through the eager phases with the gradients replaced by gp / gv (fp32 numpy)."""
    tr.begin(None, stats, lr_pf, lr_vf, skip_all=flags)
    tr.critic_grads(ro, n)
    tr.g_vf.copy_(torch.from_numpy(gv))
    tr.critic_step()
    tr.actor_grads(ro, n)
    tr.g_pf.copy_(torch.from_numpy(gp))
    tr.actor_step()
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mode_wd,wd", oc.SETTINGS)
def test_clip_adam_decay_steps_vs_float64(mode_wd, wd, mode, device):
    """optim_cases.ISO_STEPS optimiser steps of both nets with weight decay on the decay-free test's synthetic gradients (norms far
    above, near and far below max_grad_norm, elements of 1e-20 and 1e18, learning rates changed every 7 steps): parameters, both
    moments and the logged pre-clip norms (which hold no decay term) against optim_cases.FlatWD. Seven elements have a zero
    gradient and start at zero: their m and v stay zero and they stay zero."""
    decoupled = mode_wd == "decoupled"
    pf, vf, tr, ro, n, P, V = _iso_setup(mode, device, wd, decoupled)
    rs = np.random.RandomState(oc.ISO_SEED)
    stats = torch.zeros(1, 24, device=device)
    o = pf.hip.grad_offsets[pf.hip.param_names.index(oc.ISO_ZERO)]
    worst = {"params": 0.0, "norm": 0.0}
    for k in range(oc.ISO_STEPS):
        lr_pf, lr_vf = oc.iso_lrs(k)
        gp, gv = oc.iso_grads(rs, k, pf.hip.total_params, vf.hip.total_params, o)
        _step(tr, ro, n, stats, gp, gv, lr_pf, lr_vf)
        nv = V.step(torch.from_numpy(gv), lr_vf)
        npf = P.step(torch.from_numpy(gp), lr_pf)
        rec = tr.stats_cur().double().cpu().numpy()
        for got, want in ((rec[5], nv), (rec[17], npf)):
            r = abs(got - want) / (64 * EPS * want)
            worst["norm"] = max(worst["norm"], float(r))
            assert r <= 1.0, (k, got, want)
        if oc.iso_compared(k):
            worst["params"] = max(worst["params"], la._cmp(mode, "vf", V, vf.state_dict(keep_vars=True), tr.m_vf, tr.v_vf, k),
                                  la._cmp(mode, "pf", P, pf.state_dict(keep_vars=True), tr.m_pf, tr.v_pf, k))
    assert tr.adam_steps() == (oc.ISO_STEPS, oc.ISO_STEPS)
    assert torch.all(tr.v_pf[o:o + 7] == 0) and torch.all(tr.m_pf[o:o + 7] == 0)
    assert torch.all(pf.state_dict()[oc.ISO_ZERO].view(-1)[:7] == 0)
    print("\n[%s wd=%g %s] worst error / gate: %s" % (mode_wd, wd, mode, worst))
    for key, v in worst.items():
        util.record("optim/clip_adam_steps/%s/wd%g/%s/%s_err_over_gate" % (mode_wd, wd, mode, key), v)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mode_wd", oc.MODES_WD)
def test_shared_encoder_tensor_shows_both_optimisers_decay(mode_wd, mode, device):
    """One update with all-zero gradients (norm 0, clip coefficient 1), lr_pf = 2e-3, lr_vf = 1e-3, wd = 0.1: what moves a
    parameter is the decay alone. Decoupled: m = v = 0, the update is 0, so a tensor both nets own ends at fl(fl(p f_vf) f_pf) —
    checked bit for bit — and the others at fl(p f_pf) / fl(p f_vf). Coupled: g' = wd p, the first Adam step is
    lr wd |p| / (wd |p| + eps) towards zero, from the critic and again from the actor: a shared element with wd |p| > 100 eps
    moves by lr_vf + lr_pf to 2 %, an unshared one by its own optimiser's lr."""
    decoupled = mode_wd == "decoupled"
    wd, lr_pf, lr_vf = 0.1, 2e-3, 1e-3
    pf, vf, tr, ro, n, P, V = _iso_setup(mode, device, wd, decoupled)
    before_pf = {k: v.detach().clone() for k, v in pf.state_dict().items()}
    before_vf = {k: v.detach().clone() for k, v in vf.state_dict().items()}
    stats = torch.zeros(1, 24, device=device)
    gp = np.zeros(pf.hip.total_params, dtype=np.float32)
    gv = np.zeros(vf.hip.total_params, dtype=np.float32)
    _step(tr, ro, n, stats, gp, gv, lr_pf, lr_vf)
    V.step(torch.from_numpy(gv), lr_vf)
    P.step(torch.from_numpy(gp), lr_pf)
    la._cmp(mode, "vf", V, vf.state_dict(keep_vars=True), tr.m_vf, tr.v_vf, 0)
    la._cmp(mode, "pf", P, pf.state_dict(keep_vars=True), tr.m_pf, tr.v_pf, 0)
    psd, vsd = pf.state_dict(keep_vars=True), vf.state_dict(keep_vars=True)
    shared = [k for k in psd if k in vsd and psd[k] is vsd[k]]
    assert shared and any(k not in shared for k in psd) and any(k not in shared for k in vsd)
    f = lambda lr: torch.tensor(1.0 - lr * wd, dtype=torch.float64).to(torch.float32).to(device)  # double, rounded once
    for tag, sd, before, lr_own in (("pf", psd, before_pf, lr_pf), ("vf", vsd, before_vf, lr_vf)):
        for k, v in sd.items():
            got, p0 = v.detach(), before[k]
            if decoupled:
                want = (p0 * f(lr_vf)) * f(lr_pf) if k in shared else p0 * f(lr_own)
                assert torch.equal(got, want), (tag, k, (got - want).abs().max().item())
            else:
                big = wd * p0.abs() > 100 * 1e-5
                if not big.any():
                    continue
                moved = (p0 - got)[big] * torch.sign(p0[big])
                want = lr_vf + lr_pf if k in shared else lr_own
                assert ((moved - want).abs() <= 0.02 * want).all(), (tag, k, moved.min().item(), moved.max().item(), want)
    if decoupled:
        assert not tr.m_pf.any() and not tr.v_pf.any() and not tr.m_vf.any() and not tr.v_vf.any()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mode_wd", oc.MODES_WD)
def test_guarded_steps_apply_no_decay(mode_wd, mode, device):
    """tests/test_gpu_loss_adam.py::test_guarded_steps_skip_and_resume_with_right_bias_correction with wd = 0.1: NaN in the
    policy's gradient at step 5, Inf in the critic's at 9, both at 13. A skipped step leaves that optimiser's parameters and
    moments bit for bit — no decay either — and the next taken step matches the float64 reference that skipped the same step."""
    decoupled = mode_wd == "decoupled"
    pf, vf, tr, ro, n, P, V = _iso_setup(mode, device, 0.1, decoupled)
    rs = np.random.RandomState(7)
    stats = torch.zeros(1, 24, device=device)
    flags = torch.zeros(1, 2, dtype=torch.int32, device=device)
    K = 20
    bad = {5: "pf", 9: "vf", 13: "both"}
    for k in range(K):
        gp = la._grads(rs, pf.hip.total_params, ["big", "small"][k % 2], False).astype(np.float32)
        gv = la._grads(rs, vf.hip.total_params, ["near", "big"][k % 2], False).astype(np.float32)
        if bad.get(k) in ("pf", "both"):
            gp[11] = np.nan
        if bad.get(k) in ("vf", "both"):
            gv[3] = np.inf
        before_pf = {name: v.clone() for name, v in pf.state_dict().items()}
        before_vf = {name: v.clone() for name, v in vf.state_dict().items()}
        mom = [b.clone() for b in (tr.m_pf, tr.v_pf, tr.m_vf, tr.v_vf)]
        _step(tr, ro, n, stats, gp, gv, 1e-3, 2e-3, flags)
        f = flags[0].cpu().numpy()
        assert tuple(f) == (int(bad.get(k) in ("pf", "both")), int(bad.get(k) in ("vf", "both"))), (k, f)
        V.step(torch.from_numpy(gv), 2e-3, skip=bool(f[1]))
        P.step(torch.from_numpy(gp), 1e-3, skip=bool(f[0]))
        if f[0]:
            assert torch.equal(tr.m_pf, mom[0]) and torch.equal(tr.v_pf, mom[1])
            for name in pf.hip.param_names:
                if f[1] or name not in vf.hip.param_names:  # (shared tensors move with the critic's step)
                    assert torch.equal(pf.state_dict()[name], before_pf[name]), (k, name)
        if f[1]:
            assert torch.equal(tr.m_vf, mom[2]) and torch.equal(tr.v_vf, mom[3])
            for name in vf.hip.param_names:
                if f[0] or name not in pf.hip.param_names:
                    assert torch.equal(vf.state_dict()[name], before_vf[name]), (k, name)
        assert tr.adam_steps() == (P.opt.steps, V.opt.steps)
        la._cmp(mode, "vf", V, vf.state_dict(keep_vars=True), tr.m_vf, tr.v_vf, k)
        la._cmp(mode, "pf", P, pf.state_dict(keep_vars=True), tr.m_pf, tr.v_pf, k)
    assert tr.adam_steps() == (K - 2, K - 2)


class _Coll:
    epoch_frames = 1


def _ppo(case, mode, device, **kw):
    from vision4leg_amd.torchrl.algo import PPO
    pf, vf = par._build(case, mode, device)
    agent = PPO(pf=pf, vf=vf, plr=oc.GOLDEN_LR, vlr=oc.GOLDEN_LR, clip_para=0.2, opt_epochs=3, tau=0.95, shuffle=True,
                entropy_coeff=0.005, env=None, replay_buffer=None, collector=_Coll(), logger=None, device=device, discount=0.99,
                num_epochs=1500, batch_size=case["B"], save_dir=None, **kw)
    agent.trainer.sync_target()
    return agent


_KEYS = ("obs", "acts", "advs", "estimate_returns", "values")


@pytest.mark.parametrize("mode", MODES)
def test_adamw_without_decay_is_adam_bit_for_bit(mode, device):
    """20 PPO.update calls of mlp_s93: AdamW(weight_decay=0) and Adam(weight_decay=0) leave the same parameters, moments and
    infos as the default, bit for bit (weight_decay == 0 launches the kernel without decay)."""
    case = util.CASES["mlp_s93"]
    runs = []
    for oc_ in (None, functools.partial(torch.optim.AdamW, weight_decay=0), "Adam"):
        agent = _ppo(case, mode, device, optimizer_class=oc_)
        infos = []
        for u in range(20):
            b = util.make_batch(case, update=u)
            infos.append(agent.update({k: b[k] for k in _KEYS}))
        runs.append((rsm._state(agent), infos))
    assert runs[0][0]["m_pf"].abs().sum() > 0
    for state, infos in runs[1:]:
        rsm._assert_same(runs[0][0], state)
        assert infos == runs[0][1]


def _check_against_oracle(name, mode, tag, u, info, oinfo, ginfo, nets, gold):
    """tests/test_gpu_parity.py::test_ppo_update's rules for one update, unchanged: the 18 infos against the same-mode oracle
    (5e-4 f32 / 5e-3), f16's first update within 1e-3 of the reference's own, the ratio-discontinuous four either-or from the
    second 16-bit update on; every parameter within 2e-5 (f32) / 2.2e-4 (u + 1) of the oracle, the mean within 1e-7 / 2e-5 (u + 1);
    f32 also against the reference's fixture."""
    for k in util.STAT_KEYS:
        tol = (5e-4 if mode == "f32" else 5e-3) * max(1.0, abs(oinfo[k]))
        if mode == "f16" and u == 0:
            assert abs(info[k] - ginfo[k]) <= 1e-3 * max(1.0, abs(ginfo[k])), (u, k, info[k], ginfo[k])
        strict_ok = abs(info[k] - oinfo[k]) <= tol
        if mode != "f32" and u >= 1:
            if k in ("grad_norm/pf", "ratio/max", "ratio/min", "Training/policy_loss"):
                assert strict_ok or abs(info[k] - ginfo[k]) <= 5e-2 * max(1.0, abs(ginfo[k])), (u, k, info[k], oinfo[k], ginfo[k])
            else:
                assert strict_ok, (u, k, info[k], oinfo[k], ginfo[k])
            continue
        assert strict_ok, (u, k, info[k], oinfo[k])
        if mode == "f32":
            assert abs(info[k] - ginfo[k]) <= tol, (u, k, info[k], ginfo[k])
    worst, tot, cnt = 0.0, 0.0, 0
    for t, net, onet in nets:
        for k, v in net.state_dict().items():
            dd = (v.detach().cpu() - onet[k]).abs()
            worst = max(worst, dd.max().item())
            tot += dd.sum().item(); cnt += dd.numel()
            assert dd.max().item() <= (2e-5 if mode == "f32" else 2.2e-4 * (u + 1)), (u, t, k, dd.max().item())
            if mode == "f32" and ("u%d/%s/%s" % (u, t, k)) in gold.files:
                assert np.abs(v.detach().cpu().numpy() - gold["u%d/%s/%s" % (u, t, k)]).max() <= 2e-5, (u, t, k)
    util.record("optim/ppo_update/%s/%s/u%d/worst_abs_param_vs_oracle" % (tag, mode, u), worst)
    util.record("optim/ppo_update/%s/%s/u%d/mean_abs_param_vs_oracle" % (tag, mode, u), tot / cnt)
    assert tot / cnt <= (1e-7 if mode == "f32" else 2e-5 * (u + 1)), (u, tot / cnt)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mode_wd", oc.MODES_WD)
@pytest.mark.parametrize("name", oc.GOLDEN_CASES)
def test_ppo_update_with_decay_vs_reference(name, mode_wd, mode, device, monkeypatch):
    """Two PPO.update calls with AdamW / Adam(weight_decay=) (optim_cases.GOLDEN_WD) against what the unmodified reference left
    (tests/golden/ppo_optim_*.npz) and the oracle, whose adam_step is replaced by the pinned restatement for this test. Then the
    same two minibatches as a device-resident epoch, three times: an agent that replays the epoch's hipGraph and one that
    launches everything eagerly end bit-identical."""
    from vision4leg_amd.engine import HipTrainer
    case = util.CASES[name]
    wd, decoupled = oc.GOLDEN_WD[mode_wd], mode_wd == "decoupled"
    cls = functools.partial(torch.optim.AdamW if decoupled else torch.optim.Adam, weight_decay=wd)
    monkeypatch.setattr(orc, "adam_step", oc.oracle_adam_step(wd, decoupled))
    gold = util.load_golden(oc.golden_name(name, mode_wd))
    assert float(gold["weight_decay"]) == wd and bool(gold["decoupled"]) == decoupled and float(gold["lr"]) == oc.GOLDEN_LR
    agent = _ppo(case, mode, device, optimizer_class=cls)
    agent.use_graph = False
    assert agent.optimizer_class is (torch.optim.AdamW if decoupled else torch.optim.Adam)
    g = agent.pf_optimizer.param_groups[0]
    assert g["weight_decay"] == wd and g["decoupled_weight_decay"] == decoupled and agent.trainer.hp.weight_decay == wd
    pf, vf = agent.pf, agent.vf
    opf, ovf = par._oracle_params(pf, vf, case["kind"])
    oracle = orc.PPOOracle(case["kind"], opf, ovf, {k: v.clone() for k, v in opf.items()}, case["S"], mode)
    oracle.sync_target()
    t = lambda a: torch.tensor(a, dtype=torch.float32)
    batches = [util.make_batch(case, update=u) for u in range(2)]
    for u, b in enumerate(batches):
        info = agent.update({k: b[k] for k in _KEYS})
        oinfo = oracle.update(t(b["obs"]), t(b["acts"]), t(b["advs"]), t(b["estimate_returns"]), t(b["values"]),
                              oc.GOLDEN_LR, oc.GOLDEN_LR)
        ginfo = dict(zip(util.STAT_KEYS, gold["u%d/info" % u]))
        _check_against_oracle(name, mode, "%s/%s" % (name, mode_wd), u, info, oinfo, ginfo,
                              (("pf", pf, opf), ("vf", vf, ovf)), gold)
    # ---- the same minibatches through run_updates: the epoch graph against eager launches
    B = case["B"]
    cat = lambda key: np.concatenate([b[key] for b in batches]).astype(np.float32)
    rows = torch.arange(2 * B, dtype=torch.int32, device=device).view(2, B)
    results = []
    for graph in (False, True):
        monkeypatch.setenv("V4L_EPOCH_GRAPH", "1")
        a = _ppo(case, mode, device, optimizer_class=cls)
        a.use_graph = graph
        net = a.pf.hip
        net.ensure_bound()
        state, image = net.alloc_rollout(2 * B, device)
        up = lambda x: torch.tensor(x, dtype=torch.float32, device=device)
        net.ingest(up(cat("obs")), state, image)
        ro = HipTrainer.rollout(state, image, up(cat("acts")).reshape(2 * B, -1), up(cat("advs")).reshape(-1),
                                up(cat("estimate_returns")).reshape(-1), up(cat("values")).reshape(-1))
        recs = []
        for ep in range(3):
            a.pf_optimizer.param_groups[0]["lr"] = oc.GOLDEN_LR * (1 - 0.1 * ep)   # the decoupled factor follows the schedule
            a.vf_optimizer.param_groups[0]["lr"] = oc.GOLDEN_LR * (1 - 0.2 * ep)
            stats = torch.zeros(2, 24, device=device)
            a.run_updates(ro, rows, stats)
            torch.cuda.synchronize()
            recs.append(stats.cpu().numpy())
            if ep == 0 and not graph:  # the eager epoch saw what the two update() calls saw
                for k, v in a.pf.state_dict().items():
                    assert (v.detach().cpu() - pf.state_dict()[k].cpu()).abs().max().item() <= (2e-5 if mode == "f32" else 4.4e-4), k
        assert a.trainer.adam_steps() == (6, 6)
        results.append((np.concatenate(recs), rsm._state(a)))
    (se, ste), (sg, stg) = results
    assert np.isfinite(se[:, :18]).all() and np.array_equal(se, sg), np.abs(se - sg).max()
    rsm._assert_same(ste, stg)


def _resume_agent(case, seed, device, **kw):
    kw.setdefault("optimizer_class", "AdamW")
    kw.setdefault("optimizer_kwargs", {"weight_decay": 0.05})
    return rsm._agent(case, seed, device, **kw)


@pytest.mark.parametrize("mode", MODES)
def test_resume_with_adamw_is_bit_identical(mode, device, tmp_path, monkeypatch):
    """tests/test_gpu_resume.py::test_continuation_is_bit_identical's shape on mlp_s93 with
    PPO(optimizer_class="AdamW", optimizer_kwargs={"weight_decay": 0.05}): two epochs, save_checkpoint, a fresh PPO from another
    seed, load_checkpoint, one more epoch == three epochs in one agent, bit for bit (the decay factor follows the schedule's
    learning rate of the resumed epoch). The same file under another weight_decay, or under plain Adam, raises ValueError naming
    both sides and leaves the trainer alone. The policy optimiser's state_dict loads into a real torch.optim.AdamW, and back."""
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    monkeypatch.setenv("V4L_COMPUTE", mode)
    case = util.CASES["mlp_s93"]
    ckpt = str(tmp_path)
    a = _resume_agent(case, case["seed"], device)
    assert a.optimizer_class is torch.optim.AdamW and a.trainer.hp.decoupled_weight_decay == 1
    np.random.seed(5)
    for epoch in range(3):
        rsm._epoch(a, case, epoch)
    b1 = _resume_agent(case, case["seed"], device)
    np.random.seed(5)
    for epoch in range(2):
        rsm._epoch(b1, case, epoch)
    b1.save_checkpoint(ckpt, 1)
    sd = b1.pf_optimizer.state_dict()
    assert sd["param_groups"][0]["weight_decay"] == 0.05 and sd["param_groups"][0]["decoupled_weight_decay"] is True
    np.random.seed(999)
    b2 = _resume_agent(case, case["seed"] + 100, device)
    b2.load_checkpoint(ckpt, 1)
    assert b2.trainer.adam_steps() == (2 * rsm.U, 2 * rsm.U)
    rsm._epoch(b2, case, 2)
    rsm._assert_same(rsm._state(a), rsm._state(b2))
    assert torch.equal(a.records[2], b2.records[0]) and a.lrs[2:] == b2.lrs
    assert a.logger.updates[2 * rsm.U:] == b2.logger.updates
    # the decay is in it: the same three epochs under plain Adam end elsewhere
    plain = rsm._agent(case, case["seed"], device)
    np.random.seed(5)
    for epoch in range(3):
        rsm._epoch(plain, case, epoch)
    assert not torch.equal(rsm._state(plain)["pf/base.seq_fcs.0.weight"], rsm._state(a)["pf/base.seq_fcs.0.weight"])
    # another setting does not resume
    for kw, what in (({"optimizer_kwargs": {"weight_decay": 0.1}}, r"weight_decay 0\.05 .*weight_decay 0\.1"),
                     ({"optimizer_class": None, "optimizer_kwargs": None}, "weight_decay"),
                     ({"optimizer_class": "Adam"}, "decoupled, AdamW.*coupled L2, Adam")):
        c = _resume_agent(case, case["seed"] + 7, device, **kw)
        before = rsm._state(c)
        with pytest.raises(ValueError, match=what):
            c.load_checkpoint(ckpt, 1)
        for k in ("m_pf", "v_pf", "m_vf", "v_vf"):
            assert torch.equal(before[k], rsm._state(c)[k])
        assert c.trainer.adam_steps() == (0, 0)
    # a real AdamW over the same module takes the state, keeps the decoupled flag, and hands it back
    torch.manual_seed(7)
    cpu_pf, _ = util.build_nets(networks, policies, case)
    opt = torch.optim.AdamW(cpu_pf.parameters(), lr=3e-4, eps=1e-5, weight_decay=0.05)
    opt.load_state_dict(sd)
    assert opt.param_groups[0]["decoupled_weight_decay"] is True and opt.param_groups[0]["weight_decay"] == 0.05
    assert all(float(opt.state[p]["step"]) == 2 * rsm.U for p in cpu_pf.parameters())
    fresh = _resume_agent(case, case["seed"] + 9, device)
    fresh.pf_optimizer.load_state_dict(opt.state_dict())
    assert torch.equal(fresh.trainer.m_pf, b1.trainer.m_pf) and torch.equal(fresh.trainer.v_pf, b1.trainer.v_pf)
    assert fresh.trainer.adam_steps()[0] == 2 * rsm.U


def test_refusals(device):
    """Another optimiser class is still a NotImplementedError; the library itself refuses a negative or non-finite weight_decay
    and names the field."""
    from vision4leg_amd.torchrl.algo import PPO
    case = dict(util.CASES["mlp_s93"], B=16)
    pf, vf = par._build(case, "f16", device)
    for bad in (torch.optim.SGD, functools.partial(torch.optim.RMSprop), "SGD"):
        with pytest.raises(NotImplementedError):
            PPO(pf=pf, vf=vf, collector=_Coll(), device=device, batch_size=16, optimizer_class=bad)
    with pytest.raises(ValueError, match="amsgrad"):
        PPO(pf=pf, vf=vf, collector=_Coll(), device=device, batch_size=16,
            optimizer_class=functools.partial(torch.optim.AdamW, amsgrad=True))
    agent = PPO(pf=pf, vf=vf, collector=_Coll(), device=device, batch_size=16, optimizer_class=torch.optim.AdamW)
    assert agent.optimizer_class is torch.optim.AdamW and agent.pf_optimizer.param_groups[0]["weight_decay"] == 0.01
    tr = agent.trainer
    stats = torch.zeros(1, 24, device=device)
    for value in (-0.01, float("nan"), float("inf")):
        tr.hp.weight_decay = value
        with pytest.raises(RuntimeError, match="weight_decay"):
            tr.begin(None, stats, 1e-4, 1e-4)
    tr.hp.weight_decay = 0.01
    tr.begin(None, stats, 1e-4, 1e-4)
    torch.cuda.synchronize()
