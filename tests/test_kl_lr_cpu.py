"""PPO(desired_kl=...), the KL-adaptive learning rates, without a GPU: the validity of the shared cases in the
CPU oracle, the restatement against the plain oracle, the C ABI surface, the argument refusals and the epoch's schedule. The
device side is tests/test_gpu_kl_lr.py."""
import contextlib
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import util
import kl_cases as kc
import kl_lr_cases as lc
from oracle import ppo_oracle as orc

_ORACLE = {}


def _runs(name, mode):
    """(adaptive, fixed-rate) oracle runs of a case (computed once per (case, mode), shared, never changed)."""
    if (name, mode) not in _ORACLE:
        opf, ovf = lc.cpu_nets(name)
        dat = lc.data(name)
        _ORACLE[name, mode] = (lc.oracle_run(name, mode, opf, ovf, dat, lc.CASES[name]["desired_kl"]),
                               lc.oracle_run(name, mode, opf, ovf, dat, None))
    return _ORACLE[name, mode]


@pytest.mark.parametrize("mode", lc.MODES)
@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_case_is_valid_in_the_oracle(name, mode):
    """Every update's approx_kl keeps 2 x kl_tol from both thresholds in the oracle of each compute mode, before any kernel is
    asked; the rates follow the rule from the decisions; U <= 8."""
    c = lc.CASES[name]
    run, _ = _runs(name, mode)
    print("   %s %s: approx_kl %s d %s" % (name, mode, np.array2string(run["kl"], precision=4), run["d"].tolist()))
    print("   margins (distance, 2 x kl_tol): %s" % [(round(a, 3), round(b, 3)) for a, b in lc.margins(name, mode, run)])
    print("   rates %s" % run["lrs"].tolist())
    assert not lc.validity(name, mode, run), lc.validity(name, mode, run)
    # (the guarded case's NaN advantage costs the policy the step of update 0; the option itself never skips one)
    assert len(run["d"]) == c["U"] <= 8 and run["steps"] == {"pf": c["U"] - (1 if c.get("guard") else 0), "vf": c["U"]}
    assert np.isfinite(run["kl"]).all()
    assert run["lrs"][0].tolist() == [c["plr"], c["vlr"]]
    for u, d in enumerate(run["d"]):
        assert d == lc.decide(run["kl"][u], c["desired_kl"])
        for w in range(2):
            assert run["lrs"][u + 1][w] == lc.next_rate(run["lrs"][u][w], d, c["factor"], c["lr_min"], c["lr_max"])
            assert c["lr_min"] <= run["lrs"][u + 1][w] <= c["lr_max"]


@pytest.mark.parametrize("mode", lc.MODES)
def test_the_cases_cover_the_rule(mode):
    """Over the cases: each of the three decisions; a run with two different decisions whose change of rate shows in a later
    approx_kl (against the fixed-rate run, beyond 2 x kl_tol); a run that reaches a clamp."""
    runs = {name: _runs(name, mode)[0] for name in lc.CASES}
    fixed = {name: _runs(name, mode)[1] for name in lc.CASES}
    assert not lc.coverage(mode, runs, fixed), lc.coverage(mode, runs, fixed)
    # the two clamps by name: the critic's rate on kl_lr_min while the policy's falls; the policy's on kl_lr_max while the critic's grows
    a, b = runs["mlp_all_three"], runs["loco_clamp_max"]
    assert a["d"].tolist() == [1, 0, 0, -1, -1, -1]
    assert a["lrs"][-1][1] == lc.CASES["mlp_all_three"]["lr_min"] and a["lrs"][-1][0] < a["lrs"][-2][0] < a["lrs"][-3][0]
    assert b["d"].tolist() == [1] * 6
    assert (b["lrs"][1:, 0] == lc.CASES["loco_clamp_max"]["lr_max"]).all() and (np.diff(b["lrs"][:, 1]) > 0).all()


@pytest.mark.parametrize("name", lc.PLAIN)
def test_inert_restatement_is_the_plain_oracle(name):
    """With a factor of 1 every decision leaves both rates where they are: parameters and infos equal those of PPOOracle.update
    called with the case's rates, bit for bit (the wrapping itself changes nothing); and the fixed-rate run of the restatement
    (desired_kl None) is that run too."""
    c = lc.CASES[name]
    opf, ovf = lc.cpu_nets(name)
    dat = lc.data(name)
    case, obs, acts, advs, rets, rows = dat
    inert = lc.oracle_run(name, "f32", opf, ovf, dat, c["desired_kl"], factor=1.0)
    assert set(inert["d"].tolist()) != {0}  # decisions are taken; they move nothing
    assert (inert["lrs"] == np.array([c["plr"], c["vlr"]])).all()
    p = {k: v.clone() for k, v in opf.items()}
    v = util.share_encoder(p, {k: x.clone() for k, x in ovf.items()}, case["kind"])
    plain = orc.PPOOracle(case["kind"], p, v, {k: x.clone() for k, x in p.items()}, case["S"], "f32")
    plain.sync_target()
    f = lambda x: torch.tensor(x, dtype=torch.float32)
    infos = [plain.update(f(obs[r]), f(acts[r]), f(advs[r]).view(-1, 1), f(rets[r]).view(-1, 1), f(rets[r]).view(-1, 1),
                          c["plr"], c["vlr"]) for r in rows]
    fixed = _runs(name, "f32")[1]
    for run in (inert, fixed):
        assert run["infos"] == infos
        for k in p:
            assert torch.equal(run["pf"][k], p[k]), k
        for k in v:
            assert torch.equal(run["vf"][k], v[k]), k
    assert np.array_equal(inert["kl"], fixed["kl"])


ENTRIES = {"v4l_trainer_kl_adapt": 7, "v4l_trainer_kl_adapt_update_next": 6, "v4l_trainer_kl_adapt_update_run": 7,
           "v4l_trainer_kl_adapt_graph_counts": 3, "v4l_trainer_lrs": 3}


def test_entry_points_declared_exported_and_bound():
    from vision4leg_amd import _lib
    hdr = open(os.path.join(util.ROOT, "include", "v4l_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    l = _lib.lib()
    for name, nargs in ENTRIES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        assert name in _lib.exported_symbols(), name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), name
        assert len(getattr(l, name).argtypes) == nargs, name
    assert l.v4l_version() >= 117
    assert l.v4l_trainer_kl_adapt.argtypes[1:5] == [ctypes.c_double] * 4  # scalars: no new ABI struct
    assert l.v4l_abi_sizeof(3) == -1 and l.v4l_abi_sizeof(5) == -1
    assert _lib.V4L_STATS == 24  # the record layout is unchanged: the [U][4] columns travel in a buffer of their own
    # the pinned sizes and signatures stay
    assert ctypes.sizeof(_lib.PPOHyper) == l.v4l_abi_sizeof(1) and ctypes.sizeof(_lib.NetCfg) == l.v4l_abi_sizeof(0)
    assert len(l.v4l_trainer_begin_guarded.argtypes) == 10 and len(l.v4l_trainer_update_run.argtypes) == 7
    assert len(l.v4l_trainer_kl_stop.argtypes) == 4 and len(l.v4l_trainer_kl_update_run.argtypes) == 7


def _nets(name="mlp_s93"):
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    return util.build_nets(networks, policies, kc.geometry(name))


def test_keywords_and_defaults():
    from vision4leg_amd.torchrl.algo import PPO
    from vision4leg_amd.engine import HipTrainer
    sig = inspect.signature(PPO.__init__).parameters
    assert sig["desired_kl"].default is None
    assert (sig["kl_lr_factor"].default, sig["kl_lr_min"].default, sig["kl_lr_max"].default) == (1.5, 1e-5, 1e-2)
    assert list(inspect.signature(HipTrainer.kl_adapt_arm).parameters) == ["self", "rec_all", "desired_kl", "factor", "lr_min", "lr_max"]
    for name in ("kl_adapt_update_next", "kl_adapt_update_run", "kl_adapt_graph_counts", "lrs"):
        assert callable(getattr(HipTrainer, name)), name
    assert callable(PPO._run_updates_kl_adapt)
    # the disarmed path's calls are as they were
    assert list(inspect.signature(PPO.run_updates).parameters)[-2:] == ["skip", "kl"]
    assert list(inspect.signature(HipTrainer.begin).parameters)[-1] == "skip_all"


BAD = [dict(desired_kl=v) for v in (0, 0.0, -0.01, float("inf"), float("nan"), "0.01", True, [0.01])]
BAD += [dict(desired_kl=0.01, kl_lr_factor=v) for v in (1, 1.0, 0.5, 0, -2.0, float("inf"), float("nan"), "1.5", True, None)]
BAD += [dict(desired_kl=0.01, kl_lr_min=v) for v in (0, -1e-5, float("nan"), float("inf"), "1e-5", None, 2e-2)]
BAD += [dict(desired_kl=0.01, kl_lr_max=v) for v in (0, -1e-2, float("nan"), float("inf"), "1e-2", None, 1e-6)]


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: ",".join("%s=%r" % i for i in kw.items()))
def test_refused_values(kw):
    """Raised before anything touches a device (the constructor's own GPU check would raise RuntimeError)."""
    from vision4leg_amd.torchrl.algo import PPO
    pf, vf = _nets()
    with pytest.raises(ValueError, match="desired_kl|kl_lr_"):
        PPO(pf=pf, vf=vf, device="cpu", **kw)


GOOD = [dict(), dict(desired_kl=None), dict(desired_kl=0.01), dict(desired_kl=1), dict(desired_kl=np.float32(0.02)),
        dict(desired_kl=0.01, kl_lr_factor=2, kl_lr_min=1e-4, kl_lr_max=1e-4), dict(desired_kl=0.01, kl_lr_factor=np.float64(1.0001))]


@pytest.mark.parametrize("kw", GOOD, ids=lambda kw: ",".join("%s=%r" % i for i in kw.items()) or "none")
def test_accepted_values_reach_the_device_check(kw):
    from vision4leg_amd.torchrl.algo import PPO
    pf, vf = _nets()
    with pytest.raises(RuntimeError, match="needs a GPU"):
        PPO(pf=pf, vf=vf, device="cpu", **kw)


def test_target_kl_and_desired_kl_exclude_each_other():
    from vision4leg_amd.torchrl.algo import PPO
    pf, vf = _nets()
    with pytest.raises(ValueError, match="desired_kl and target_kl"):
        PPO(pf=pf, vf=vf, device="cpu", target_kl=0.01, desired_kl=0.01)
    for kw in (dict(target_kl=0.01), dict(desired_kl=0.01)):  # either alone passes the argument checks
        with pytest.raises(RuntimeError, match="needs a GPU"):
            PPO(pf=pf, vf=vf, device="cpu", **kw)


def test_refused_data_parallel(monkeypatch):
    from vision4leg_amd.torchrl.algo import PPO
    from vision4leg_amd.torchrl.algo.on_policy import ppo
    pf, vf = _nets()
    monkeypatch.setattr(ppo, "_dist_world", lambda: 2)
    with pytest.raises(NotImplementedError, match="single process"):
        PPO(pf=pf, vf=vf, device="cpu", desired_kl=0.01)
    with pytest.raises(RuntimeError, match="needs a GPU"):  # without the option data parallel is what it was
        PPO(pf=pf, vf=vf, device="cpu")
    monkeypatch.setattr(ppo, "_dist_world", lambda: 1)
    monkeypatch.setenv("V4L_FORCE_DP_PHASES", "1")
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    with pytest.raises(NotImplementedError, match="single process"):
        PPO(pf=pf, vf=vf, device="cpu", desired_kl=0.01)


@pytest.mark.parametrize("learner", ["VMPO", "A2C", "Reinforce"])
def test_the_other_learners_refuse_it(learner):
    import vision4leg_amd.torchrl.algo as algo
    pf, vf = _nets()
    cls = getattr(algo, learner)
    kw = dict(pf=pf, plr=1e-4) if learner == "Reinforce" else dict(pf=pf, vf=vf)
    with pytest.raises(NotImplementedError, match=learner + " does not take desired_kl"):
        cls(device="cpu", desired_kl=0.01, **kw)


class _Buffer:
    def one_iteration(self, batch_size, keys, shuffle):
        return iter(range(2))


class _Logger:
    def __init__(self):
        self.infos = []

    def add_update_info(self, info):
        self.infos.append(info)


class _Opt:
    def __init__(self, lr):
        self.param_groups = [{"lr": lr}]


def _stub_agent(desired_kl):
    """A PPO whose constructor never ran: the attributes update_per_epoch's host-buffer loop reads, a trainer that only syncs the
    target, and an update() that records the rates it would open with."""
    from vision4leg_amd.torchrl.algo import PPO

    class Trainer:
        def sync_target(self):
            pass

    agent = PPO.__new__(PPO)
    agent.device = torch.device("cpu")
    agent.replay_buffer, agent.logger, agent.trainer = _Buffer(), _Logger(), Trainer()
    agent.opt_epochs, agent.batch_size, agent.sample_key, agent.shuffle = 2, 32, [], False
    agent.pf_optimizer, agent.vf_optimizer = _Opt(3.7e-4), _Opt(2.9e-5)  # what the device left after the last run
    agent.current_epoch, agent.num_epochs, agent.plr, agent.vlr = 50, 100, 1e-3, 1e-3
    agent.target_kl, agent.last_kl_stop, agent.kl_stops = None, None, 0
    agent.desired_kl = desired_kl
    agent.process_epoch_samples = lambda: None
    seen = []
    agent.update = lambda batch: seen.append((agent.pf_optimizer.param_groups[0]["lr"], agent.vf_optimizer.param_groups[0]["lr"])) or {}
    return agent, seen


def test_update_per_epoch_leaves_the_rates_alone_when_armed(monkeypatch):
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    agent, seen = _stub_agent(0.01)
    agent.update_per_epoch()
    assert seen == [(3.7e-4, 2.9e-5)] * 4
    assert agent.pf_optimizer.param_groups[0]["lr"] == 3.7e-4 and agent.vf_optimizer.param_groups[0]["lr"] == 2.9e-5
    # the option off: the reference's linear schedule, as before (epoch 50 of 100 from 1e-3)
    agent, seen = _stub_agent(None)
    agent.update_per_epoch()
    assert seen == [(5e-4, 5e-4)] * 4
    # and an agent built before the option existed (no attribute) is scheduled too
    agent, seen = _stub_agent(None)
    del agent.desired_kl
    agent.update_per_epoch()
    assert seen == [(5e-4, 5e-4)] * 4


def test_info_dict_keys():
    from vision4leg_amd.torchrl.algo import PPO
    from vision4leg_amd import _lib
    agent = PPO.__new__(PPO)
    agent.lr_changes = {"down": 0, "up": 0}
    row = np.arange(24, dtype=np.float32)
    new = ["approx_kl", "lr_decision", "lr/pf", "lr/vf"]
    assert list(agent._info(row, None)) == _lib.STAT_KEYS and len(_lib.STAT_KEYS) == 18  # the option off: the 18 keys, as before
    info = agent._info(row, None, None, np.array([0.25, -1.0, 2e-4, 1e-5], np.float32))
    assert list(info) == _lib.STAT_KEYS + new
    assert info["approx_kl"] == 0.25 and info["lr_decision"] == -1 and isinstance(info["lr_decision"], int)
    assert info["lr/pf"] == float(np.float32(2e-4)) and info["lr/vf"] == float(np.float32(1e-5))
    info = agent._info(row, np.array([1, 0]), None, np.array([np.nan, 0.0, 2e-4, 1e-5], np.float32))
    assert list(info) == _lib.STAT_KEYS + ["skipped/pf", "skipped/vf"] + new and info["lr_decision"] == 0
    for d in (-1.0, 0.0, 1.0, 1.0):
        agent._note_lr_decision(d)
    assert agent.lr_changes == {"down": 1, "up": 2}
