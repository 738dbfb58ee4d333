"""PPO(target_kl=...), the KL early stop, without a GPU: the validity of the shared cases in the CPU oracle,
the C ABI surface, the argument refusals and the host-buffer epoch loop. The device side is tests/test_gpu_kl_stop.py."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import util
import kl_cases as kc

_ORACLE = {}


def _never_stopping(name, mode):
    """The oracle's run of a case without a stop (computed once per (case, mode), shared, never changed)."""
    if (name, mode) not in _ORACLE:
        opf, ovf = kc.cpu_nets(name)
        _ORACLE[name, mode] = kc.oracle_run(name, mode, opf, ovf, kc.data(name), None)
    return _ORACLE[name, mode]


@pytest.mark.parametrize("mode", kc.MODES)
@pytest.mark.parametrize("name", sorted(kc.CASES))
def test_case_is_valid_in_the_oracle(name, mode):
    """The threshold lies a factor 3 above every approx_kl before u*, above the info tolerance taken twice, a factor 3 below
    approx_kl[u*], and 1 <= u* <= U - 2 — in the oracle of each compute mode, before any kernel is asked."""
    run = _never_stopping(name, mode)
    bad, us = kc.validity(name, mode, run)
    print("   %s %s: approx_kl %s, u* = %s" % (name, mode, np.array2string(run["kl"], precision=4), us))
    assert not bad, bad
    assert run["u_star"] is None and run["steps"] == {"pf": kc.CASES[name]["U"], "vf": kc.CASES[name]["U"]}


@pytest.mark.parametrize("name", sorted(kc.CASES))
def test_oracle_with_the_stop(name):
    """The restated semantics: the policy's step of u* is the first one skipped, the critic's of u* + 1; the latch stays."""
    opf, ovf = kc.cpu_nets(name)
    dat = kc.data(name)
    c = kc.CASES[name]
    _, us = kc.validity(name, "f32", _never_stopping(name, "f32"))
    run = kc.oracle_run(name, "f32", opf, ovf, dat, c["target_kl"])
    assert run["u_star"] == us
    assert run["steps"] == {"pf": us, "vf": us + 1}
    assert run["latch"].tolist() == [0] * us + [1] * (c["U"] - us)
    # nothing moves after the stop: the same parameters as the run that ends with update u*
    short = kc.oracle_run(name, "f32", opf, ovf, dat, c["target_kl"], rows=dat[5][:us + 1])
    for k in run["pf"]:
        assert torch.equal(run["pf"][k], short["pf"][k]), k
    for k in run["vf"]:
        assert torch.equal(run["vf"][k], short["vf"][k]), k
    # and up to u* the approx_kl of the run that never stops
    assert np.array_equal(run["kl"][:us + 1], _never_stopping(name, "f32")["kl"][:us + 1])


def test_entry_point_declared_exported_and_bound():
    from vision4leg_amd import _lib
    hdr = open(os.path.join(util.ROOT, "include", "v4l_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("v4l_trainer_kl_stop", "v4l_trainer_kl_update_next", "v4l_trainer_kl_update_run", "v4l_trainer_kl_graph_counts"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.exported_symbols(), name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), name
    l = _lib.lib()
    assert l.v4l_version() >= 116
    assert len(l.v4l_trainer_kl_stop.argtypes) == 4 and len(l.v4l_trainer_kl_update_run.argtypes) == 7
    assert _lib.V4L_STATS == 24  # the record layout is unchanged: the KL columns travel in a buffer of their own
    # the pinned sizes and signatures stay
    assert ctypes.sizeof(_lib.PPOHyper) == l.v4l_abi_sizeof(1) and ctypes.sizeof(_lib.NetCfg) == l.v4l_abi_sizeof(0)
    assert len(l.v4l_trainer_begin_guarded.argtypes) == 10 and len(l.v4l_trainer_update_run.argtypes) == 7


def _nets(name="mlp_s93"):
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    return util.build_nets(networks, policies, kc.geometry(name))


def test_ppo_takes_target_kl_as_a_keyword():
    from vision4leg_amd.torchrl.algo import PPO
    from vision4leg_amd.engine import HipTrainer
    assert inspect.signature(PPO.__init__).parameters["target_kl"].default is None
    sig = inspect.signature(PPO.run_updates).parameters
    assert list(sig)[-2:] == ["skip", "kl"] and sig["kl"].default is None
    assert list(inspect.signature(HipTrainer.kl_arm).parameters) == ["self", "kl_all", "target_kl"]
    assert list(inspect.signature(HipTrainer.begin).parameters)[-1] == "skip_all"  # the disarmed path's calls are as they were


@pytest.mark.parametrize("bad", [0, 0.0, -0.01, float("inf"), float("nan"), "0.01", True, [0.01]])
def test_refused_values(bad):
    """Raised before anything touches a device (the constructor's own GPU check would raise RuntimeError)."""
    from vision4leg_amd.torchrl.algo import PPO
    pf, vf = _nets()
    with pytest.raises(ValueError, match="target_kl"):
        PPO(pf=pf, vf=vf, device="cpu", target_kl=bad)


@pytest.mark.parametrize("good", [None, 0.01, 1, np.float32(0.02)])
def test_accepted_values_reach_the_device_check(good):
    from vision4leg_amd.torchrl.algo import PPO
    pf, vf = _nets()
    with pytest.raises(RuntimeError, match="needs a GPU"):
        PPO(pf=pf, vf=vf, device="cpu", target_kl=good)


def test_refused_data_parallel(monkeypatch):
    from vision4leg_amd.torchrl.algo import PPO
    from vision4leg_amd.torchrl.algo.on_policy import ppo
    pf, vf = _nets()
    monkeypatch.setattr(ppo, "_dist_world", lambda: 2)
    with pytest.raises(NotImplementedError, match="single process"):
        PPO(pf=pf, vf=vf, device="cpu", target_kl=0.01)
    with pytest.raises(RuntimeError, match="needs a GPU"):  # without the option data parallel is what it was
        PPO(pf=pf, vf=vf, device="cpu")
    monkeypatch.setattr(ppo, "_dist_world", lambda: 1)
    monkeypatch.setenv("V4L_FORCE_DP_PHASES", "1")
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    with pytest.raises(NotImplementedError, match="single process"):
        PPO(pf=pf, vf=vf, device="cpu", target_kl=0.01)


@pytest.mark.parametrize("learner", ["VMPO", "A2C", "Reinforce"])
def test_the_other_learners_refuse_it(learner):
    import vision4leg_amd.torchrl.algo as algo
    pf, vf = _nets()
    cls = getattr(algo, learner)
    kw = dict(pf=pf, plr=1e-4) if learner == "Reinforce" else dict(pf=pf, vf=vf)
    with pytest.raises(NotImplementedError, match=learner + " does not take target_kl"):
        cls(device="cpu", target_kl=0.01, **kw)


class _Buffer:
    def __init__(self, batches):
        self.batches = batches

    def one_iteration(self, batch_size, keys, shuffle):
        return iter(range(self.batches))


class _Logger:
    def __init__(self):
        self.infos = []

    def add_update_info(self, info):
        self.infos.append(info)


class _Sched:
    param_groups = [{"lr": 1e-4}]


def _stub_agent(stop_at, opt_epochs=3, batches=4):
    """A PPO whose constructor never ran: the attributes update_per_epoch's host-buffer loop reads, and an update() that reports
    kl_stop = 1 at call number stop_at (None: never)."""
    from vision4leg_amd.torchrl.algo import PPO

    class Trainer:
        def sync_target(self):
            pass

    agent = PPO.__new__(PPO)
    agent.device = torch.device("cpu")
    agent.replay_buffer, agent.logger, agent.trainer = _Buffer(batches), _Logger(), Trainer()
    agent.opt_epochs, agent.batch_size, agent.sample_key, agent.shuffle = opt_epochs, 32, [], False
    agent.pf_optimizer, agent.vf_optimizer = _Sched(), _Sched()
    agent.current_epoch, agent.num_epochs, agent.plr, agent.vlr = 5, 100, 1e-4, 1e-4
    agent.target_kl, agent.last_kl_stop, agent.kl_stops = 0.01, None, 0
    agent.process_epoch_samples = lambda: None
    calls = []

    def update(batch):
        calls.append(batch)
        return {"approx_kl": 0.1 * len(calls), "kl_stop": int(stop_at is not None and len(calls) - 1 >= stop_at)}

    agent.update = update
    return agent, calls


def test_host_buffer_epoch_ends_both_loops_after_a_stop(monkeypatch):
    import contextlib
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    agent, calls = _stub_agent(stop_at=5)  # update 1 of the second pass
    agent.update_per_epoch()
    assert len(calls) == 6 and len(agent.logger.infos) == 6
    assert [i["kl_stop"] for i in agent.logger.infos] == [0, 0, 0, 0, 0, 1]
    assert agent.last_kl_stop == (5, 5) and agent.kl_stops == 1
    # without a stop: every minibatch of every pass, as before
    agent, calls = _stub_agent(stop_at=None)
    agent.update_per_epoch()
    assert len(calls) == 12 and agent.last_kl_stop is None and agent.kl_stops == 0
    # an info dict without the key (the option off) never ends the loops
    agent, calls = _stub_agent(stop_at=None)
    agent.update = lambda batch: calls.append(batch) or {"Training/vf_loss": 0.0}
    agent.update_per_epoch()
    assert len(calls) == 12


def test_info_dict_keys():
    from vision4leg_amd.torchrl.algo import PPO
    from vision4leg_amd import _lib
    agent = PPO.__new__(PPO)
    row = np.arange(24, dtype=np.float32)
    assert list(agent._info(row, None)) == _lib.STAT_KEYS  # the option off: the 18 keys, as before
    info = agent._info(row, None, np.array([0.25, 1.0], np.float32))
    assert list(info) == _lib.STAT_KEYS + ["approx_kl", "kl_stop"] and info["approx_kl"] == 0.25 and info["kl_stop"] == 1
    info = agent._info(row, np.array([1, 0]), np.array([np.nan, 0.0], np.float32))
    assert list(info) == _lib.STAT_KEYS + ["skipped/pf", "skipped/vf", "approx_kl", "kl_stop"] and info["kl_stop"] == 0
