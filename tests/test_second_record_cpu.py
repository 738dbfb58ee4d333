"""CPU: the shell VMPO and A2C share (vision4leg_amd/torchrl/algo/on_policy/second_record.py): that they do share it, what each
declares, the one-allocation buffers of a run, what both refuse, and the engine's A2C signatures. No GPU: nothing here launches a
kernel."""
import inspect

import pytest
import torch

import util
import a2c_cases as ac
import vmpo_cases as vc

CLASSES = ["VMPO", "A2C"]


def _cls(name):
    import vision4leg_amd.torchrl.algo as algo
    return getattr(algo, name)


def test_the_shell_is_shared():
    from vision4leg_amd.torchrl.algo import A2C, PPO, VMPO
    for m in ("_run", "_buffers", "update", "update_per_epoch", "_update_epoch_resident", "train_state", "save_checkpoint",
              "load_checkpoint", "run_updates", "_refuse"):
        assert getattr(VMPO, m) is getattr(A2C, m), m
        assert getattr(VMPO, m) is not getattr(PPO, m, None), m
    for cls in (VMPO, A2C):
        assert issubclass(cls, PPO) and cls.train is PPO.train and cls.snapshot is PPO.snapshot
        assert cls._epoch_rowidx is PPO._epoch_rowidx and cls._upload_batch is PPO._upload_batch
    assert VMPO._info is not A2C._info


def test_hook_table():
    from vision4leg_amd import _lib
    from vision4leg_amd.engine import HipTrainer
    from vision4leg_amd.torchrl.algo import A2C, VMPO
    assert (VMPO._second_stats, A2C._second_stats) == (_lib.V4L_VMPO_STATS, _lib.V4L_A2C_STATS) == (12, 16)
    assert VMPO._rollout_keys == ("acts", "advs", "estimate_returns", "values")
    assert A2C._rollout_keys == ("acts", "advs", "estimate_returns")
    v = object.__new__(VMPO)
    v.opt_epochs = 7
    a = object.__new__(A2C)  # (A2C instances have no opt_epochs)
    assert (v._passes, a._passes) == (7, 1)
    assert (VMPO._syncs_target, A2C._syncs_target) == (True, False)
    assert (VMPO._run_entry, VMPO._next_entry) == ("vmpo_update_run", "vmpo_update_next")
    assert (A2C._run_entry, A2C._next_entry) == ("a2c_update_run", "a2c_update_next")
    for name in (VMPO._run_entry, VMPO._next_entry, A2C._run_entry, A2C._next_entry):
        assert callable(getattr(HipTrainer, name))
    row, second = [float(j) for j in range(_lib.V4L_STATS)], [100.0 + j for j in range(16)]
    info = v._info(row, second[:12])
    assert list(info) == _lib.VMPO_INFO_KEYS and len(info) == 19
    assert info["Training/eta"] == 102.0 and info[_lib.STAT_KEYS[0]] == 0.0  # both rows are read
    info = a._info(row, second)
    assert list(info) == _lib.A2C_INFO_KEYS and list(info.values()) == second[:12]  # the second row alone


@pytest.mark.parametrize("name", CLASSES)
def test_buffers_on_the_cpu(name):
    from vision4leg_amd import _lib
    agent = object.__new__(_cls(name))
    agent.device = torch.device("cpu")
    width = agent._second_stats
    rowidx = torch.arange(15, dtype=torch.int32).reshape(3, 5)
    rows, both, first, second = agent._buffers(rowidx, 3)
    assert both.dtype == torch.float32 and both.numel() == 3 * (_lib.V4L_STATS + width) and not both.any()
    assert first.data_ptr() == both.data_ptr() and tuple(first.shape) == (3, _lib.V4L_STATS)
    assert second.data_ptr() == both.data_ptr() + 3 * _lib.V4L_STATS * 4 and tuple(second.shape) == (3, width)
    assert rows.data_ptr() != rowidx.data_ptr() and torch.equal(rows, rowidx)
    ptrs = (rows.data_ptr(), first.data_ptr(), second.data_ptr())
    rows2, both2, first2, second2 = agent._buffers(rowidx + 100, 3)
    assert (rows2.data_ptr(), first2.data_ptr(), second2.data_ptr()) == ptrs and both2 is both
    assert torch.equal(rows2, rowidx + 100)
    rows3, both3, first3, second3 = agent._buffers(None, 1)
    assert rows3 is None and both3 is not both and both3.numel() == _lib.V4L_STATS + width
    assert tuple(first3.shape) == (1, _lib.V4L_STATS) and tuple(second3.shape) == (1, width)
    assert second3.data_ptr() == both3.data_ptr() + _lib.V4L_STATS * 4


def _nets(name):
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    if name == "A2C":
        return ac.seeded_nets(networks, policies, ac.A2C_CASES["a2c_mlp_odd"])
    return util.build_nets(networks, policies, vc.VMPO_CASES["vmpo_mlp_odd"])


class _HeadStub:
    logstd_head = True


@pytest.mark.parametrize("name", CLASSES)
@pytest.mark.parametrize("kw", [dict(skip_nonfinite_steps=True), dict(save_train_state=True), dict(resume="x"), "logstd_head"])
def test_refusals_name_the_class(name, kw):
    """Raised before anything touches a device: with nothing to refuse the same call reaches the PPO shell's device check."""
    cls = _cls(name)
    pf, vf = _nets(name)
    with pytest.raises(RuntimeError, match="needs a GPU"):
        cls(pf=pf, vf=vf, device="cpu")
    if kw == "logstd_head":
        pf, kw = _HeadStub(), {}
    with pytest.raises(NotImplementedError, match=r"\b%s\b" % name):
        cls(pf=pf, vf=vf, device="cpu", **kw)


@pytest.mark.parametrize("name", CLASSES)
def test_no_train_state(name):
    agent = object.__new__(_cls(name))
    for call in (agent.train_state, lambda: agent.save_checkpoint("x", 0), lambda: agent.load_checkpoint("x", 0),
                 lambda: agent.run_updates(None, None, None)):
        with pytest.raises(NotImplementedError, match=r"\b%s\b" % name):
            call()


def test_engine_signatures():
    from vision4leg_amd.engine import HipTrainer
    assert str(inspect.signature(HipTrainer.a2c_update_next)) == "(self, ro, n, astats_all, graph=False)"
    assert str(inspect.signature(HipTrainer.a2c_update_run)) == "(self, ro, n, count, astats_all, graph=True)"
    assert str(inspect.signature(HipTrainer.vmpo_update_next)) == "(self, ro, n, vstats_all=None, graph=False)"
    assert str(inspect.signature(HipTrainer.vmpo_update_run)) == "(self, ro, n, count, vstats_all, graph=True)"
    assert str(inspect.signature(HipTrainer.update_next)) == "(self, ro, n, graph=True)"
    assert str(inspect.signature(HipTrainer.update_run)) == "(self, ro, n, count, graph=True)"
