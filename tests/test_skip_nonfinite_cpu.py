"""Opt-in skipping of non-finite optimiser steps (PPO(skip_nonfinite_steps=True)): the C ABI surface and the host's rule for
the statistics records, without a GPU. The device side is tests/test_gpu_skip_nonfinite.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import util


def _ppo_mod():
    from vision4leg_amd.torchrl.algo.on_policy import ppo
    return ppo


def test_guard_entry_points_declared_exported_and_bound():
    from vision4leg_amd import _lib
    hdr = open(os.path.join(util.ROOT, "include", "v4l_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("v4l_trainer_begin_guarded", "v4l_trainer_steps"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.exported_symbols(), name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), name
    l = _lib.lib()
    assert l.v4l_version() >= 107
    assert len(l.v4l_trainer_begin_guarded.argtypes) == 10 and len(l.v4l_trainer_steps.argtypes) == 4
    # the record layout is unchanged: the flags travel in a buffer of their own
    assert _lib.V4L_STATS == 24


def test_ppo_takes_the_switch_as_a_keyword():
    import inspect
    sig = inspect.signature(_ppo_mod().PPO.__init__)
    assert sig.parameters["skip_nonfinite_steps"].default is False


def _records(U, nonfinite_rows=()):
    st = np.ones((U, 24), dtype=np.float32)
    st[:, 22] = 0
    for u in nonfinite_rows:
        st[u, :18] = np.nan
        st[u, 22] = 18
    return st


def test_guard_off_raises_exactly_as_before():
    check = _ppo_mod()._check_update_records
    assert check(_records(4), None, False) == (0, 0)
    with pytest.raises(FloatingPointError, match=r"non-finite training statistics in minibatch update 2 of epoch 7"):
        check(_records(4, [2, 3]), None, False, lambda u: "minibatch update %d of epoch %d" % (u, 7))
    # guard off: flags (if any were passed) change nothing
    with pytest.raises(FloatingPointError, match="non-finite"):
        check(_records(4, [2]), np.array([[0, 0], [0, 0], [1, 1], [0, 0]], np.int32), False)


def test_guarded_nonfinite_without_a_skip_still_raises():
    check = _ppo_mod()._check_update_records
    flags = np.zeros((4, 2), np.int32)
    with pytest.raises(FloatingPointError, match="minibatch update 1"):
        check(_records(4, [1]), flags, True)
    # a skip in another update does not cover this one
    flags[3] = (1, 1)
    with pytest.raises(FloatingPointError, match="minibatch update 1"):
        check(_records(4, [1, 3]), flags, True)


def test_guarded_nonfinite_with_a_skip_is_counted_not_raised():
    check = _ppo_mod()._check_update_records
    flags = np.array([[0, 0], [0, 0], [1, 1], [0, 0]], np.int32)
    assert check(_records(4, [2]), flags, True) == (1, 1)
    # actor-only and critic-only skips (slot 0 = pf, slot 1 = vf)
    flags = np.array([[1, 0], [0, 1], [1, 0], [0, 0]], np.int32)
    assert check(_records(4, [0, 1, 2]), flags, True) == (2, 1)
    # a skip with finite statistics (cannot come from the kernels, but the count is the flags')
    assert check(_records(2), np.array([[0, 1], [0, 0]], np.int32), True) == (0, 1)
    assert check(_records(3), np.zeros((3, 2), np.int32), True) == (0, 0)
