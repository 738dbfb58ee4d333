"""CPU: the C ABI of the captured V-MPO update (library version 111) against the header and the ctypes mirror. No GPU: nothing
here launches a kernel."""
import ctypes
import inspect
import os
import re

import util

NAMES = ["v4l_trainer_vmpo_update_next", "v4l_trainer_vmpo_update_run", "v4l_trainer_vmpo_graph_counts"]


def test_abi_header_exports_and_mirror():
    from vision4leg_amd import _lib
    hdr = open(os.path.join(util.ROOT, "include", "v4l_hip.h")).read()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, hdr) and n in _lib.exported_symbols() and hasattr(dll, n), n
    l = _lib.lib()
    assert l.v4l_version() >= 111
    assert l.v4l_abi_sizeof(4) == ctypes.sizeof(_lib.VMPOHyper) == 40  # v4l_vmpo_hyper did not move
    assert l.v4l_abi_sizeof(1) == ctypes.sizeof(_lib.PPOHyper) == 48   # nor v4l_ppo_hyper
    # the arguments the header declares, counted: (tr, ro, n, hp, vstats_all_dev, [count,] use_graph, stream) / (tr, captures, replays)
    for n, argc in zip(NAMES, (7, 8, 3)):
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % n, hdr).group(1)
        assert len(decl.split(",")) == argc == len(_lib._SIGS[n][1]), n


def test_engine_signatures():
    from vision4leg_amd.engine import HipTrainer
    run = inspect.signature(HipTrainer.vmpo_update_run).parameters
    assert list(run) == ["self", "ro", "n", "count", "vstats_all", "graph"] and run["graph"].default is True
    nxt = inspect.signature(HipTrainer.vmpo_update_next).parameters
    assert list(nxt) == ["self", "ro", "n", "vstats_all", "graph"]
    assert nxt["vstats_all"].default is None and nxt["graph"].default is False  # existing callers stay eager
    assert callable(HipTrainer.vmpo_graph_counts)
