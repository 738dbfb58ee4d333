"""CPU: A2C (tests/a2c_cases.py). The restatement against the fixtures the unmodified reference produced
(tests/golden/make_golden_a2c.py), the seed rule of every case, the C ABI's A2C entries against the header and the ctypes
mirror, what `algo.A2C` refuses, its constructor defaults, and the overlay's opt-in. No GPU: nothing here launches a kernel."""
import ctypes
import inspect
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import util
import a2c_cases as ac

REF = "/root/reference"
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "torchrl")), reason="reference tree not present")


@pytest.mark.parametrize("name", ac.FIXTURE_CASES)
def test_restatement_matches_reference_fixture(name):
    """A2COracle in fp32 against two A2C.update calls of the reference: 12 infos to 1e-5 relative, every small parameter to
    1e-6, every parameter's checksum."""
    from vision4leg_amd.torchrl.algo import A2C  # noqa: F401  (the feature under test exists)
    case = ac.A2C_CASES[name]
    gold = util.load_golden(name)
    assert int(gold["seed"]) == case["seed"]
    oracle = ac.fresh_oracle(case)
    for u in range(2):
        info = oracle.update(*ac.batch_tensors(case, u), ac.LR, ac.LR)
        assert list(info) == ac.INFO_KEYS
        for k, want in zip(ac.INFO_KEYS, gold["u%d/info" % u]):
            assert abs(info[k] - want) <= 1e-5 * max(1.0, abs(want)), (u, k, info[k], want)
        seen = 0
        for tag, onet in (("pf", oracle.pf), ("vf", oracle.vf)):
            for k, v in onet.items():
                s = gold["u%d/sum/%s/%s" % (u, tag, k)]
                d = v.double()
                assert abs(d.sum().item() - s[0]) <= 1e-6 * max(1.0, v.numel()) and abs(d.abs().sum().item() - s[1]) <= 1e-6 * max(1.0, v.numel())
                key = "u%d/%s/%s" % (u, tag, k)
                if key in gold.files:
                    seen += 1
                    assert np.abs(v.numpy() - gold[key]).max() <= 1e-6, (u, tag, k)
        assert seen >= 4


@pytest.mark.parametrize("name", list(ac.A2C_CASES))
def test_seed_rule(name):
    """tests/wide_cases.py "Seeds" for A2C: after the updates the GPU test runs, the fp32 restatement and the float64 one agree
    to ORACLE_F32_ERR_MAX on every parameter."""
    from vision4leg_amd.torchrl.algo import A2C  # noqa: F401
    case = ac.A2C_CASES[name]
    o32, o64 = ac.fresh_oracle(case), ac.fresh_oracle(case, dtype=torch.float64)
    for u in range(ac.updates_of(case)):
        o32.update(*ac.batch_tensors(case, u), ac.LR, ac.LR)
        o64.update(*ac.batch_tensors(case, u, torch.float64), ac.LR, ac.LR)
    worst = max((o32.pf[k].double() - o64.pf[k]).abs().max().item() for k in o32.pf)
    worst = max(worst, max((o32.vf[k].double() - o64.vf[k]).abs().max().item() for k in o32.vf))
    print("\n[%s] fp32 vs float64 restatement: worst parameter %.2e" % (name, worst))
    assert worst <= ac.ORACLE_F32_ERR_MAX, worst


def test_loss_rows_wide_block_oracle():
    """What tests/test_gpu_a2c.py::test_loss_rows[a2c_mlp_odd@513] compares with, alone: the restatement at 513 rows with a log
    sigma beyond either end of the clamp is finite everywhere, and its d(loss)/d(logstd) is exactly 0 at those two columns and
    at no other."""
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    case = util.loss_rows_case(ac.A2C_CASES, "a2c_mlp_odd@513")
    assert case["B"] == 513 and case["A"] == 12 and ac.A2C_CASES["a2c_mlp_odd"]["B"] == 23
    assert util.loss_rows_both_ends("a2c_mlp_odd@513", "f32", False) and not util.loss_rows_both_ends("a2c_mlp_odd", "f32", False)
    pf, vf = ac.seeded_nets(networks, policies, case)
    logstd = util.loss_rows_logstd(case["A"], False, both_ends=True)
    assert logstd[0] < -5.0 and logstd[-1] > 2.0 and (logstd[1:-1] > -5.0).all() and (logstd[1:-1] < 2.0).all()
    util.spread_policy_head(pf, logstd)
    dout, dls, dval, info = ac.oracle_of(pf.state_dict(), vf.state_dict(), case).loss_grads(*ac.batch_tensors(case, 0))
    assert dout.shape == (513, 12) and torch.isfinite(dout).all() and torch.isfinite(dls).all() and torch.isfinite(dval).all()
    assert np.isfinite(list(info.values())).all()
    assert dls[0].item() == 0.0 and dls[-1].item() == 0.0 and (dls[1:-1] != 0).all()


def test_case_nets_share_nothing_and_the_starters_pair_does():
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    for case in ac.A2C_CASES.values():
        pf, vf = ac.seeded_nets(networks, policies, case)
        assert not {id(p) for p in pf.parameters()} & {id(p) for p in vf.parameters()}
        assert pf._net_cfg().kind == vf._net_cfg().kind == 0
    pf, vf = util.build_nets(networks, policies, ac.A2C_CASES["a2c_mlp_odd"])
    assert {id(p) for p in pf.parameters()} & {id(p) for p in vf.parameters()}


def test_abi_header_exports_and_mirror():
    from vision4leg_amd import _lib
    hdr = open(os.path.join(util.ROOT, "include", "v4l_hip.h")).read()
    names = ["v4l_trainer_a2c_critic_grads", "v4l_trainer_a2c_actor_grads", "v4l_trainer_a2c_update_next",
             "v4l_trainer_a2c_update_run", "v4l_trainer_a2c_graph_counts"]
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, hdr) and n in _lib.exported_symbols() and hasattr(dll, n), n
    l = _lib.lib()
    assert l.v4l_version() >= 112
    assert int(re.search(r"#define V4L_A2C_STATS (\d+)", hdr).group(1)) == _lib.V4L_A2C_STATS >= len(_lib.A2C_INFO_KEYS) == 12
    assert _lib.A2C_INFO_KEYS == ac.INFO_KEYS
    # the pinned sizes did not move; A2C added no struct
    assert l.v4l_abi_sizeof(3) == -1 and l.v4l_abi_sizeof(5) == -1
    assert l.v4l_abi_sizeof(1) == ctypes.sizeof(_lib.PPOHyper) == 48 and l.v4l_abi_sizeof(4) == ctypes.sizeof(_lib.VMPOHyper) == 40
    assert l.v4l_abi_sizeof(0) == ctypes.sizeof(_lib.NetCfg)
    assert int(re.search(r"#define V4L_STATS (\d+)", hdr).group(1)) == _lib.V4L_STATS == 24 and len(_lib.STAT_KEYS) == 18


@needs_reference
def test_info_keys_are_the_references_order():
    """The key list against the reference's source text: the order in which a2c.py assigns info[...]."""
    src = open(os.path.join(REF, "torchrl", "algo", "on_policy", "a2c.py")).read()
    assert re.findall(r"info\['([^']+)'\]\s*=", src) == ac.INFO_KEYS


def _nets(name="a2c_mlp_odd"):
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    return ac.seeded_nets(networks, policies, ac.A2C_CASES[name])


@pytest.mark.parametrize("kw", [dict(skip_nonfinite_steps=True), dict(save_train_state=True), dict(resume="/nonexistent")])
def test_refused_options(kw):
    """Raised before anything touches a device (the constructor's own GPU check would raise RuntimeError)."""
    from vision4leg_amd.torchrl.algo import A2C
    pf, vf = _nets()
    with pytest.raises(NotImplementedError):
        A2C(pf=pf, vf=vf, device="cpu", **kw)
    with pytest.raises(RuntimeError, match="needs a GPU"):  # nothing refused: the PPO shell's device check is reached
        A2C(pf=pf, vf=vf, device="cpu")


def test_refused_nets():
    from vision4leg_amd.torchrl.algo import A2C
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    # a common parameter: the starters' own state-MLP pair (vf.base = pf.base)
    pf, vf = util.build_nets(networks, policies, ac.A2C_CASES["a2c_mlp_odd"])
    with pytest.raises(NotImplementedError, match="common parameter"):
        A2C(pf=pf, vf=vf, device="cpu")
    # another net kind
    case = dict(kind="cnn", S=93, A=6, seed=1, B=8, enc=[256, 256], head=[256, 256], visual_dim=256)
    pf, vf = util.build_nets(networks, policies, case)
    with pytest.raises(NotImplementedError, match="raises on a shared encoder"):
        A2C(pf=pf, vf=vf, device="cpu")
    with pytest.raises(NotImplementedError, match="raises on a shared encoder"):
        A2C(pf=torch.nn.Linear(4, 2), vf=torch.nn.Linear(4, 1), device="cpu")


def test_refused_data_parallel(monkeypatch):
    from vision4leg_amd.torchrl.algo import A2C
    from vision4leg_amd.torchrl.algo.on_policy import ppo
    pf, vf = _nets()
    monkeypatch.setattr(ppo, "_dist_world", lambda: 2)
    with pytest.raises(NotImplementedError, match="single process"):
        A2C(pf=pf, vf=vf, device="cpu")
    monkeypatch.setattr(ppo, "_dist_world", lambda: 1)
    monkeypatch.setenv("V4L_FORCE_DP_PHASES", "1")
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    with pytest.raises(NotImplementedError, match="single process"):
        A2C(pf=pf, vf=vf, device="cpu")


def test_signature_is_the_references():
    from vision4leg_amd.torchrl.algo import A2C, PPO
    p = inspect.signature(A2C.__init__).parameters
    assert list(p)[:3] == ["self", "pf", "vf"]
    got = {k: p[k].default for k in ("plr", "vlr", "optimizer_class", "entropy_coeff", "shuffle", "tau", "gae")}
    assert got == dict(plr=3e-4, vlr=3e-4, optimizer_class=torch.optim.Adam, entropy_coeff=0.001, shuffle=True, tau=None, gae=True)
    assert not {"clip_para", "opt_epochs", "clipped_value_loss"} & set(p)
    assert issubclass(A2C, PPO) and A2C.train is PPO.train and A2C.snapshot is PPO.snapshot
    assert A2C.process_epoch_samples is PPO.process_epoch_samples and A2C.snapshot_networks is PPO.snapshot_networks


@needs_reference
def test_signature_defaults_against_the_reference_source():
    out = _run("""
        import inspect, ref_stubs
        ref_stubs.install()
        from torchrl.algo.on_policy.a2c import A2C as Ref
        from torchrl.algo.on_policy.on_rl_algo import OnRLAlgo
        from vision4leg_amd.torchrl.algo import A2C
        mine = inspect.signature(A2C.__init__).parameters
        for cls in (Ref, OnRLAlgo):
            for k, v in inspect.signature(cls.__init__).parameters.items():
                if v.default is not inspect.Parameter.empty:
                    assert mine[k].default == v.default, (k, mine[k].default, v.default)
        print("OK")
    """)
    assert out.startswith("OK")


def _run(code):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([util.ROOT, os.path.join(util.ROOT, "tests")]), PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    return r.stdout


@needs_reference
def test_overlay_opt_in():
    """install() leaves torchrl.algo.A2C the reference's; install(a2c=True) rebinds it (and not VMPO) on the package and on the
    module that defines it; uninstall() puts the reference's back."""
    out = _run("""
        import ref_stubs
        ref_stubs.install()
        import vision4leg_amd.overlay as overlay
        import vision4leg_amd.torchrl.algo as hip_algo
        overlay.install()
        import torchrl.algo, torchrl.algo.on_policy.a2c as ref_mod
        ref_cls, ref_vmpo = torchrl.algo.A2C, torchrl.algo.VMPO
        assert ref_cls.__module__.startswith("torchrl.algo") and ref_cls is not hip_algo.A2C
        overlay.uninstall()
        report = overlay.install(vmpo=True)
        assert "algo.A2C" not in report and torchrl.algo.A2C is ref_cls
        overlay.uninstall()
        report = overlay.install(a2c=True)
        assert "algo.A2C" in report and "algo.VMPO" not in report
        from torchrl.algo import PPO, A2C
        assert A2C is hip_algo.A2C and PPO is hip_algo.PPO and ref_mod.A2C is hip_algo.A2C and torchrl.algo.VMPO is ref_vmpo
        overlay.uninstall()
        assert torchrl.algo.A2C is ref_cls and ref_mod.A2C is ref_cls
        print("OK")
    """)
    assert out.startswith("OK")
