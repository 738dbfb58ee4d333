"""CPU: V-MPO (tests/vmpo_cases.py). The restatement against the fixtures the unmodified reference produced
(tests/golden/make_golden_vmpo.py), the seed rule of every case, the C ABI's V-MPO entries against the header and the ctypes
mirror, what `algo.VMPO` refuses, and the overlay's opt-in. No GPU: nothing here launches a kernel."""
import ctypes
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import util
import vmpo_cases as vc

REF = "/root/reference"
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "torchrl")), reason="reference tree not present")


@pytest.mark.parametrize("name", vc.FIXTURE_CASES)
def test_restatement_matches_reference_fixture(name):
    """VMPOOracle in fp32 against two VMPO.update calls of the reference: 19 infos to 1e-5 relative, eta / alpha and every
    small parameter to 1e-6, every parameter's checksum."""
    from vision4leg_amd.torchrl.algo import VMPO  # noqa: F401  (the feature under test exists)
    case = vc.VMPO_CASES[name]
    gold = util.load_golden(name)
    oracle = vc.fresh_oracle(case)
    for u in range(2):
        info = oracle.update(*vc.batch_tensors(case, u), vc.LR, vc.LR)
        assert list(info) == vc.INFO_KEYS
        for k, want in zip(vc.INFO_KEYS, gold["u%d/info" % u]):
            assert abs(info[k] - want) <= 1e-5 * max(1.0, abs(want)), (u, k, info[k], want)
        assert abs(oracle.eta.item() - float(gold["u%d/eta" % u])) <= 1e-6
        assert abs(oracle.alpha.item() - float(gold["u%d/alpha" % u])) <= 1e-6
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


@pytest.mark.parametrize("name", list(vc.VMPO_CASES))
def test_seed_rule(name):
    """tests/wide_cases.py "Seeds" for V-MPO: after the updates the GPU test runs, the fp32 restatement and the float64 one agree
    to ORACLE_F32_ERR_MAX on every parameter and on eta and alpha; and no update's selection sits on a tie."""
    from vision4leg_amd.torchrl.algo import VMPO  # noqa: F401
    case = vc.VMPO_CASES[name]
    o32, o64 = vc.fresh_oracle(case), vc.fresh_oracle(case, dtype=torch.float64)
    for u in range(vc.updates_of(case)):
        gap = vc.tie_gap(util.make_batch(case, update=u)["advs"])
        assert gap > vc.TIE_GAP_MIN, (u, gap)
        o32.update(*vc.batch_tensors(case, u), vc.LR, vc.LR)
        o64.update(*vc.batch_tensors(case, u, torch.float64), vc.LR, vc.LR)
        # the two precisions kept the same rows
        a32, a64 = vc.batch_tensors(case, u)[2], vc.batch_tensors(case, u, torch.float64)[2]
        n32 = (a32 - a32.mean()) / (a32.std() + 1e-5)
        n64 = (a64 - a64.mean()) / (a64.std() + 1e-5)
        assert torch.equal(o32.select(n32), o64.select(n64))
    worst = max((o32.pf[k].double() - o64.pf[k]).abs().max().item() for k in o32.pf)
    worst = max(worst, max((o32.vf[k].double() - o64.vf[k]).abs().max().item() for k in o32.vf))
    scal = max(abs(o32.eta.item() - o64.eta.item()), abs(o32.alpha.item() - o64.alpha.item()))
    print("\n[%s] fp32 vs float64 restatement: worst parameter %.2e, eta / alpha %.2e" % (name, worst, scal))
    assert worst <= vc.ORACLE_F32_ERR_MAX and scal <= vc.ORACLE_F32_ERR_MAX, (worst, scal)


def test_abi_header_exports_and_mirror():
    from vision4leg_amd import _lib
    hdr = open(os.path.join(util.ROOT, "include", "v4l_hip.h")).read()
    names = ["v4l_trainer_vmpo_bytes", "v4l_trainer_vmpo_init", "v4l_trainer_vmpo_actor_grads", "v4l_trainer_vmpo_state",
             "v4l_trainer_vmpo_set_state", "v4l_vmpo_select"]
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, hdr) and n in _lib.exported_symbols() and hasattr(dll, n), n
    l = _lib.lib()
    assert l.v4l_version() >= 110
    assert l.v4l_abi_sizeof(4) == ctypes.sizeof(_lib.VMPOHyper) == 40
    assert l.v4l_abi_sizeof(3) == -1 and l.v4l_abi_sizeof(1) == 48  # the PPO structs did not move
    assert int(re.search(r"#define V4L_VMPO_STATS (\d+)", hdr).group(1)) == _lib.V4L_VMPO_STATS
    assert int(re.search(r"#define V4L_VMPO_STATE (\d+)", hdr).group(1)) == _lib.V4L_VMPO_STATE
    assert int(re.search(r"#define V4L_STATS (\d+)", hdr).group(1)) == _lib.V4L_STATS == 24 and len(_lib.STAT_KEYS) == 18
    assert _lib.VMPO_INFO_KEYS == vc.INFO_KEYS and len(_lib.VMPO_STAT_KEYS) == 7 <= _lib.V4L_VMPO_STATS


def _nets():
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    case = vc.VMPO_CASES["vmpo_mlp_odd"]
    torch.manual_seed(case["seed"])
    return util.build_nets(networks, policies, case)


@pytest.mark.parametrize("kw", [dict(skip_nonfinite_steps=True), dict(save_train_state=True), dict(resume="/nonexistent")])
def test_refused_options(kw):
    """Raised before anything touches a device (the constructor's own GPU check would raise RuntimeError)."""
    from vision4leg_amd.torchrl.algo import VMPO
    pf, vf = _nets()
    with pytest.raises(NotImplementedError):
        VMPO(pf=pf, vf=vf, device="cpu", **kw)
    with pytest.raises(RuntimeError, match="needs a GPU"):  # nothing refused: the PPO shell's device check is reached
        VMPO(pf=pf, vf=vf, device="cpu")


def test_refused_data_parallel(monkeypatch):
    from vision4leg_amd.torchrl.algo import VMPO
    from vision4leg_amd.torchrl.algo.on_policy import ppo
    pf, vf = _nets()
    monkeypatch.setattr(ppo, "_dist_world", lambda: 2)
    with pytest.raises(NotImplementedError, match="single process"):
        VMPO(pf=pf, vf=vf, device="cpu")
    monkeypatch.setattr(ppo, "_dist_world", lambda: 1)
    monkeypatch.setenv("V4L_FORCE_DP_PHASES", "1")
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    with pytest.raises(NotImplementedError, match="single process"):
        VMPO(pf=pf, vf=vf, device="cpu")


def test_signature_is_the_references():
    import inspect
    from vision4leg_amd.torchrl.algo import PPO, VMPO
    p = inspect.signature(VMPO.__init__).parameters
    assert [p[k].default for k in ("opt_epochs", "eta_eps", "alpha_eps", "clipped_value_loss")] == [10, 0.02, 0.1, False]
    assert issubclass(VMPO, PPO) and VMPO.train is PPO.train and VMPO.snapshot is PPO.snapshot
    assert VMPO.process_epoch_samples is PPO.process_epoch_samples


def _run(code):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([util.ROOT, os.path.join(util.ROOT, "tests")]), PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    return r.stdout


@needs_reference
def test_overlay_opt_in():
    """install() leaves torchrl.algo.VMPO the reference's; install(vmpo=True) rebinds it on the package and on the module that
    defines it; uninstall() puts the reference's back."""
    out = _run("""
        import ref_stubs
        ref_stubs.install()
        import vision4leg_amd.overlay as overlay
        import vision4leg_amd.torchrl.algo as hip_algo
        overlay.install()
        import torchrl.algo, torchrl.algo.on_policy.v_mpo as ref_mod
        ref_cls = torchrl.algo.VMPO
        assert ref_cls.__module__.startswith("torchrl.algo") and ref_cls is not hip_algo.VMPO
        overlay.uninstall()
        report = overlay.install(vmpo=True)
        assert "algo.VMPO" in report
        from torchrl.algo import PPO, VMPO
        assert VMPO is hip_algo.VMPO and PPO is hip_algo.PPO and ref_mod.VMPO is hip_algo.VMPO
        overlay.uninstall()
        assert torchrl.algo.VMPO is ref_cls and ref_mod.VMPO is ref_cls
        print("OK")
    """)
    assert out.startswith("OK")
