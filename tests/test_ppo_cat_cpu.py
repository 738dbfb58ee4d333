"""CPU: algo.PPODiscrete (the clipped-surrogate PPO update on policies.CategoricalDisPolicy; tests/ppo_cat_cases.py). The
restatement against the fixture the unmodified reference's PPO produced (tests/golden/make_golden_ppo_cat.py), the seed rule and
the conditions of every case — from the float64 restatement alone —, the library's version and unchanged sizes, the learner's
refusals (each raised before the constructor's GPU check), its returned keys, and the overlay's binding. No GPU: nothing here
launches a kernel."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import util
import cat_cases as cc
import ppo_cat_cases as pc
from ppo_cat_cases import PPO_CAT_CASES

from test_a2c_cpu import needs_reference  # (skips where the reference tree is not present)
from test_cat_cpu import _check_fixture, _run

NAMES = list(PPO_CAT_CASES)


def test_restatement_matches_reference_fixture():
    """CatPPOOracle in fp32 against two update calls of the reference's PPO (no target sync in between) with a subclass of the
    reference's CategoricalDisPolicy that adds the one key ppo.py:53 misses: infos to 1e-5 relative, every small parameter to
    1e-6, every parameter's checksum."""
    from vision4leg_amd.torchrl.algo import PPODiscrete  # noqa: F401  (the feature under test exists)
    case = PPO_CAT_CASES[pc.FIXTURE_CASE]
    gold = util.load_golden(pc.FIXTURE)
    assert int(gold["seed"]) == case["seed"] and case["shared"] and pc.updates_of(case) == 2
    assert not [k for k in gold.files if "log_std" in k] and len(gold["u0/info"]) == len(pc.INFO_KEYS) == 14
    o = pc.fresh_oracle(case)
    assert all(o.vf[k] is o.pf[k] for k in o.vf if k.startswith("base."))  # vf.base = pf.base
    for u in range(2):
        info = o.update(*pc.batch_tensors(case, u), pc.lr_of(case), pc.lr_of(case))
        assert list(info) == pc.INFO_KEYS
        assert _check_fixture(gold, u, info, pc.INFO_KEYS, (("pf", o.pf), ("vf", o.vf))) >= 4


@pytest.mark.parametrize("name", NAMES)
def test_seed_rule(name):
    """tests/wide_cases.py "Seeds": after the updates the GPU test runs, the fp32 restatement and the float64 one agree to
    ORACLE_F32_ERR_MAX on every parameter."""
    from vision4leg_amd.torchrl.algo import PPODiscrete  # noqa: F401
    case = PPO_CAT_CASES[name]
    assert pc.SEED_LOG[name][0] == case["seed"]
    o32, o64 = pc.fresh_oracle(case), pc.fresh_oracle(case, dtype=torch.float64)
    pc.run_updates(o32, case)
    pc.run_updates(o64, case, torch.float64)
    worst = max(max((a[k].double() - b[k]).abs().max().item() for k in a) for a, b in ((o32.pf, o64.pf), (o32.vf, o64.vf)))
    print("\n[%s] fp32 vs float64 restatement after %d updates: worst parameter %.2e" % (name, pc.updates_of(case), worst))
    assert worst <= pc.ORACLE_F32_ERR_MAX, worst


@pytest.mark.parametrize("name", NAMES)
def test_case_conditions(name):
    """Conditions, not measurements, from the float64 restatement alone. tests/test_cat_cpu.py::test_case_conditions' statements
    on the probabilities of every batch (the largest in P_MAX_RANGE, the smallest in P_MIN_RANGE — K = 2: cat_cases' exemption —,
    the reference's clamp inactive, every action index present where B >= K, not the uniform head); and on the clip: in at least
    one update after the first the share of zero-slope rows lies in ZERO_SLOPE_RANGE (B >= 23) and, in that same update, no
    ratio lies within RATIO_GAP of 1 +- clip."""
    from vision4leg_amd.torchrl.algo import PPODiscrete  # noqa: F401
    case = PPO_CAT_CASES[name]
    K, B = case["K"], case["B"]
    o = pc.fresh_oracle(case, dtype=torch.float64)
    for u in range(pc.updates_of(case)):
        obs, acts, _, _, vals = pc.batch_tensors(case, u, torch.float64)
        p, _, ent = cc.head(o.fwd(o.pf, obs, o.S, o.mode))
        pmax, pmin = p.max().item(), p.min().item()
        print("\n[%s] batch %d: largest p %.4f, smallest p %.3e, mean entropy %.4f (log K %.4f)" % (name, u, pmax, pmin, ent.mean().item(), np.log(K)))
        assert pc.P_MAX_RANGE[0] <= pmax <= pc.P_MAX_RANGE[1], pmax
        assert pc.P_MIN_RANGE[0] <= pmin <= (pc.P_MIN_RANGE[1] if K > 2 else 1.0 - pc.P_MAX_RANGE[0]), pmin
        assert pmin > 10 * torch.finfo(torch.float32).eps  # the reference's clamp to [eps, 1 - eps] is inactive
        assert acts.dtype == torch.int64 and tuple(acts.shape) == (B,) and 0 <= int(acts.min()) and int(acts.max()) < K
        assert tuple(vals.shape) == (B, 1)
        if B >= K:
            assert set(acts.tolist()) == set(range(K))
        assert ent.mean().item() < 0.9 * np.log(K)
    pc.run_updates(o, case, torch.float64)
    for u, s in enumerate(o.seen):
        print("[%s] update %d: zero-slope share %.3f, smallest |ratio - (1 +- clip)| %.4f" % (name, u, s["zero_slope"], s["ratio_gap"]))
    if B >= 23:
        assert any(pc.ZERO_SLOPE_RANGE[0] <= s["zero_slope"] <= pc.ZERO_SLOPE_RANGE[1] and s["ratio_gap"] >= pc.RATIO_GAP
                   for s in o.seen[1:]), o.seen


def test_library_version_and_unchanged_abi():
    """Version 118 with its history line; no new C-ABI entry, struct or size; the header says which updates take a flagged net."""
    from vision4leg_amd import _lib
    l = _lib.lib()
    assert l.v4l_version() >= 118
    assert l.v4l_abi_sizeof(0) == ctypes.sizeof(_lib.NetCfg) == 104 and l.v4l_abi_sizeof(1) == ctypes.sizeof(_lib.PPOHyper) == 48
    assert l.v4l_abi_sizeof(2) == ctypes.sizeof(_lib.Rollout) == 56 and l.v4l_abi_sizeof(4) == ctypes.sizeof(_lib.VMPOHyper) == 40
    assert l.v4l_abi_sizeof(3) == -1 and l.v4l_abi_sizeof(5) == -1 and _lib.V4L_STATS == 24
    assert not [s for s in _lib.exported_symbols() if "discrete" in s.lower() or "ppo_cat" in s.lower()]
    src = open(os.path.join(util.ROOT, "vision4leg_amd", "csrc", "v4l_hip.hip")).read()
    assert re.search(r"^// 118: .*actor_loss_cat_kernel", src, re.M)
    hdr = open(os.path.join(util.ROOT, "include", "v4l_hip.h")).read()
    assert "(version 118)" in hdr and "actor_loss_cat_kernel" in hdr
    assert [k for k in _lib.STAT_KEYS if not k.startswith("log_std/")] == pc.INFO_KEYS


# ------------------------------------------------------------------------------------------ Python surface
def _nets(name="ppo_cat_k16"):
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    return pc.seeded_nets(networks, policies, PPO_CAT_CASES[name])


def test_class_and_exports():
    import vision4leg_amd.torchrl.algo as algo
    from vision4leg_amd.torchrl.algo.on_policy import ppo_discrete
    assert algo.PPODiscrete is ppo_discrete.PPODiscrete and "PPODiscrete" in algo.__all__
    assert issubclass(algo.PPODiscrete, algo.PPO) and algo.PPODiscrete._takes_categorical is True
    assert algo.PPO._takes_categorical is False and algo.VMPO._takes_categorical is False
    assert ppo_discrete.INFO_KEYS == pc.INFO_KEYS
    p = inspect.signature(algo.PPODiscrete.__init__).parameters
    assert list(p) == ["self", "pf", "vf", "kwargs"]


@pytest.mark.parametrize("name", ["ppo_cat_k16", "ppo_cat_sep"])
def test_valid_policy_reaches_the_gpu_check(name):
    """A CategoricalDisPolicy with a state-MLP critic, with a common base (vf.base = pf.base) and without, passes every refusal and
    reaches the constructor's GPU check; so do the options that carry over from PPO."""
    from vision4leg_amd.torchrl.algo import PPODiscrete
    pf, vf = _nets(name)
    for kw in (dict(), dict(clipped_value_loss=True), dict(optimizer_class="AdamW", optimizer_kwargs={"weight_decay": 0.01})):
        with pytest.raises(RuntimeError, match="needs a GPU"):
            PPODiscrete(pf=pf, vf=vf, device="cpu", **kw)


def test_plain_ppo_and_vmpo_keep_refusing_the_class():
    from vision4leg_amd.torchrl.algo import PPO, VMPO
    pf, vf = _nets()
    for cls in (PPO, VMPO):
        with pytest.raises(NotImplementedError, match=r"%s does not take policies\.CategoricalDisPolicy \(discrete actions\): its loss "
                                                      r"kernels are Gaussian; the policy runs under algo\.A2C and algo\.Reinforce"
                                                      % cls.__name__):
            cls(pf=pf, vf=vf, device="cpu")


def test_refuses_a_policy_that_is_not_categorical():
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    from vision4leg_amd.torchrl.algo import PPODiscrete
    case = PPO_CAT_CASES["ppo_cat_k16"]
    _, vf = _nets()
    net = dict(input_shape=case["S"], base_type=networks.MLPBase, hidden_shapes=[16], append_hidden_shapes=[16])
    for gauss in (policies.GaussianContPolicyBasicBias(output_shape=3, **net), policies.GaussianContPolicy(output_shape=6, **net)):
        with pytest.raises(NotImplementedError, match=r"PPODiscrete takes policies\.CategoricalDisPolicy .* runs under algo\.PPO"):
            PPODiscrete(pf=gauss, vf=vf, device="cpu")


@pytest.mark.parametrize("kw,word", [(dict(target_kl=0.01), "target_kl"), (dict(desired_kl=0.01), "desired_kl"),
                                     (dict(skip_nonfinite_steps=True), "skip_nonfinite_steps"),
                                     (dict(save_train_state=True), "train state"), (dict(resume="/nowhere"), "train state")])
def test_options_refused_before_the_gpu_check(kw, word):
    """Each with its reason, as NotImplementedError (the GPU check would raise RuntimeError)."""
    from vision4leg_amd.torchrl.algo import PPODiscrete
    pf, vf = _nets()
    with pytest.raises(NotImplementedError, match=r"PPODiscrete does not .*%s" % word):
        PPODiscrete(pf=pf, vf=vf, device="cpu", **kw)


def test_data_parallel_is_refused(monkeypatch):
    from vision4leg_amd.torchrl.algo import PPODiscrete
    from vision4leg_amd.torchrl.algo.on_policy import ppo
    pf, vf = _nets()
    monkeypatch.setattr(ppo, "_dist_world", lambda: 2)
    with pytest.raises(NotImplementedError, match="single process"):
        PPODiscrete(pf=pf, vf=vf, device="cpu")


def test_no_train_state():
    from vision4leg_amd.torchrl.algo import PPODiscrete
    agent = PPODiscrete.__new__(PPODiscrete)
    for call in (agent.train_state, lambda: agent.save_checkpoint("x", 0), lambda: agent.load_checkpoint("x", 0)):
        with pytest.raises(NotImplementedError, match="no resumable train state"):
            call()


@pytest.mark.parametrize("bad", [[0, 1, 16], [0, -1, 3], [0.5, 1, 2], [float("nan"), 1, 2]])
def test_out_of_range_acts_raise_before_upload(bad):
    """PPO._upload_batch's check of the host batch's action indices runs first: ValueError with no device in sight (the object is
    a bare instance: nothing of the constructor has run)."""
    from vision4leg_amd.torchrl.algo import PPODiscrete
    pf, _ = _nets()
    agent = PPODiscrete.__new__(PPODiscrete)
    agent.pf = pf
    batch = {"obs": np.zeros((3, 45)), "acts": np.array(bad), "advs": np.zeros((3, 1)), "estimate_returns": np.zeros((3, 1)),
             "values": np.zeros((3, 1))}
    with pytest.raises(ValueError, match=r"integer action indices in \[0, 16\)"):
        agent._upload_batch(batch, ("acts", "advs", "estimate_returns", "values"))


def test_returned_keys_are_the_fourteen():
    """update() and the logger get the reference PPO's keys in its order without the four log_std/*."""
    from vision4leg_amd import _lib
    from vision4leg_amd.torchrl.algo import PPO, PPODiscrete
    row = np.arange(_lib.V4L_STATS, dtype=np.float32)
    info = PPODiscrete.__new__(PPODiscrete)._info(row, None)
    assert list(info) == pc.INFO_KEYS and len(info) == 14
    assert info["logprob/min"] == 10.0 and info["ratio/max"] == 15.0 and info["ratio/min"] == 16.0 and info["grad_norm/pf"] == 17.0
    assert list(PPO.__new__(PPO)._info(row, None)) == _lib.STAT_KEYS  # plain PPO: the 18, unchanged


def test_overlay_signature_is_unchanged():
    import vision4leg_amd.overlay as overlay
    p = inspect.signature(overlay.install).parameters
    assert list(p) == ["fast_path", "reference_package", "vmpo", "a2c", "state_std", "reinforce", "discrete"]
    assert overlay.DISCRETE_NEW == {"algo": ["PPODiscrete"]}


@needs_reference
def test_overlay_binds_the_name():
    """install(discrete=True) puts PPODiscrete on the reference's torchrl.algo — a name the reference does not have: nothing is
    rebound, the report does not list it —, install() without the flag does not, uninstall() takes it off again."""
    out = _run("""
        import ref_stubs
        ref_stubs.install()
        import vision4leg_amd.overlay as overlay
        import vision4leg_amd.torchrl.algo as hip_algo
        base = overlay.install(a2c=True, reinforce=True, state_std=True, vmpo=True)
        import torchrl.algo
        assert not hasattr(torchrl.algo, "PPODiscrete")
        ref_ppo_module = torchrl.algo.PPO.__module__
        overlay.uninstall()
        report = overlay.install(discrete=True)
        assert "algo.PPODiscrete" not in report
        from torchrl.algo import PPODiscrete, PPO
        assert PPODiscrete is hip_algo.PPODiscrete and PPO is hip_algo.PPO and issubclass(PPODiscrete, PPO)
        assert torchrl.policies.CategoricalDisPolicy.categorical_head is True
        overlay.uninstall()
        assert not hasattr(torchrl.algo, "PPODiscrete") and torchrl.algo.PPO.__module__.startswith("torchrl.algo")
        print("OK")
    """)
    assert out.startswith("OK")
