"""CPU: the discrete policy (policies.CategoricalDisPolicy under algo.A2C and algo.Reinforce; tests/cat_cases.py). The restatements
against the fixtures the unmodified reference produced (tests/golden/make_golden_cat.py), the conditions and the seed rule of every
case, the C ABI's new entries against the header and the ctypes mirror with every pinned size, what v4l_net_set_categorical
refuses, the Python surface (state_dict keys, refusals, the host batch's action check, the overlay's opt-in) and the inverse CDF
the GPU sampling test compares with. No GPU: nothing here launches a kernel.

One refusal of the setter needs a device — a net can only be bound on one: tests/test_gpu_cat.py::test_setter_refuses_a_bound_net."""
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
import cat_cases as cc
from cat_cases import CAT_CASES

from test_a2c_cpu import needs_reference  # (skips where the reference tree is not present)
NAMES = list(CAT_CASES)


def _check_fixture(gold, u, info, keys, nets):
    for k, want in zip(keys, gold["u%d/info" % u]):
        assert abs(info[k] - want) <= 1e-5 * max(1.0, abs(want)), (u, k, info[k], want)
    seen = 0
    for tag, onet in nets:
        for k, v in onet.items():
            s = gold["u%d/sum/%s/%s" % (u, tag, k)]
            d = v.double()
            assert abs(d.sum().item() - s[0]) <= 1e-6 * max(1.0, v.numel()) and abs(d.abs().sum().item() - s[1]) <= 1e-6 * max(1.0, v.numel())
            key = "u%d/%s/%s" % (u, tag, k)
            if key in gold.files:
                seen += 1
                assert np.abs(v.numpy() - gold[key]).max() <= 1e-6, (u, tag, k)
    return seen


def test_restatements_match_reference_fixtures():
    """CatOracle and CatReinforceOracle in fp32 against two update calls of the reference's A2C / Reinforce with the reference's
    CategoricalDisPolicy: infos to 1e-5 relative, every small parameter to 1e-6, every parameter's checksum."""
    from vision4leg_amd.torchrl.policies import CategoricalDisPolicy  # noqa: F401  (the feature under test exists)
    case = CAT_CASES[cc.FIXTURE_CASE]
    ga, gr = util.load_golden(cc.FIXTURES["a2c"]), util.load_golden(cc.FIXTURES["rf"])
    assert int(ga["seed"]) == int(gr["seed"]) == case["seed"]
    a2c, rf = cc.fresh_a2c_oracle(case), cc.fresh_rf_oracle(case)
    for u in range(2):
        info = a2c.update(*cc.batch_tensors(case, u), cc.LR, cc.LR)
        assert list(info) == cc.A2C_INFO_KEYS and len(info) == 8
        assert _check_fixture(ga, u, info, cc.A2C_INFO_KEYS, (("pf", a2c.pf), ("vf", a2c.vf))) >= 4
        info = rf.update(*cc.batch_tensors(case, u), cc.LR)
        assert list(info) == cc.RF_INFO_KEYS and len(info) == 10
        assert _check_fixture(gr, u, info, cc.RF_INFO_KEYS, (("pf", rf.pf),)) >= 2


@pytest.mark.parametrize("name", NAMES)
def test_case_conditions(name):
    """What a case's `scale` is chosen for, from the float64 restatement alone, on both batches: the largest probability in
    [0.6, 0.99], the smallest in [1e-6, 1e-2] (K = 2: in [1e-6, 0.4], see tests/cat_cases.py — there the smallest is 1 - the
    largest of its row), every action index in acts where B >= K; the probabilities are not the uniform ones of a fresh head."""
    from vision4leg_amd.torchrl.policies import CategoricalDisPolicy  # noqa: F401
    case = CAT_CASES[name]
    K, B = case["K"], case["B"]
    o = cc.fresh_a2c_oracle(case, dtype=torch.float64)
    for u in range(cc.updates_of(case)):
        obs, acts, _, _ = cc.batch_tensors(case, u, torch.float64)
        p, _, ent = cc.head(o.fwd(o.pf, obs, o.S, o.mode))
        pmax, pmin = p.max().item(), p.min().item()
        print("\n[%s] batch %d: largest p %.4f, smallest p %.3e, mean entropy %.4f (log K %.4f)" % (name, u, pmax, pmin, ent.mean().item(), np.log(K)))
        assert cc.P_MAX_RANGE[0] <= pmax <= cc.P_MAX_RANGE[1], pmax
        assert cc.P_MIN_RANGE[0] <= pmin <= (cc.P_MIN_RANGE[1] if K > 2 else 1.0 - cc.P_MAX_RANGE[0]), pmin
        assert pmin > 10 * torch.finfo(torch.float32).eps  # the reference's clamp to [eps, 1 - eps] is inactive
        assert acts.dtype == torch.int64 and tuple(acts.shape) == (B,) and 0 <= int(acts.min()) and int(acts.max()) < K
        if B >= K:
            assert set(acts.tolist()) == set(range(K))
        assert ent.mean().item() < 0.9 * np.log(K)


@pytest.mark.parametrize("name", NAMES)
def test_seed_rule(name):
    """tests/wide_cases.py "Seeds" for both learners: after the updates the GPU test runs, the fp32 restatement and the float64
    one agree to ORACLE_F32_ERR_MAX on every parameter."""
    from vision4leg_amd.torchrl.policies import CategoricalDisPolicy  # noqa: F401
    case = CAT_CASES[name]
    assert cc.SEED_LOG[name][0] == case["seed"]
    a32, a64 = cc.fresh_a2c_oracle(case), cc.fresh_a2c_oracle(case, dtype=torch.float64)
    r32, r64 = cc.fresh_rf_oracle(case), cc.fresh_rf_oracle(case, dtype=torch.float64)
    for u in range(cc.updates_of(case)):
        b32, b64 = cc.batch_tensors(case, u), cc.batch_tensors(case, u, torch.float64)
        a32.update(*b32, cc.LR, cc.LR)
        a64.update(*b64, cc.LR, cc.LR)
        r32.update(*b32, cc.LR)
        r64.update(*b64, cc.LR)
    wa = max((a32.pf[k].double() - a64.pf[k]).abs().max().item() for k in a32.pf)
    wa = max(wa, max((a32.vf[k].double() - a64.vf[k]).abs().max().item() for k in a32.vf))
    wr = max((r32.pf[k].double() - r64.pf[k]).abs().max().item() for k in r32.pf)
    print("\n[%s] fp32 vs float64 restatement: worst parameter A2C %.2e, REINFORCE %.2e" % (name, wa, wr))
    assert wa <= cc.ORACLE_F32_ERR_MAX and wr <= cc.ORACLE_F32_ERR_MAX, (wa, wr)


# ------------------------------------------------------------------------------------------ C ABI
NEW_SYMBOLS = ["v4l_net_set_categorical", "v4l_cat_head", "v4l_cat_sample"]


def test_abi_header_exports_and_pinned_sizes():
    from vision4leg_amd import _lib
    hdr = open(os.path.join(util.ROOT, "include", "v4l_hip.h")).read()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, hdr) and n in _lib.exported_symbols() and hasattr(dll, n), n
    l = _lib.lib()
    assert l.v4l_version() >= 115
    # every pinned size: the flag is no field of v4l_net_cfg and the feature adds no struct
    assert l.v4l_abi_sizeof(0) == ctypes.sizeof(_lib.NetCfg) == 104 and _lib.NetCfg._fields_[-1][0] == "activation"
    assert l.v4l_abi_sizeof(3) == -1 and l.v4l_abi_sizeof(5) == -1
    assert l.v4l_abi_sizeof(1) == ctypes.sizeof(_lib.PPOHyper) == 48 and l.v4l_abi_sizeof(4) == ctypes.sizeof(_lib.VMPOHyper) == 40
    assert l.v4l_abi_sizeof(2) == ctypes.sizeof(_lib.Rollout) == 56
    assert int(re.search(r"#define V4L_STATS (\d+)", hdr).group(1)) == _lib.V4L_STATS == 24
    assert int(re.search(r"#define V4L_A2C_STATS (\d+)", hdr).group(1)) == _lib.V4L_A2C_STATS == 16
    assert int(re.search(r"#define V4L_REINFORCE_STATS (\d+)", hdr).group(1)) == _lib.V4L_REINFORCE_STATS == 12
    assert _lib.A2C_CAT_INFO_KEYS == cc.A2C_INFO_KEYS and _lib.REINFORCE_INFO_KEYS == cc.RF_INFO_KEYS


def _cfg(**kw):
    from vision4leg_amd import _lib
    c = _lib.NetCfg()
    c.kind, c.compute, c.state_dim, c.out_dim = _lib.V4L_NET_MLP, _lib.V4L_F32, 9, 6
    c.n_enc_hidden, c.n_head_hidden = 1, 1
    c.enc_hidden[0] = c.head_hidden[0] = 16
    c.has_logstd = _lib.V4L_LOGSTD_NONE
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _create(c, flag=None):
    from vision4leg_amd import _lib
    l, h = _lib.lib(), ctypes.c_void_p()
    assert l.v4l_net_create(ctypes.byref(c), ctypes.byref(h)) == 0, l.v4l_last_error()
    rc = l.v4l_net_set_categorical(h, 1) if flag else 0
    return h, rc, (l.v4l_last_error().decode() if rc else "")


def test_setter_and_what_it_refuses():
    """v4l_net_set_categorical on host-side plans: accepted for a has_logstd = 0 state-MLP net with out_dim 2 .. 16, where it adds
    no parameter; a CNN net, a logstd parameter and out_dim 1 are refused with a message that names the condition (out_dim 17
    does not get past v4l_net_create: its message names V4L_MAX_ACT). A flagged pair makes a trainer and an actor; an unflagged
    has_logstd = 0 net is still refused as pf, and a flagged / unflagged policy pair too."""
    from vision4leg_amd import _lib
    l = _lib.lib()
    plain, _, _ = _create(_cfg())
    names = lambda h: [_info(l, h, i) for i in range(l.v4l_net_num_params(h))]
    for K in (2, 6, 16):
        h, rc, msg = _create(_cfg(out_dim=K), flag=True)
        assert rc == 0, msg
        assert l.v4l_net_num_params(h) == l.v4l_net_num_params(plain) and "logstd" not in names(h)
        l.v4l_net_destroy(h)
    for kw, word in ((dict(kind=_lib.V4L_NET_CNN, in_channels=4, img_hw=64, visual_dim=256), "V4L_NET_MLP"),
                     (dict(has_logstd=_lib.V4L_LOGSTD_PARAM), "has_logstd must be 0"), (dict(out_dim=1), "2 <= out_dim <= 16")):
        h, rc, msg = _create(_cfg(**kw), flag=True)
        assert rc != 0 and word in msg and msg.startswith("v4l_net_set_categorical"), (kw, msg)
        l.v4l_net_destroy(h)
    h = ctypes.c_void_p()
    c = _cfg(out_dim=17)
    assert l.v4l_net_create(ctypes.byref(c), ctypes.byref(h)) != 0 and "V4L_MAX_ACT" in l.v4l_last_error().decode()
    assert l.v4l_net_set_categorical(None, 1) != 0
    # has_logstd keeps its three values (tests/test_sd_cpu.py): no fourth one for this policy
    for bad in (3, -1):
        c = _cfg(has_logstd=bad)
        assert l.v4l_net_create(ctypes.byref(c), ctypes.byref(h)) != 0 and "0 (none), 1" in l.v4l_last_error().decode()
    cat1, rc1, _ = _create(_cfg(), flag=True)
    cat2, rc2, _ = _create(_cfg(), flag=True)
    vf, _, _ = _create(_cfg(out_dim=1))
    gauss, _, _ = _create(_cfg(has_logstd=_lib.V4L_LOGSTD_PARAM))
    assert rc1 == 0 and rc2 == 0
    tr, ac = ctypes.c_void_p(), ctypes.c_void_p()
    assert l.v4l_trainer_create(cat1, vf, cat2, ctypes.byref(tr)) == 0
    l.v4l_trainer_destroy(tr)
    assert l.v4l_actor_create(cat1, vf, 3, ctypes.byref(ac)) == 0
    assert l.v4l_actor_ws_floats(ac) > 0 and l.v4l_actor_route(ac, 1) == b"GENERAL" and l.v4l_actor_route(ac, 0) == b"GENERAL"
    l.v4l_actor_destroy(ac)
    one_kind = "Gaussian policies of one kind"
    assert l.v4l_trainer_create(plain, vf, plain, ctypes.byref(tr)) != 0 and one_kind in l.v4l_last_error().decode()
    assert l.v4l_trainer_create(cat1, vf, plain, ctypes.byref(tr)) != 0 and one_kind in l.v4l_last_error().decode()
    assert l.v4l_trainer_create(cat1, vf, gauss, ctypes.byref(tr)) != 0 and l.v4l_trainer_create(gauss, vf, cat1, ctypes.byref(tr)) != 0
    assert l.v4l_trainer_create(cat1, cat2, cat2, ctypes.byref(tr)) != 0  # a flagged net is no value net
    assert l.v4l_actor_create(plain, vf, 3, ctypes.byref(ac)) != 0 and "pf must be a Gaussian policy" in l.v4l_last_error().decode()
    # the flag can be taken back before bind: the net is a plain one again
    assert l.v4l_net_set_categorical(cat2, 0) == 0 and l.v4l_trainer_create(cat1, vf, cat2, ctypes.byref(tr)) != 0
    for n in (plain, cat1, cat2, vf, gauss):
        l.v4l_net_destroy(n)


def _info(l, h, i):
    name, ndim, numel, goff = ctypes.c_char_p(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64()
    shape = (ctypes.c_int64 * 4)()
    assert l.v4l_net_param_info(h, i, ctypes.byref(name), ctypes.byref(ndim), shape, ctypes.byref(numel), ctypes.byref(goff)) == 0
    return name.value.decode()


# ------------------------------------------------------------------------------------------ Python surface
def _nets(name="cat_mlp_k16"):
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    return cc.seeded_nets(networks, policies, CAT_CASES[name])


def test_class_surface_and_state_dict_keys():
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    case = CAT_CASES["cat_mlp_k16"]
    pf, vf = _nets()
    assert isinstance(pf, networks.Net) and pf.continuous is False and not hasattr(pf, "logstd")
    plain = networks.Net(input_shape=(case["S"],), output_shape=case["K"], append_hidden_shapes=list(case["head"]),
                         base_type=networks.MLPBase, hidden_shapes=list(case["enc"]))
    assert list(pf.state_dict()) == list(plain.state_dict())
    assert [tuple(v.shape) for v in pf.state_dict().values()] == [tuple(v.shape) for v in plain.state_dict().values()]
    cfg = pf._net_cfg()
    assert cfg.has_logstd == 0 and cfg.out_dim == case["K"] and cfg.kind == 0 and pf.categorical_head is True
    p = inspect.signature(policies.CategoricalDisPolicy.__init__).parameters
    assert list(p) == ["self", "kwargs"] and p["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    assert list(inspect.signature(policies.CategoricalDisPolicy.explore).parameters) == ["self", "x", "return_log_probs"]
    assert "torch.multinomial" in policies.CategoricalDisPolicy.explore.__doc__
    for K in (1, 17):
        with pytest.raises(NotImplementedError, match="2 <= output_shape <= 16"):
            policies.CategoricalDisPolicy(input_shape=case["S"], output_shape=K, base_type=networks.MLPBase, hidden_shapes=[16])


@needs_reference
def test_state_dict_keys_are_the_reference_class():
    out = _run("""
        import ref_stubs
        ref_stubs.install()
        import torch, torchrl.networks as rn, torchrl.policies as rp
        import vision4leg_amd.torchrl.networks as networks, vision4leg_amd.torchrl.policies as policies
        import cat_cases as cc
        case = cc.CAT_CASES["cat_mlp_k16"]
        ref, _ = cc.seeded_nets(rn, rp, case)
        mine, _ = cc.seeded_nets(networks, policies, case)
        assert type(ref).__module__.startswith("torchrl.policies") and ref.continuous is False
        assert list(ref.state_dict()) == list(mine.state_dict())
        mine.load_state_dict(ref.state_dict(), strict=True)
        ref.load_state_dict(mine.state_dict(), strict=True)
        assert all(torch.equal(v, mine.state_dict()[k]) for k, v in ref.state_dict().items())
        print("OK")
    """)
    assert out.startswith("OK")


def test_ppo_and_vmpo_refuse_the_class():
    """Raised before anything touches a device (the constructor's own GPU check would raise RuntimeError); A2C and Reinforce get
    as far as that check."""
    from vision4leg_amd.torchrl.algo import A2C, PPO, VMPO, Reinforce
    pf, vf = _nets()
    for cls in (PPO, VMPO):
        with pytest.raises(NotImplementedError, match=r"%s does not take policies\.CategoricalDisPolicy" % cls.__name__):
            cls(pf=pf, vf=vf, device="cpu")
    with pytest.raises(RuntimeError, match="needs a GPU"):
        A2C(pf=pf, vf=vf, device="cpu")
    with pytest.raises(RuntimeError, match="needs a GPU"):
        Reinforce(pf=pf, plr=1e-4, device="cpu")


def test_data_parallel_is_refused(monkeypatch):
    from vision4leg_amd.torchrl.algo import A2C, Reinforce
    from vision4leg_amd.torchrl.algo.on_policy import ppo
    pf, vf = _nets()
    monkeypatch.setattr(ppo, "_dist_world", lambda: 2)
    with pytest.raises(NotImplementedError, match="single process"):
        A2C(pf=pf, vf=vf, device="cpu")
    with pytest.raises(NotImplementedError, match="single process"):
        Reinforce(pf=pf, plr=1e-4, device="cpu")


class _DiscreteSpace:
    def __init__(self, n):
        self.n = n


class _StubEnv(util.FakeVecEnv):
    """A vec env whose constructor-time surface is all the collector's refusals need."""

    def __init__(self, E, S, discrete_n=None):
        super().__init__(E, S, 1, img=0)
        if discrete_n is not None:
            self.action_space = _DiscreteSpace(discrete_n)


def test_collector_refuses_mismatched_policy_and_env():
    """Both raise in the constructor's first lines, before a device is touched."""
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    from vision4leg_amd.torchrl.collector import VecOnPolicyCollector
    from vision4leg_amd.torchrl.replay_buffers import OnPolicyReplayBuffer
    case = CAT_CASES["cat_mlp_k16"]
    cat, vf = _nets()
    gauss = policies.GaussianContPolicyBasicBias(input_shape=case["S"], output_shape=3, base_type=networks.MLPBase, hidden_shapes=[16])
    buf = OnPolicyReplayBuffer(8, env_nums=2)
    with pytest.raises(NotImplementedError, match="Gaussian .continuous actions. only"):
        VecOnPolicyCollector(vf, env=_StubEnv(2, case["S"], discrete_n=case["K"]), eval_env=None, pf=gauss, replay_buffer=buf,
                             epoch_frames=8, device="cpu")
    with pytest.raises(NotImplementedError, match="CategoricalDisPolicy acts in a discrete env"):
        VecOnPolicyCollector(vf, env=_StubEnv(2, case["S"]), eval_env=None, pf=cat, replay_buffer=buf, epoch_frames=8, device="cpu")


@pytest.mark.parametrize("bad", [[0, 1, 16], [0, -1, 3], [0.5, 1, 2], [float("nan"), 1, 2]])
def test_out_of_range_acts_raise_before_upload(bad):
    """PPO._upload_batch's check of a categorical policy's host batch runs first: ValueError with no device in sight (the object
    is a bare instance: nothing of the constructor has run)."""
    from vision4leg_amd.torchrl.algo import A2C
    pf, _ = _nets()
    agent = A2C.__new__(A2C)
    agent.pf = pf
    batch = {"obs": np.zeros((3, 45)), "acts": np.array(bad), "advs": np.zeros((3, 1)), "estimate_returns": np.zeros((3, 1))}
    with pytest.raises(ValueError, match=r"integer action indices in \[0, 16\)"):
        agent._upload_batch(batch, A2C._rollout_keys)


def test_a2c_info_keys_of_a_categorical_policy():
    from vision4leg_amd import _lib
    from vision4leg_amd.torchrl.algo import A2C
    agent = A2C.__new__(A2C)
    row = np.arange(_lib.V4L_A2C_STATS, dtype=np.float32)
    agent.pf = _nets()[0]
    info = agent._info(None, row)
    assert list(info) == cc.A2C_INFO_KEYS and info["ent"] == 10.0 and info["log_prob"] == 11.0 and info["v_pred/min"] == 5.0
    agent.pf = torch.nn.Linear(2, 2)
    assert list(agent._info(None, row)) == _lib.A2C_INFO_KEYS


def _run(code):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([util.ROOT, os.path.join(util.ROOT, "tests")]), PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    return r.stdout


def test_overlay_signature():
    import vision4leg_amd.overlay as overlay
    p = inspect.signature(overlay.install).parameters
    assert list(p)[-1] == "discrete" and p["discrete"].default is False
    assert list(p)[:-1] == ["fast_path", "reference_package", "vmpo", "a2c", "state_std", "reinforce"]


@needs_reference
def test_overlay_opt_in_rebinds_one_name():
    """install() leaves torchrl.policies.CategoricalDisPolicy the reference's; install(discrete=True) rebinds that one name, on
    the package and on the module that defines it; uninstall() puts the reference's back."""
    out = _run("""
        import ref_stubs
        ref_stubs.install()
        import vision4leg_amd.overlay as overlay
        import vision4leg_amd.torchrl.policies as hip_policies
        base = overlay.install()
        import torchrl.policies, torchrl.policies.discrete_policies as ref_mod
        ref_cls = torchrl.policies.CategoricalDisPolicy
        assert ref_cls.__module__.startswith("torchrl.policies") and ref_cls is not hip_policies.CategoricalDisPolicy
        overlay.uninstall()
        report = overlay.install(a2c=True, reinforce=True, state_std=True)
        assert "policies.CategoricalDisPolicy" not in report and torchrl.policies.CategoricalDisPolicy is ref_cls
        overlay.uninstall()
        report = overlay.install(discrete=True)
        assert set(report) - set(base) == {"policies.CategoricalDisPolicy"}
        from torchrl.policies import CategoricalDisPolicy
        assert CategoricalDisPolicy is hip_policies.CategoricalDisPolicy and ref_mod.CategoricalDisPolicy is CategoricalDisPolicy
        assert ref_mod.UniformPolicyDiscrete.__module__.startswith("torchrl.policies")
        overlay.uninstall()
        assert torchrl.policies.CategoricalDisPolicy is ref_cls and ref_mod.CategoricalDisPolicy is ref_cls
        print("OK")
    """)
    assert out.startswith("OK")


# ------------------------------------------------------------------------------------------ inverse CDF
@pytest.mark.parametrize("name", NAMES)
def test_inverse_cdf_boundary_band(name):
    """The reference arithmetic of tests/test_gpu_cat.py::test_sample alone: fp32 probabilities of the case's first batch (the
    fp32 restatement, rows cycled to 4096), float64 running sums, 4096 uniforms from a fixed seed. At most 1 % of the uniforms
    lie within 1e-6 of a boundary — the rows the GPU test leaves out — and every index is in [0, K)."""
    from vision4leg_amd.torchrl.policies import CategoricalDisPolicy  # noqa: F401
    case = CAT_CASES[name]
    o = cc.fresh_a2c_oracle(case)
    obs = cc.batch_tensors(case, 0)[0]
    probs = cc.head(o.fwd(o.pf, obs, o.S, o.mode))[0].detach().numpy().astype(np.float32)
    u = cc.uniforms(case)
    rows = probs[np.arange(len(u)) % len(probs)]
    idx, dist = cc.inverse_cdf(rows, u)
    near = float((dist <= 1e-6).mean())
    print("\n[%s] %d of %d uniforms within 1e-6 of a boundary" % (name, int((dist <= 1e-6).sum()), len(u)))
    assert u.dtype == np.float32 and len(u) == 4096 and (u >= 0).all() and (u < 1).all()
    assert near <= 0.01
    assert idx.min() >= 0 and idx.max() < case["K"] and len(set(idx.tolist())) >= 2
    # the definition, spelled out on a row: the first k whose running sum exceeds u, K - 1 if none does
    i, d = cc.inverse_cdf(np.array([[0.25, 0.25, 0.5], [0.25, 0.25, 0.5], [0.5, 0.25, 0.125]], dtype=np.float32), [0.25, 0.49, 0.9])
    assert i.tolist() == [1, 1, 2] and abs(d[0]) == 0.0
