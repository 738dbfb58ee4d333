"""CPU: REINFORCE (tests/reinforce_cases.py). The restatement against the fixtures the unmodified reference produced
(tests/golden/make_golden_reinforce.py), the seed rule of every case, the C ABI's REINFORCE entries against the header and the
ctypes mirror, `algo.Reinforce`'s constructor and what it refuses, the zero critic, and the overlay's opt-in. No GPU: nothing
here launches a kernel."""
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
import reinforce_cases as rc

REF = "/root/reference"
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "torchrl")), reason="reference tree not present")


@pytest.mark.parametrize("name", rc.FIXTURE_CASES)
def test_restatement_matches_reference_fixture(name):
    """ReinforceOracle in fp32 against two Reinforce.update calls of the reference: 10 infos to 1e-5 relative, every small
    parameter to 1e-6, every parameter's checksum."""
    from vision4leg_amd.torchrl.algo import Reinforce  # noqa: F401  (the feature under test exists)
    case = rc.REINFORCE_CASES[name]
    gold = util.load_golden(name)
    assert int(gold["seed"]) == case["seed"]
    oracle = rc.fresh_oracle(case)
    for u in range(2):
        info = oracle.update(*rc.batch_tensors(case, u), rc.LR)
        assert list(info) == rc.INFO_KEYS
        for k, want in zip(rc.INFO_KEYS, gold["u%d/info" % u]):
            assert abs(info[k] - want) <= 1e-5 * max(1.0, abs(want)), (u, k, info[k], want)
        seen = 0
        for k, v in oracle.pf.items():
            s = gold["u%d/sum/pf/%s" % (u, k)]
            d = v.double()
            assert abs(d.sum().item() - s[0]) <= 1e-6 * max(1.0, v.numel()) and abs(d.abs().sum().item() - s[1]) <= 1e-6 * max(1.0, v.numel())
            key = "u%d/pf/%s" % (u, k)
            if key in gold.files:
                seen += 1
                assert np.abs(v.numpy() - gold[key]).max() <= 1e-6, (u, k)
        assert seen >= 4
    assert oracle.pf_opt.param_groups[0]["eps"] == rc.ADAM_EPS == 1e-8


@pytest.mark.parametrize("name", list(rc.REINFORCE_CASES))
def test_seed_rule(name):
    """tests/wide_cases.py "Seeds" for REINFORCE: after the updates the GPU test runs, the fp32 restatement and the float64 one
    agree to ORACLE_F32_ERR_MAX on every parameter."""
    from vision4leg_amd.torchrl.algo import Reinforce  # noqa: F401
    case = rc.REINFORCE_CASES[name]
    o32, o64 = rc.fresh_oracle(case), rc.fresh_oracle(case, dtype=torch.float64)
    for u in range(rc.updates_of(case)):
        o32.update(*rc.batch_tensors(case, u), rc.LR)
        o64.update(*rc.batch_tensors(case, u, torch.float64), rc.LR)
    worst = max((o32.pf[k].double() - o64.pf[k]).abs().max().item() for k in o32.pf)
    print("\n[%s] fp32 vs float64 restatement: worst parameter %.2e" % (name, worst))
    assert worst <= rc.ORACLE_F32_ERR_MAX, worst
    assert rc.SEED_LOG[name][0] == case["seed"]


def test_loss_rows_wide_block_oracle():
    """What tests/test_gpu_reinforce.py::test_loss_rows[rf_mlp_odd@513] compares with, alone: the float64 loss stage on the
    restatement's head rows at 513 rows, with a log sigma beyond either end of the clamp, is finite everywhere, and its
    d(loss)/d(logstd) is exactly 0 at those two columns and at no other."""
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    case = util.loss_rows_case(rc.REINFORCE_CASES, "rf_mlp_odd@513")
    assert case["B"] == 513 and case["A"] == 12 and rc.REINFORCE_CASES["rf_mlp_odd"]["B"] == 23
    pf = rc.seeded_policy(networks, policies, case)
    util.spread_policy_head(pf, util.loss_rows_logstd(case["A"], False, both_ends=True))
    oracle = rc.oracle_of(pf.state_dict(), case)
    head = oracle.fwd({k: v for k, v in oracle.pf.items() if k != "logstd"}, rc.batch_tensors(case, 0)[0], case["S"], "f32")
    b = rc.host_batch(case, 0)
    dout, dls, info = rc.loss_stage64(head.detach().numpy(), pf.state_dict()["logstd"].numpy().reshape(-1), b["acts"].astype(np.float32),
                                      b["advs"].astype(np.float32).reshape(-1), case["A"], rc.ENTROPY_COEFF, False)
    assert dout.shape == (513, 12) and torch.isfinite(dout).all() and torch.isfinite(dls).all()
    assert np.isfinite(list(info.values())).all()
    assert dls[0].item() == 0.0 and dls[-1].item() == 0.0 and (dls[1:-1] != 0).all()


def test_abi_header_exports_and_mirror():
    from vision4leg_amd import _lib
    hdr = open(os.path.join(util.ROOT, "include", "v4l_hip.h")).read()
    names = ["v4l_trainer_reinforce_actor_grads", "v4l_trainer_reinforce_update_next", "v4l_trainer_reinforce_update_run",
             "v4l_trainer_reinforce_graph_counts"]
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, hdr) and n in _lib.exported_symbols() and hasattr(dll, n), n
    l = _lib.lib()
    assert l.v4l_version() >= 114
    assert int(re.search(r"#define V4L_REINFORCE_STATS (\d+)", hdr).group(1)) == _lib.V4L_REINFORCE_STATS == 12
    assert _lib.REINFORCE_INFO_KEYS == rc.INFO_KEYS and len(rc.INFO_KEYS) == 10
    # the pinned sizes did not move; REINFORCE added no struct
    assert l.v4l_abi_sizeof(3) == -1 and l.v4l_abi_sizeof(5) == -1
    assert l.v4l_abi_sizeof(1) == ctypes.sizeof(_lib.PPOHyper) == 48 and l.v4l_abi_sizeof(4) == ctypes.sizeof(_lib.VMPOHyper) == 40
    assert l.v4l_abi_sizeof(0) == ctypes.sizeof(_lib.NetCfg) and l.v4l_abi_sizeof(2) == ctypes.sizeof(_lib.Rollout) == 56


def test_hook_table_and_engine_signatures():
    from vision4leg_amd import _lib
    from vision4leg_amd.engine import HipTrainer
    from vision4leg_amd.torchrl.algo import A2C, PPO, Reinforce
    from vision4leg_amd.torchrl.algo.on_policy.second_record import _SecondRecordPPO
    assert issubclass(Reinforce, _SecondRecordPPO) and issubclass(Reinforce, PPO)
    assert Reinforce._second_stats == _lib.V4L_REINFORCE_STATS and Reinforce._passes == 1 and Reinforce._syncs_target is False
    assert (Reinforce._run_entry, Reinforce._next_entry) == ("reinforce_update_run", "reinforce_update_next")
    ppo_keys = ("acts", "advs", "estimate_returns", "values")
    assert Reinforce._rollout_keys == ppo_keys[:len(Reinforce._rollout_keys)] and Reinforce._rollout_keys[:2] == ("acts", "advs")
    for m in ("_run", "_buffers", "update", "update_per_epoch", "_update_epoch_resident", "_refuse"):
        assert getattr(Reinforce, m) is getattr(A2C, m) is getattr(_SecondRecordPPO, m), m
    assert str(inspect.signature(HipTrainer.reinforce_actor_grads)) == "(self, ro, n, rstats_all)"
    assert str(inspect.signature(HipTrainer.reinforce_update_next)) == "(self, ro, n, rstats_all, graph=False)"
    assert str(inspect.signature(HipTrainer.reinforce_update_run)) == "(self, ro, n, count, rstats_all, graph=True)"
    assert callable(HipTrainer.reinforce_graph_counts)


@needs_reference
def test_info_keys_are_the_references_order():
    """The key list against the reference's source text: the order in which reinforce.py assigns info[...]."""
    src = open(os.path.join(REF, "torchrl", "algo", "on_policy", "reinforce.py")).read()
    assert re.findall(r"info\['([^']+)'\]\s*=", src) == rc.INFO_KEYS


def _pf(name="rf_mlp_odd"):
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    return rc.seeded_policy(networks, policies, rc.REINFORCE_CASES[name])


def test_signature_is_the_references():
    from vision4leg_amd.torchrl.algo import PPO, Reinforce
    p = inspect.signature(Reinforce.__init__).parameters
    assert list(p) == ["self", "pf", "plr", "optimizer_class", "entropy_coeff", "kwargs"]
    assert p["plr"].default is inspect.Parameter.empty and p["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    assert p["optimizer_class"].default is torch.optim.Adam and p["entropy_coeff"].default == 0.001
    assert Reinforce.train is PPO.train and Reinforce.snapshot is PPO.snapshot
    assert Reinforce.process_epoch_samples is PPO.process_epoch_samples
    assert Reinforce._call_eps is None and PPO._call_eps == 1e-5


def test_optimizer_eps_is_torchs_default():
    """reinforce.py:26-29 hands optimizer_class no eps: torch's 1e-8, or a partial's own; PPO's call-time 1e-5 is unchanged."""
    import functools
    from vision4leg_amd import optim as hip_optim
    assert hip_optim.resolve(torch.optim.Adam, None, lr=1e-4, eps=None).eps == 1e-8
    assert hip_optim.resolve(functools.partial(torch.optim.AdamW, eps=1e-6), None, lr=1e-4, eps=None).eps == 1e-6
    assert hip_optim.resolve(torch.optim.Adam, None, lr=1e-4).eps == 1e-5


@pytest.mark.parametrize("kw", [dict(skip_nonfinite_steps=True), dict(save_train_state=True), dict(resume="/nonexistent")])
def test_refused_options(kw):
    """Raised before anything touches a device (the constructor's own GPU check would raise RuntimeError)."""
    from vision4leg_amd.torchrl.algo import Reinforce
    pf = _pf()
    with pytest.raises(NotImplementedError):
        Reinforce(pf, rc.LR, device="cpu", **kw)
    with pytest.raises(RuntimeError, match="needs a GPU"):  # nothing refused: the PPO shell's device check is reached
        Reinforce(pf, rc.LR, device="cpu")


@pytest.mark.parametrize("key", ["vf", "vlr", "clip_para", "opt_epochs", "clipped_value_loss"])
def test_refused_keywords(key):
    from vision4leg_amd.torchrl.algo import Reinforce
    with pytest.raises(TypeError, match="unexpected keyword argument '%s'" % key):
        Reinforce(_pf(), rc.LR, device="cpu", **{key: 1})


def test_refused_policy_and_critic():
    from vision4leg_amd.torchrl.algo import Reinforce
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    torch.manual_seed(1)
    sd = policies.GaussianContPolicy(input_shape=45, output_shape=2 * 3, base_type=networks.MLPBase, hidden_shapes=[32],
                                     append_hidden_shapes=[16])
    with pytest.raises(NotImplementedError, match="GaussianContPolicy"):
        Reinforce(sd, rc.LR, device="cpu")
    case = rc.REINFORCE_CASES["rf_mlp_odd"]
    pf, vf = util.build_nets(networks, policies, case)

    class Coll:
        epoch_frames = 1
    coll = Coll()
    coll.vf = vf  # a real critic
    with pytest.raises(ValueError, match="networks.ZeroNet.*networks.zero_critic"):
        Reinforce(pf, rc.LR, device="cpu", collector=coll)
    coll.vf = networks.zero_critic(_pf())  # a zero critic of ANOTHER policy
    with pytest.raises(ValueError, match="networks.zero_critic"):
        Reinforce(pf, rc.LR, device="cpu", collector=coll)
    for ok in (networks.zero_critic(pf), networks.ZeroNet()):
        coll.vf = ok
        with pytest.raises(RuntimeError, match="needs a GPU"):
            Reinforce(pf, rc.LR, device="cpu", collector=coll)


def test_refused_data_parallel(monkeypatch):
    from vision4leg_amd.torchrl.algo import Reinforce
    from vision4leg_amd.torchrl.algo.on_policy import ppo
    pf = _pf()
    monkeypatch.setattr(ppo, "_dist_world", lambda: 2)
    with pytest.raises(NotImplementedError, match="single process"):
        Reinforce(pf, rc.LR, device="cpu")
    monkeypatch.setattr(ppo, "_dist_world", lambda: 1)
    monkeypatch.setenv("V4L_FORCE_DP_PHASES", "1")
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    with pytest.raises(NotImplementedError, match="single process"):
        Reinforce(pf, rc.LR, device="cpu")


# ------------------------------------------------------------------------------------------ the zero critic
def test_zero_net():
    import vision4leg_amd.torchrl.networks as networks
    z = networks.ZeroNet()
    assert list(z.parameters()) == [] and torch.equal(z(torch.randn(5, 7)), torch.zeros(1))


@pytest.mark.parametrize("name", ["rf_mlp_odd", "rf_loco", "rf_cnn"])
def test_zero_critic(name):
    """Trunk modules identical to pf's, the head its own with an all-zero last layer, no own parameter requires grad, the
    engine's plan is a value net of pf's kind and geometry; building it draws nothing from torch's generator."""
    import vision4leg_amd.torchrl.networks as networks
    pf = _pf(name)
    rng = torch.get_rng_state()
    vf = networks.zero_critic(pf)
    assert torch.equal(rng, torch.get_rng_state())
    mlp = name.startswith("rf_mlp")
    if mlp:
        assert vf.base is pf.base and type(vf) is networks.Net
        head = vf.seq_append_fcs
    else:
        assert vf.encoder is pf.encoder and not hasattr(vf, "logstd")
        assert type(vf) is (networks.LocoTransformer if name == "rf_loco" else networks.ImpalaEncoderProjNet)
        head = vf.visual_seq_append_fcs if name == "rf_loco" else vf.seq_append_fcs
    last = head[-1]
    assert tuple(last.weight.shape)[0] == 1 and not last.weight.any() and not last.bias.any()
    shared = {id(p) for p in pf.parameters()}
    own = [p for p in vf.parameters() if id(p) not in shared]
    trunk = [p for p in vf.parameters() if id(p) in shared]
    assert own and trunk and not any(p.requires_grad for p in own) and all(p.requires_grad for p in trunk)
    pf_head = {id(p) for k, p in pf.named_parameters() if "append" in k or k == "logstd"}
    assert not pf_head & {id(p) for p in vf.parameters()}  # the head's hidden layers are its own
    cp, cv = pf._net_cfg(), vf._net_cfg()
    assert cv.out_dim == 1 and cv.has_logstd == 0
    for f in ("kind", "state_dim", "n_enc_hidden", "n_head_hidden", "n_layers", "ff_dim", "visual_dim", "token_dim", "activation"):
        assert getattr(cp, f) == getattr(cv, f), f
    assert list(cp.head_hidden) == list(cv.head_hidden) and list(cp.enc_hidden) == list(cv.enc_hidden)
    assert networks.is_zero_critic(vf, pf) and not networks.is_zero_critic(vf, _pf(name))
    _, real = util.build_nets(networks, __import__("vision4leg_amd.torchrl.policies", fromlist=["x"]), rc.REINFORCE_CASES[name])
    assert not networks.is_zero_critic(real, pf) and not networks.is_zero_critic(networks.ZeroNet(), pf)


def test_zero_critic_keeps_tanh_activation():
    import vision4leg_amd.torchrl.networks as networks
    pf = _pf("rf_mlp_tact")
    vf = networks.zero_critic(pf)
    assert vf.activation_func is torch.nn.Tanh and vf._net_cfg().activation == pf._net_cfg().activation != 0


def test_collector_swaps_a_zero_net():
    """VecOnPolicyCollector given the reference's vacant critic holds a zero critic on pf's trunk; any other vf is kept."""
    import vision4leg_amd.torchrl.networks as networks
    from vision4leg_amd import recipes
    from vision4leg_amd.torchrl.collector import VecOnPolicyCollector
    from vision4leg_amd.torchrl.replay_buffers import OnPolicyReplayBuffer
    case = rc.REINFORCE_CASES["rf_mlp_odd"]
    pf = _pf()

    def coll(vf):
        return VecOnPolicyCollector(vf, env=recipes.ZeroCostVecEnv(2, case, seed=2), eval_env=recipes.ZeroCostVecEnv(2, case, seed=3),
                                    pf=pf, replay_buffer=OnPolicyReplayBuffer(max_replay_buffer_size=8, env_nums=2,
                                                                              time_limit_filter=True),
                                    device="cpu", epoch_frames=8)
    assert networks.is_zero_critic(coll(networks.ZeroNet()).vf, pf)
    other = networks.zero_critic(pf)
    assert coll(other).vf is other


# ------------------------------------------------------------------------------------------ the overlay
def _run(code):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([util.ROOT, os.path.join(util.ROOT, "tests")]), PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    return r.stdout


@needs_reference
def test_overlay_opt_in():
    """install() is what it was; install(reinforce=True) rebinds torchrl.algo.Reinforce on the package and on the module that
    defines it, and networks.ZeroNet, adds "algo.Reinforce" to the report and nothing else; uninstall() puts the reference's
    back."""
    out = _run("""
        import ref_stubs
        ref_stubs.install()
        import vision4leg_amd.overlay as overlay
        import vision4leg_amd.torchrl.algo as hip_algo
        import vision4leg_amd.torchrl.networks as hip_networks
        plain = overlay.install()
        import torchrl.algo, torchrl.networks, torchrl.networks.nets as ref_nets, torchrl.algo.on_policy.reinforce as ref_mod
        ref_cls, ref_zero, ref_a2c, ref_vmpo = torchrl.algo.Reinforce, torchrl.networks.ZeroNet, torchrl.algo.A2C, torchrl.algo.VMPO
        assert ref_cls.__module__.startswith("torchrl.algo") and ref_cls is not hip_algo.Reinforce and ref_zero is not hip_networks.ZeroNet
        assert "algo.Reinforce" not in plain
        overlay.uninstall()
        for kw in (dict(vmpo=True), dict(a2c=True), dict(state_std=True), dict(fast_path=True)):
            report = overlay.install(**kw)
            assert "algo.Reinforce" not in report and torchrl.algo.Reinforce is ref_cls and torchrl.networks.ZeroNet is ref_zero
            overlay.uninstall()
        report = overlay.install(reinforce=True)
        assert set(report) - set(plain) == {"algo.Reinforce"} and {k: report[k] for k in plain} == plain
        from torchrl.algo import PPO, Reinforce
        assert Reinforce is hip_algo.Reinforce and PPO is hip_algo.PPO and ref_mod.Reinforce is hip_algo.Reinforce
        assert torchrl.networks.ZeroNet is hip_networks.ZeroNet and ref_nets.ZeroNet is hip_networks.ZeroNet
        assert torchrl.algo.A2C is ref_a2c and torchrl.algo.VMPO is ref_vmpo
        overlay.uninstall()
        assert torchrl.algo.Reinforce is ref_cls and ref_mod.Reinforce is ref_cls
        assert torchrl.networks.ZeroNet is ref_zero and ref_nets.ZeroNet is ref_zero
        print("OK")
    """)
    assert out.startswith("OK")
