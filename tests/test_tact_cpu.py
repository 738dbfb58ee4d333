"""CPU suite (`-m "not gpu"`): activation_func=nn.Tanh on the state-MLP net (networks.Net + MLPBase, V4L_NET_MLP) — the
host-side part of the C ABI (config field, plan checks, error texts), the Python shell's checks, and the restatement of
tests/tact_cases.py against what the unmodified reference produced (tests/golden/make_golden_tact.py). The GPU tests
(tests/test_gpu_tact.py) compare the engine with this restatement."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn

import util
from oracle import ppo_oracle as orc
from tact_cases import FIXTURE_CASES, TACT_CASES
from wide_cases import ORACLE_F32_ERR_MAX


def _nets(case, seed=None):
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    torch.manual_seed(case["seed"] if seed is None else seed)
    return util.build_nets(networks, policies, case)


def _cfg(kind, activation):
    """The shipped geometry of a net kind (tests/test_wide_actions_cpu.py::_cfg) with the activation selector set."""
    from vision4leg_amd import _lib
    c = _lib.NetCfg()
    c.kind, c.compute, c.out_dim, c.has_logstd = kind, _lib.V4L_F16, 6, 1
    c.state_dim, c.n_enc_hidden = 84, 2
    c.enc_hidden[0] = c.enc_hidden[1] = 256
    c.n_head_hidden = 2
    c.head_hidden[0] = c.head_hidden[1] = 256
    if kind != _lib.V4L_NET_MLP:
        c.in_channels, c.img_hw, c.visual_dim = 4, 64, 256
    if kind == _lib.V4L_NET_LOCO:
        c.token_dim, c.n_layers, c.ff_dim = 64, 2, 256
    c.activation = activation
    return c


def _create(cfg):
    from vision4leg_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    rc = L.v4l_net_create(C.byref(cfg), C.byref(h))
    err = (L.v4l_last_error() or b"").decode()
    return rc, h, err


@pytest.mark.parametrize("name", list(TACT_CASES))
def test_build_nets_plan_carries_the_tanh_selector(name):
    """build_nets(case).hip: the plan exists and carries V4L_ACT_TANH on both nets; the ReLU twin of the case keeps 0."""
    from vision4leg_amd import _lib
    case = TACT_CASES[name]
    pf, vf = _nets(case)
    assert pf.activation_func is nn.Tanh and vf.activation_func is nn.Tanh and pf.base.activation_func is nn.Tanh
    assert all(isinstance(m, nn.Tanh) for m in list(pf.base.seq_fcs)[1::2] + list(pf.seq_append_fcs)[1::2])
    for net in (pf, vf):
        assert net.hip.cfg.kind == _lib.V4L_NET_MLP and net.hip.cfg.activation == _lib.V4L_ACT_TANH == 1
    assert pf.hip.cfg.tanh_action == int(case["kind"].endswith("_tanh"))
    rpf, rvf = _nets(dict(case, kind=case["kind"].replace("_tact", "")))
    assert rpf.hip.cfg.activation == rvf.hip.cfg.activation == _lib.V4L_ACT_RELU == 0
    assert rpf.hip.param_names == pf.hip.param_names and rpf.hip.param_shapes == pf.hip.param_shapes  # no parameter of its own
    for (k, a), (k2, b) in zip(pf.state_dict().items(), rpf.state_dict().items()):
        assert k == k2 and torch.equal(a, b)  # (nor another seeded initialisation: base.py:8-44 never asks the activation)


def test_constants_field_and_version():
    from vision4leg_amd import _lib
    hdr = open(util.ROOT + "/include/v4l_hip.h").read()
    assert "#define V4L_ACT_RELU 0" in hdr and "#define V4L_ACT_TANH 1" in hdr
    assert _lib.NetCfg._fields_[-1][0] == "activation"  # at the end: every older field keeps its offset
    assert _lib.NetCfg().activation == _lib.V4L_ACT_RELU  # a zero-initialised config stays ReLU
    assert _lib.lib().v4l_version() >= 108
    assert _lib.lib().v4l_abi_sizeof(0) == C.sizeof(_lib.NetCfg)


@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_plan_matches_reference_state_dict(name):
    """The library's parameter table against the reference's own state_dict as the fixture recorded it."""
    case, gold = TACT_CASES[name], util.load_golden("ppo_" + name)
    pf, vf = _nets(case, seed=0)
    for tag, net in (("pf", pf), ("vf", vf)):
        want = {f[len("shape_%s/" % tag):]: tuple(int(x) for x in gold[f]) for f in gold.files if f.startswith("shape_%s/" % tag)}
        hip = net.hip
        assert sorted(hip.param_names) == sorted(want), (name, tag)
        assert dict(zip(hip.param_names, hip.param_shapes)) == want, (name, tag)
        assert hip.total_params == sum(int(np.prod(s)) for s in want.values())


def test_library_refuses_unknown_activation_and_tanh_on_other_kinds():
    from vision4leg_amd import _lib
    rc, h, err = _create(_cfg(_lib.V4L_NET_MLP, _lib.V4L_ACT_TANH))
    assert rc == 0 and h.value, err
    _lib.lib().v4l_net_destroy(h)
    for bad in (2, -1, 7):
        for kind in (_lib.V4L_NET_MLP, _lib.V4L_NET_LOCO):
            rc, h, err = _create(_cfg(kind, bad))
            assert rc != 0 and not h.value
            assert "activation" in err and str(bad) in err, err
    for kind in (_lib.V4L_NET_CNN, _lib.V4L_NET_LOCO):
        rc, h, err = _create(_cfg(kind, _lib.V4L_ACT_TANH))
        assert rc != 0 and not h.value
        assert "activation" in err and "V4L_ACT_TANH" in err and "V4L_NET_MLP" in err, err
        rc, h, err = _create(_cfg(kind, _lib.V4L_ACT_RELU))
        assert rc == 0, err
        _lib.lib().v4l_net_destroy(h)
    for kind in (_lib.V4L_NET_CNN_VIS, _lib.V4L_NET_LOCO_VIS):
        c = _cfg(kind, _lib.V4L_ACT_TANH)
        c.state_dim = c.n_enc_hidden = 0
        if kind == _lib.V4L_NET_LOCO_VIS:
            c.token_dim, c.n_layers, c.ff_dim = 64, 2, 256
        rc, h, err = _create(c)
        assert rc != 0 and "activation" in err and "V4L_NET_MLP" in err, err


def test_shell_refuses_tanh_elsewhere_and_mixed_last_activation():
    import vision4leg_amd.torchrl.networks as networks
    head = dict(append_hidden_shapes=[256, 256], activation_func=nn.Tanh)
    tf = dict(transformer_params=[[1, 256], [1, 256]])
    img = (4, 64, 64)
    loco_enc = networks.LocoTransformerEncoder(in_channels=4, state_input_dim=84, hidden_shapes=[256, 256])
    fuse_enc = networks.NatureFuseEncoder(in_channels=4, state_input_dim=93, hidden_shapes=[256, 256], visual_dim=256)
    others = [
        networks.LocoTransformer(encoder=loco_enc, output_shape=1, state_input_shape=84, visual_input_shape=img, **tf, **head),
        networks.ImpalaEncoderProjNet(encoder=fuse_enc, output_shape=1, state_input_shape=93, visual_input_shape=img, **head),
        networks.Transformer(encoder=networks.TransformerEncoder(in_channels=4), output_shape=1, visual_input_shape=img, **tf, **head),
        networks.NatureEncoderProjNet(encoder=networks.NatureEncoder(in_channels=4), output_shape=1, visual_input_shape=img, **head),
    ]
    for net in others:
        with pytest.raises(NotImplementedError, match="Tanh runs on networks.Net"):
            net.hip
    # a Tanh proprio MLP under a ReLU net of another kind
    tanh_enc = networks.LocoTransformerEncoder(in_channels=4, state_input_dim=84, hidden_shapes=[256, 256], activation_func=nn.Tanh)
    with pytest.raises(NotImplementedError, match="networks.Net only"):
        networks.LocoTransformer(encoder=tanh_enc, output_shape=1, state_input_shape=84, visual_input_shape=img,
                                 append_hidden_shapes=[256, 256], **tf).hip
    # the state-MLP net itself: a last activation of its own, LayerNorm and other activations stay refused
    mk = lambda **kw: networks.Net(input_shape=8, output_shape=2, base_type=networks.MLPBase, hidden_shapes=[16, 16],
                                   append_hidden_shapes=[16], **kw)
    for kw in (dict(activation_func=nn.Tanh, last_activation_func=nn.ReLU), dict(last_activation_func=nn.Tanh),
               dict(activation_func=nn.Tanh, last_activation_func=nn.Identity), dict(activation_func=nn.Tanh, add_ln=True),
               dict(activation_func=nn.Sigmoid), dict(add_ln=True)):
        with pytest.raises(NotImplementedError):
            mk(**kw).hip
    net = mk(activation_func=nn.Tanh)
    net.base = networks.MLPBase(input_shape=8, hidden_shapes=[16, 16])  # a ReLU base under a Tanh head
    with pytest.raises(NotImplementedError):
        net.hip
    assert mk(activation_func=nn.Tanh, last_activation_func=nn.Tanh).hip.cfg.activation == 1
    assert mk().hip.cfg.activation == 0


@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_restatement_matches_reference_golden(name):
    """tests/test_wide_actions_cpu.py::test_oracle_matches_reference_golden_at_a12's statements and tolerances on the Tanh
    fixture, on both recorded updates."""
    case, gold = TACT_CASES[name], util.load_golden("ppo_" + name)
    pf, vf = _nets(case)
    for tag, net in (("pf", pf), ("vf", vf)):
        sd = net.state_dict()
        assert sorted("init_%s/%s" % (tag, k) for k in sd) == sorted(f for f in gold.files if f.startswith("init_%s/" % tag))
        for k, v in sd.items():
            fp = gold["init_%s/%s" % (tag, k)]
            assert abs(v.double().sum().item() - fp[0]) <= 1e-5 * max(1.0, fp[1]), (tag, k)
            assert abs(v.double().abs().sum().item() - fp[1]) <= 1e-5 * max(1.0, fp[1]), (tag, k)
    opf = {k: v.clone() for k, v in pf.state_dict().items()}
    ovf = util.share_encoder(opf, {k: v.clone() for k, v in vf.state_dict().items()}, case["kind"])
    b = util.make_batch(case)
    t = lambda a: torch.tensor(a, dtype=torch.float32)
    pm = {k: v for k, v in opf.items() if k != "logstd"}
    with torch.no_grad():
        om = orc.FORWARDS[case["kind"]](pm, t(b["obs"]), case["S"])
        ov = orc.FORWARDS[case["kind"]](ovf, t(b["obs"]), case["S"])
        relu = orc.mlp_forward(pm, t(b["obs"]), case["S"])
    assert tuple(om.shape) == (case["B"], case["A"])
    assert util.rel_err(om, gold["fwd_mean"]) < 2e-5 and util.rel_err(ov, gold["fwd_value"]) < 2e-5
    assert util.rel_err(relu, gold["fwd_mean"]) > 0.1  # the fixture tells the activations apart
    oracle = orc.PPOOracle(case["kind"], opf, ovf, {k: v.clone() for k, v in opf.items()}, case["S"])
    oracle.sync_target()
    for u in range(2):
        b = util.make_batch(case, update=u)
        info = oracle.update(t(b["obs"]), t(b["acts"]), t(b["advs"]), t(b["estimate_returns"]), t(b["values"]), 1e-4, 1e-4)
        for k, g in zip(util.STAT_KEYS, gold["u%d/info" % u]):
            assert abs(info[k] - g) <= 2e-4 * max(1.0, abs(g)), (u, k, info[k], g)
        for tag, onet in (("pf", opf), ("vf", ovf)):
            for k, v in onet.items():
                key = "u%d/%s/%s" % (u, tag, k)
                if key in gold.files:
                    assert np.abs(v.numpy() - gold[key]).max() <= 2e-5, key


@pytest.mark.parametrize("name", list(TACT_CASES))
def test_fp32_restatement_determines_both_updates(name):
    """The precondition of the GPU tests' fp32 parameter bound (tests/wide_cases.py, "Seeds"): the fp32 restatement and the
    same restatement in float64 agree to ORACLE_F32_ERR_MAX on every parameter after each of the two updates."""
    case = TACT_CASES[name]
    runs = {}
    for dt in (torch.float32, torch.float64):
        pf, vf = _nets(case)
        opf = {k: v.clone().to(dt) for k, v in pf.state_dict().items()}
        ovf = util.share_encoder(opf, {k: v.clone().to(dt) for k, v in vf.state_dict().items()}, case["kind"])
        oracle = orc.PPOOracle(case["kind"], opf, ovf, {k: v.clone() for k, v in opf.items()}, case["S"])
        oracle.sync_target()
        t = lambda a: torch.tensor(a, dtype=torch.float32).to(dt)  # (the fp32 inputs both evaluations get)
        runs[dt] = []
        for u in range(2):
            b = util.make_batch(case, update=u)
            oracle.update(t(b["obs"]), t(b["acts"]), t(b["advs"]), t(b["estimate_returns"]), t(b["values"]), 1e-4, 1e-4)
            runs[dt].append({"pf/" + k: v.double().clone() for k, v in opf.items()} | {"vf/" + k: v.double().clone() for k, v in ovf.items()})
    for u in range(2):
        for k, v in runs[torch.float32][u].items():
            d = (v - runs[torch.float64][u][k]).abs().max().item()
            assert d <= ORACLE_F32_ERR_MAX, (u, k, d)
