"""CPU suite (`-m "not gpu"`): policies with up to V4L_MAX_ACT = 16 action dimensions — the host-side part of the C ABI (plan,
limits, error texts), the Python shell's check, and the oracle against what the unmodified reference produced at A = 12
(tests/golden/make_golden_wide.py). The GPU tests (tests/test_gpu_wide_actions.py) compare the engine with this oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

import util
from oracle import ppo_oracle as orc
from wide_cases import ALL_CASES, FIXTURE_CASES, ORACLE_F32_ERR_MAX, WIDE_CASES


def _cfg(kind, out_dim):
    """The shipped geometry of each net kind (what the Python shell fills in for tests/util.CASES) with `out_dim` actions."""
    from vision4leg_amd import _lib
    c = _lib.NetCfg()
    c.kind, c.compute, c.out_dim, c.has_logstd = kind, _lib.V4L_F16, out_dim, 1
    c.state_dim, c.n_enc_hidden = 84, 2
    c.enc_hidden[0] = c.enc_hidden[1] = 256
    c.n_head_hidden = 2
    c.head_hidden[0] = c.head_hidden[1] = 256
    if kind != _lib.V4L_NET_MLP:
        c.in_channels, c.img_hw, c.visual_dim = 4, 64, 256
    if kind == _lib.V4L_NET_LOCO:
        c.token_dim, c.n_layers, c.ff_dim = 64, 2, 256
    return c


def _create(cfg):
    from vision4leg_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    rc = L.v4l_net_create(C.byref(cfg), C.byref(h))
    err = (L.v4l_last_error() or b"").decode()
    return rc, h, err


@pytest.mark.parametrize("out_dim", [9, 12, 16])
@pytest.mark.parametrize("kind", ["MLP", "CNN", "LOCO"])
def test_net_create_accepts_up_to_max_act(kind, out_dim):
    from vision4leg_amd import _lib
    L = _lib.lib()
    rc, h, err = _create(_cfg(getattr(_lib, "V4L_NET_" + kind), out_dim))
    assert rc == 0, err
    try:
        shapes = {}
        for i in range(L.v4l_net_num_params(h)):
            name, nd, shp, numel, off = C.c_char_p(), C.c_int(), (C.c_int64 * 4)(), C.c_int64(), C.c_int64()
            assert L.v4l_net_param_info(h, i, C.byref(name), C.byref(nd), shp, C.byref(numel), C.byref(off)) == 0
            shapes[name.value.decode()] = tuple(shp[:nd.value])
        assert shapes["logstd"] == (out_dim,)
        last = [k for k, s in shapes.items() if s == (out_dim, 256)]  # the last head layer: the only out_dim x 256 weight
        assert len(last) == 1 and shapes[last[0].replace(".weight", ".bias")] == (out_dim,)
    finally:
        L.v4l_net_destroy(h)


def test_limit_is_named_by_library_and_shell():
    from vision4leg_amd import _lib
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    assert _lib.V4L_MAX_ACT == 16 == _lib.V4L_OUT_LD
    hdr = open(util.ROOT + "/include/v4l_hip.h").read()
    assert "#define V4L_MAX_ACT 16" in hdr
    for kind in (_lib.V4L_NET_MLP, _lib.V4L_NET_CNN, _lib.V4L_NET_LOCO):
        rc, h, err = _create(_cfg(kind, 17))
        assert rc != 0 and not h.value
        assert "out_dim" in err and "16" in err and "V4L_MAX_ACT" in err and "17" in err, err
    rc, _, err = _create(_cfg(_lib.V4L_NET_MLP, 0))
    assert rc != 0 and "out_dim" in err
    # the Python shell refuses before the library is called (the style of the other option checks)
    for name in ("loco_a12", "mlp_a12", "cnn_a12", "loco_vis_a12"):
        pf, vf = util.build_nets(networks, policies, dict(WIDE_CASES[name], A=17))
        with pytest.raises(NotImplementedError, match="at most 16 action dimensions"):
            pf.hip
        assert vf.hip.out_dim == 1
    pf, _ = util.build_nets(networks, policies, dict(WIDE_CASES["mlp_a12"], A=16))
    assert pf.hip.out_dim == 16


@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_plan_matches_reference_state_dict_at_a12(name):
    """The library's parameter table (names, shapes, in order of the state_dict) against the reference's own state_dict as
    the fixture recorded it."""
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    case, gold = WIDE_CASES[name], util.load_golden("ppo_" + name)
    torch.manual_seed(0)
    pf, vf = util.build_nets(networks, policies, case)
    for tag, net in (("pf", pf), ("vf", vf)):
        want = {f[len("shape_%s/" % tag):]: tuple(int(x) for x in gold[f]) for f in gold.files if f.startswith("shape_%s/" % tag)}
        hip = net.hip
        assert sorted(hip.param_names) == sorted(want), (name, tag)
        assert dict(zip(hip.param_names, hip.param_shapes)) == want, (name, tag)
        assert hip.total_params == sum(int(np.prod(s)) for s in want.values())
    assert dict(zip(pf.hip.param_names, pf.hip.param_shapes))["logstd"] == (12,)


@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_oracle_matches_reference_golden_at_a12(name):
    """tests/test_cpu.py::test_oracle_matches_reference_golden's statements and tolerances (those of loco_s84 / mlp_s93), on the
    A = 12 fixtures — and on BOTH recorded updates, since the GPU tests lean on the oracle for the second one too."""
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    case, gold = WIDE_CASES[name], util.load_golden("ppo_" + name)
    torch.manual_seed(case["seed"])
    pf, vf = util.build_nets(networks, policies, case)
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
    with torch.no_grad():
        om = orc.FORWARDS[case["kind"]]({k: v for k, v in opf.items() if k != "logstd"}, t(b["obs"]), case["S"])
        ov = orc.FORWARDS[case["kind"]](ovf, t(b["obs"]), case["S"])
    assert tuple(om.shape) == (case["B"], 12)
    assert util.rel_err(om, gold["fwd_mean"]) < 2e-5 and util.rel_err(ov, gold["fwd_value"]) < 2e-5
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


@pytest.mark.parametrize("name", list(ALL_CASES))
def test_fp32_oracle_determines_both_updates(name):
    """The precondition of the GPU tests' fp32 parameter bound (tests/wide_cases.py, "Seeds"): on this case's seeded inputs the
    fp32 oracle's own rounding error — its distance to the same oracle evaluated in float64 — is far below that bound on every
    parameter after each of the updates the GPU test runs (two; one for the big-batch case). No ReLU / clip decision of the reference hangs on fp32 summation order."""
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    case = ALL_CASES[name]
    runs = {}
    for dt in (torch.float32, torch.float64):
        torch.manual_seed(case["seed"])
        pf, vf = util.build_nets(networks, policies, case)
        opf = {k: v.clone().to(dt) for k, v in pf.state_dict().items()}
        ovf = util.share_encoder(opf, {k: v.clone().to(dt) for k, v in vf.state_dict().items()}, case["kind"])
        oracle = orc.PPOOracle(case["kind"], opf, ovf, {k: v.clone() for k, v in opf.items()}, case["S"])
        oracle.sync_target()
        t = lambda a: torch.tensor(a, dtype=torch.float32).to(dt)  # (the fp32 inputs both evaluations get)
        runs[dt] = []
        for u in range(case.get("updates", 2)):
            b = util.make_batch(case, update=u)
            oracle.update(t(b["obs"]), t(b["acts"]), t(b["advs"]), t(b["estimate_returns"]), t(b["values"]), 1e-4, 1e-4)
            runs[dt].append({"pf/" + k: v.double().clone() for k, v in opf.items()} | {"vf/" + k: v.double().clone() for k, v in ovf.items()})
    for u in range(case.get("updates", 2)):
        for k, v in runs[torch.float32][u].items():
            d = (v - runs[torch.float64][u][k]).abs().max().item()
            assert d <= ORACLE_F32_ERR_MAX, (u, k, d)
