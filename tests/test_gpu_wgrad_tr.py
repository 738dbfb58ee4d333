"""-m gpu: the conv weight-grads' MFMA operands built with transposed LDS reads (ds_read_b64_tr_b16; csrc/bwd.h, the address maps
in csrc/tr_maps.h) against the element-by-element gathers they replace (V4L_WGRAD_TR=0). Every pixel keeps its K slot and every
rounding point stays where it was, so each MFMA sees the same operand bits in the same order: every result must hold the same
bits. compute=f32 has no transposed path (the instruction is 16-bit only): the switch must change nothing there."""
import os

import numpy as np
import pytest
import torch

import util
from test_gpu_parity import _build

pytestmark = pytest.mark.gpu

SWITCHES = ("V4L_WGRAD_TR", "V4L_CONV_BWD_BLOCKS")


def _grads(case, mode, device, n, obs, w, tr, blocks):
    """Every parameter gradient of the value net through the module-level forward(train=True) / backward (fp32 saved activations:
    the A16 = false instantiations), with V4L_WGRAD_TR unset (tr) or 0 and `blocks` persistent conv-backward blocks."""
    for k in SWITCHES:
        os.environ.pop(k, None)
    if not tr:
        os.environ["V4L_WGRAD_TR"] = "0"
    if blocks is not None:
        os.environ["V4L_CONV_BWD_BLOCKS"] = str(blocks)
    try:
        _, vf = _build(case, mode, device)
        hip = vf.hip
        st, im, _ = hip.stage(obs.to(device))
        hip.forward(st, im, n, train=True)
        dout = torch.zeros(n, 16, dtype=torch.float32, device=device)
        dout[:, :1] = w.to(device)
        grads = torch.full((hip.total_params,), float("nan"), dtype=torch.float32, device=device)
        hip.backward(st, im, n, dout, grads)
        torch.cuda.synchronize()
        assert not torch.isnan(grads).any()
        return {k: hip.grad_view(grads, k).cpu().clone() for k in hip.param_names}
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)


def _same_bits(case, mode, device, n, blocks):
    case = dict(case, B=n)
    obs = torch.tensor(util.make_batch(case)["obs"], dtype=torch.float32)
    w = torch.tensor(np.random.RandomState(9).randn(n, 1), dtype=torch.float32)
    on = _grads(case, mode, device, n, obs, w, True, blocks)
    off = _grads(case, mode, device, n, obs, w, False, blocks)
    assert sum(v.dim() == 4 for v in on.values()) >= 3
    for k in on:
        assert torch.equal(on[k], off[k]), (k, (on[k] - off[k]).abs().max().item())


@pytest.mark.parametrize("mode", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("blocks", [None, 5, 1])
@pytest.mark.parametrize("name", ["loco_s93", "cnn_s93"])
def test_transposed_reads_same_bits(name, blocks, mode, device):
    """B = 64: one sample per block (default blocks), 13 / 12 samples per block (5 blocks: ragged) and all 64 on one block."""
    _same_bits(util.CASES[name], mode, device, util.CASES[name]["B"], blocks)


@pytest.mark.parametrize("mode", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", ["loco_s93", "cnn_s93"])
def test_transposed_reads_same_bits_tiny_batch(name, n, mode, device):
    """n = 1 and n = 3: fewer samples than anything else the suite runs, one sample per block."""
    _same_bits(util.CASES[name], mode, device, n, None)


@pytest.mark.parametrize("mode", ["f16", "bf16", "f32"])
def test_transposed_reads_same_bits_in_trainer_updates(mode, device, monkeypatch):
    """Two run_updates updates from stored log pi_old on loco_s93: the trainer's passes save c1 / c2 in the operand type (the
    A16 = true instantiations). Both gradient vectors, the 24-float records and both nets' parameters, bit for bit."""
    from vision4leg_amd.engine import HipTrainer
    from vision4leg_amd.torchrl.algo import PPO
    case = util.CASES["loco_s93"]
    B, U = case["B"], 2
    res = {}
    for arm in ("on", "off"):
        if arm == "off":
            monkeypatch.setenv("V4L_WGRAD_TR", "0")
        else:
            monkeypatch.delenv("V4L_WGRAD_TR", raising=False)
        pf, vf = _build(case, mode, device)

        class Coll: epoch_frames = B
        agent = PPO(pf=pf, vf=vf, plr=1e-4, vlr=1e-4, clip_para=0.2, opt_epochs=3, tau=0.95, entropy_coeff=0.005,
                    collector=Coll(), device=device, batch_size=B)
        agent.use_graph = False  # (the switch is read at every launch; a captured graph would keep the first arm's kernels)
        b = util.make_batch(case)
        t = lambda a: torch.tensor(a, dtype=torch.float32, device=device)
        net = pf.hip
        net.ensure_bound()
        st, im = net.alloc_rollout(B, device)
        net.ingest(t(b["obs"]), st, im)
        rs = np.random.RandomState(3)
        logp = t(-6.0 + 0.3 * rs.randn(B))
        ro = HipTrainer.rollout(st, im, t(b["acts"]), t(b["advs"]).reshape(-1), t(b["estimate_returns"]).reshape(-1),
                                t(b["values"]).reshape(-1), logp)
        rows = torch.stack([torch.from_numpy(rs.permutation(B).astype(np.int32)) for _ in range(U)]).to(device)
        agent.trainer.sync_target()
        snaps = []
        for u in range(U):
            stats = torch.zeros(1, 24, device=device)
            agent.run_updates(ro, rows[u:u + 1], stats)
            torch.cuda.synchronize()
            tr = agent.trainer
            snaps.append((stats.cpu().clone(), tr.g_pf.cpu().clone(), tr.g_vf.cpu().clone(),
                          {k: v.detach().cpu().clone() for k, v in pf.state_dict().items()},
                          {k: v.detach().cpu().clone() for k, v in vf.state_dict().items()}))
        res[arm] = snaps
    for u in range(U):
        (sa, gpa, gva, pa, va), (sb, gpb, gvb, pb, vb) = res["on"][u], res["off"][u]
        assert torch.isfinite(sa[0, :18]).all()
        assert torch.equal(gpa, gpb), (u, (gpa - gpb).abs().max().item())
        assert torch.equal(gva, gvb), (u, (gva - gvb).abs().max().item())
        assert torch.equal(sa.view(torch.int32), sb.view(torch.int32)), (u, sa, sb)
        for tag, a, b2 in (("pf", pa, pb), ("vf", va, vb)):
            for k in a:
                assert torch.equal(a[k], b2[k]), (u, tag, k)
