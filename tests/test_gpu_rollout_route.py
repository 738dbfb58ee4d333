"""Pins the kernel route of the rollout step (v4l_actor_step) for every net configuration the rollout tests cover.

The rollout parity tests compare outputs against tolerances, so a configuration that silently fell back to another route
would still pass them. Here one eager step runs under the library's profiler, and the phase|op|kernel labels it logged (in
first-seen order, with their call counts and FLOPs) and the answer of v4l_actor_split_supported must equal ROUTES, recorded
from the library. Labels do not carry template arguments, so the table pins the route family, not the kernel instance.

`python tests/test_gpu_rollout_route.py` prints the table as it stands (needs a GPU).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import util

CASE_NAMES = ["loco_s84", "cnn_s93", "mlp_s93", "loco_vis", "cnn_vis", "loco_tn", "loco_vis_tn", "loco_pe", "loco_vis_pe",
              "loco_max", "loco_vis_max", "loco_tanh", "mlp_tanh"]
MODES = ["f32", "bf16", "f16"]
E = 8


def _configs():
    out = [(name, mode, shared, False) for name in CASE_NAMES for mode in MODES for shared in (True, False)]
    return out + [("cnn_s93", mode, shared, True) for mode in MODES for shared in (True, False)]


def _key(name, mode, shared, dense_split):
    return "%s/%s/%s%s" % (name, mode, "shared" if shared else "own", "/dense_split" if dense_split else "")


def collect(name, mode, shared, dense_split, device):
    """-> (split_supported, ((label, calls, flops), ...)) of one eager step after a warm-up step."""
    from vision4leg_amd import engine
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    case = util.CASES[name]
    os.environ["V4L_COMPUTE"] = mode
    if dense_split:
        os.environ["V4L_ROLLOUT_DENSE_SPLIT"] = "1"
    else:
        os.environ.pop("V4L_ROLLOUT_DENSE_SPLIT", None)
    try:
        torch.manual_seed(case["seed"])
        pf, vf = util.build_nets(networks, policies, case)
        pf, vf = pf.to(device), vf.to(device)
        actor = engine.HipActor(pf.hip, vf.hip, E, shared_encoder=shared, graph=False)
        rs = np.random.RandomState(3)
        parts = [np.clip(rs.randn(E, case["S"]), -10, 10)]
        if case["kind"] != "mlp" and case["kind"] != "mlp_tanh":
            parts.append(np.clip(rs.randn(E, 4 * 64 * 64), -2.5, 2.8))
        obs = torch.tensor(np.concatenate(parts, 1), dtype=torch.float32, device=device)
        actor.step(obs)  # (packs the operand-type weights)
        return actor.split_supported(), profile_step(actor, obs)
    finally:
        os.environ.pop("V4L_ROLLOUT_DENSE_SPLIT", None)


def profile_step(actor, obs, **kw):
    """-> ((label, calls, flops), ...) of one eager actor.step(obs, **kw) under the library's profiler."""
    from vision4leg_amd import _lib
    torch.cuda.synchronize()
    L = _lib.lib()
    L.v4l_prof_enable(1)
    try:
        actor.step(obs, **kw)
        buf = C.create_string_buffer(1 << 20)
        L.v4l_prof_collect(buf, len(buf))
    finally:
        L.v4l_prof_enable(0)
    rows = []
    for line in buf.value.decode().splitlines():
        label, calls, _, flops = line.split("\t")
        rows.append((label, int(calls), flops))
    return tuple(rows)


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode,shared,dense_split", _configs(), ids=[_key(*c) for c in _configs()])
def test_rollout_step_route(name, mode, shared, dense_split, device):
    split, rows = collect(name, mode, shared, dense_split, device)
    want_split, want_rows = ROUTES[_key(name, mode, shared, dense_split)]
    assert split == want_split
    assert [r[:2] for r in rows] == [r[:2] for r in want_rows]
    assert rows == want_rows


# recorded with `python tests/test_gpu_rollout_route.py`: key -> (split_supported, ((phase|op|kernel, calls, flops), ...))
ROUTES = {
    'loco_s84/f32/shared': (False, (
        ('rollout|encoder|rollout_encoder', 1, '5.885133e+07'),
        ('rollout|layer|rollout_layers_head', 1, '5.903974e+07'),
    )),
    'loco_s84/f32/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|encoder|fused_encoder', 2, '1.210900e+08'),
        ('rollout|layer|wps_layer_stack_head', 2, '5.903974e+07'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'loco_s84/bf16/shared': (True, (
        ('rollout|encoder|rollout_encoder', 1, '5.885133e+07'),
        ('rollout|layer|rollout_layers_head', 1, '5.903974e+07'),
    )),
    'loco_s84/bf16/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|encoder|fused_encoder', 2, '1.210900e+08'),
        ('rollout|layer|wps_layer_stack_head', 2, '5.903974e+07'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'loco_s84/f16/shared': (True, (
        ('rollout|encoder|rollout_encoder', 1, '5.885133e+07'),
        ('rollout|layer|rollout_layers_head', 1, '5.903974e+07'),
    )),
    'loco_s84/f16/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|encoder|fused_encoder', 2, '1.210900e+08'),
        ('rollout|layer|wps_layer_stack_head', 2, '5.903974e+07'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'cnn_s93/f32/shared': (False, (
        ('rollout|step|rollout_cnn', 1, '1.344799e+08'),
    )),
    'cnn_s93/f32/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|encoder.base.seq_fcs.0.fwd|gemm_nt', 2, '7.618560e+05'),
        ('rollout|encoder.base.seq_fcs.2.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|conv1.fwd|gemm_nt', 2, '5.898240e+07'),
        ('rollout|conv2.fwd|gemm_nt', 2, '3.774874e+07'),
        ('rollout|conv3.fwd|gemm_nt', 2, '1.887437e+07'),
        ('rollout|dense.stack|dense_stack_fwd', 2, '1.470874e+07'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'cnn_s93/bf16/shared': (True, (
        ('rollout|encoder|rollout_encoder', 1, '5.937562e+07'),
        ('rollout|dense|rollout_dense', 1, '1.061683e+07'),
    )),
    'cnn_s93/bf16/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|encoder|fused_encoder', 2, '1.210900e+08'),
        ('rollout|dense.stack|dense_stack_fwd', 2, '1.470874e+07'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'cnn_s93/f16/shared': (True, (
        ('rollout|encoder|rollout_encoder', 1, '5.937562e+07'),
        ('rollout|dense|rollout_dense', 1, '1.061683e+07'),
    )),
    'cnn_s93/f16/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|encoder|fused_encoder', 2, '1.210900e+08'),
        ('rollout|dense.stack|dense_stack_fwd', 2, '1.470874e+07'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'mlp_s93/f32/shared': (False, (
        ('rollout|step|rollout_mlp', 1, '9.437184e+06'),
    )),
    'mlp_s93/f32/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|base.seq_fcs.0.fwd|gemm_nt', 2, '7.618560e+05'),
        ('rollout|base.seq_fcs.2.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|seq_append_fcs.0.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|seq_append_fcs.2.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|seq_append_fcs.4.fwd|gemm_nt', 2, '2.867200e+04'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'mlp_s93/bf16/shared': (False, (
        ('rollout|step|rollout_mlp', 1, '9.437184e+06'),
    )),
    'mlp_s93/bf16/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|base.seq_fcs.0.fwd|gemm_nt', 2, '7.618560e+05'),
        ('rollout|base.seq_fcs.2.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|seq_append_fcs.0.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|seq_append_fcs.2.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|seq_append_fcs.4.fwd|gemm_nt', 2, '2.867200e+04'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'mlp_s93/f16/shared': (False, (
        ('rollout|step|rollout_mlp', 1, '9.437184e+06'),
    )),
    'mlp_s93/f16/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|base.seq_fcs.0.fwd|gemm_nt', 2, '7.618560e+05'),
        ('rollout|base.seq_fcs.2.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|seq_append_fcs.0.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|seq_append_fcs.2.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|seq_append_fcs.4.fwd|gemm_nt', 2, '2.867200e+04'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'loco_vis/f32/shared': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|conv1.fwd|gemm_nt', 1, '2.949120e+07'),
        ('rollout|conv2.fwd|gemm_nt', 1, '1.887437e+07'),
        ('rollout|conv3.fwd|gemm_nt', 1, '9.437184e+06'),
        ('rollout|encoder.depth_up_conv.fwd|gemm_nt', 1, '1.048576e+06'),
        ('rollout|visual_append_layers.0.self_attn.fwd|gemm_nt', 2, '6.291456e+06'),
        ('rollout|attn|attn_fwd', 4, '2.097152e+06'),
        ('rollout|visual_append_layers.0.self_attn.out_proj.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|ln1|add_ln_fwd', 4, '0.000000e+00'),
        ('rollout|visual_append_layers.0.linear1.fwd|gemm_nt', 2, '8.388608e+06'),
        ('rollout|visual_append_layers.0.linear2.fwd|gemm_nt', 2, '8.388608e+06'),
        ('rollout|ln2|add_ln_fwd', 4, '0.000000e+00'),
        ('rollout|visual_append_layers.1.self_attn.fwd|gemm_nt', 2, '6.291456e+06'),
        ('rollout|visual_append_layers.1.self_attn.out_proj.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|visual_append_layers.1.linear1.fwd|gemm_nt', 2, '8.388608e+06'),
        ('rollout|visual_append_layers.1.linear2.fwd|gemm_nt', 2, '8.388608e+06'),
        ('rollout|pool|pool_fwd', 2, '0.000000e+00'),
        ('rollout|visual_seq_append_fcs.0.fwd|gemm_nt', 2, '5.242880e+05'),
        ('rollout|visual_seq_append_fcs.2.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|visual_seq_append_fcs.4.fwd|gemm_nt', 2, '2.867200e+04'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'loco_vis/f32/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|conv1.fwd|gemm_nt', 2, '5.898240e+07'),
        ('rollout|conv2.fwd|gemm_nt', 2, '3.774874e+07'),
        ('rollout|conv3.fwd|gemm_nt', 2, '1.887437e+07'),
        ('rollout|encoder.depth_up_conv.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|layer|wps_layer_stack_head', 2, '5.903974e+07'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'loco_vis/bf16/shared': (True, (
        ('rollout|encoder|rollout_encoder', 1, '5.885133e+07'),
        ('rollout|layer|rollout_layers_head', 1, '5.903974e+07'),
    )),
    'loco_vis/bf16/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|encoder|fused_encoder', 2, '1.210900e+08'),
        ('rollout|layer|wps_layer_stack_head', 2, '5.903974e+07'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'loco_vis/f16/shared': (True, (
        ('rollout|encoder|rollout_encoder', 1, '5.885133e+07'),
        ('rollout|layer|rollout_layers_head', 1, '5.903974e+07'),
    )),
    'loco_vis/f16/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|encoder|fused_encoder', 2, '1.210900e+08'),
        ('rollout|layer|wps_layer_stack_head', 2, '5.903974e+07'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'cnn_vis/f32/shared': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|conv1.fwd|gemm_nt', 1, '2.949120e+07'),
        ('rollout|conv2.fwd|gemm_nt', 1, '1.887437e+07'),
        ('rollout|conv3.fwd|gemm_nt', 1, '9.437184e+06'),
        ('rollout|seq_append_fcs.0.fwd|gemm_nt', 2, '8.388608e+06'),
        ('rollout|seq_append_fcs.2.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|seq_append_fcs.4.fwd|gemm_nt', 2, '2.867200e+04'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'cnn_vis/f32/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|conv1.fwd|gemm_nt', 2, '5.898240e+07'),
        ('rollout|conv2.fwd|gemm_nt', 2, '3.774874e+07'),
        ('rollout|conv3.fwd|gemm_nt', 2, '1.887437e+07'),
        ('rollout|dense.stack|dense_stack_fwd', 2, '1.051443e+07'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'cnn_vis/bf16/shared': (True, (
        ('rollout|encoder|rollout_encoder', 1, '5.780275e+07'),
        ('rollout|dense|rollout_dense', 1, '1.061683e+07'),
    )),
    'cnn_vis/bf16/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|encoder|fused_encoder', 2, '1.210900e+08'),
        ('rollout|dense.stack|dense_stack_fwd', 2, '1.051443e+07'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'cnn_vis/f16/shared': (True, (
        ('rollout|encoder|rollout_encoder', 1, '5.780275e+07'),
        ('rollout|dense|rollout_dense', 1, '1.061683e+07'),
    )),
    'cnn_vis/f16/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|encoder|fused_encoder', 2, '1.210900e+08'),
        ('rollout|dense.stack|dense_stack_fwd', 2, '1.051443e+07'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'loco_tn/f32/shared': (False, (
        ('rollout|encoder|rollout_encoder', 1, '5.885133e+07'),
        ('rollout|layer|rollout_layers_head', 1, '5.903974e+07'),
    )),
    'loco_tn/f32/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|encoder|fused_encoder', 2, '1.210900e+08'),
        ('rollout|token_ln|add_ln_fwd', 2, '0.000000e+00'),
        ('rollout|layer|wps_layer_stack_head', 2, '5.903974e+07'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'loco_tn/bf16/shared': (True, (
        ('rollout|encoder|rollout_encoder', 1, '5.885133e+07'),
        ('rollout|layer|rollout_layers_head', 1, '5.903974e+07'),
    )),
    'loco_tn/bf16/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|encoder|fused_encoder', 2, '1.210900e+08'),
        ('rollout|token_ln|add_ln_fwd', 2, '0.000000e+00'),
        ('rollout|layer|wps_layer_stack_head', 2, '5.903974e+07'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'loco_tn/f16/shared': (True, (
        ('rollout|encoder|rollout_encoder', 1, '5.885133e+07'),
        ('rollout|layer|rollout_layers_head', 1, '5.903974e+07'),
    )),
    'loco_tn/f16/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|encoder|fused_encoder', 2, '1.210900e+08'),
        ('rollout|token_ln|add_ln_fwd', 2, '0.000000e+00'),
        ('rollout|layer|wps_layer_stack_head', 2, '5.903974e+07'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'loco_vis_tn/f32/shared': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|conv1.fwd|gemm_nt', 1, '2.949120e+07'),
        ('rollout|conv2.fwd|gemm_nt', 1, '1.887437e+07'),
        ('rollout|conv3.fwd|gemm_nt', 1, '9.437184e+06'),
        ('rollout|encoder.depth_up_conv.fwd|gemm_nt', 1, '1.048576e+06'),
        ('rollout|token_ln|add_ln_fwd', 2, '0.000000e+00'),
        ('rollout|visual_append_layers.0.self_attn.fwd|gemm_nt', 2, '6.291456e+06'),
        ('rollout|attn|attn_fwd', 4, '2.097152e+06'),
        ('rollout|visual_append_layers.0.self_attn.out_proj.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|ln1|add_ln_fwd', 4, '0.000000e+00'),
        ('rollout|visual_append_layers.0.linear1.fwd|gemm_nt', 2, '8.388608e+06'),
        ('rollout|visual_append_layers.0.linear2.fwd|gemm_nt', 2, '8.388608e+06'),
        ('rollout|ln2|add_ln_fwd', 4, '0.000000e+00'),
        ('rollout|visual_append_layers.1.self_attn.fwd|gemm_nt', 2, '6.291456e+06'),
        ('rollout|visual_append_layers.1.self_attn.out_proj.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|visual_append_layers.1.linear1.fwd|gemm_nt', 2, '8.388608e+06'),
        ('rollout|visual_append_layers.1.linear2.fwd|gemm_nt', 2, '8.388608e+06'),
        ('rollout|pool|pool_fwd', 2, '0.000000e+00'),
        ('rollout|visual_seq_append_fcs.0.fwd|gemm_nt', 2, '5.242880e+05'),
        ('rollout|visual_seq_append_fcs.2.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|visual_seq_append_fcs.4.fwd|gemm_nt', 2, '2.867200e+04'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'loco_vis_tn/f32/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|conv1.fwd|gemm_nt', 2, '5.898240e+07'),
        ('rollout|conv2.fwd|gemm_nt', 2, '3.774874e+07'),
        ('rollout|conv3.fwd|gemm_nt', 2, '1.887437e+07'),
        ('rollout|encoder.depth_up_conv.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|token_ln|add_ln_fwd', 2, '0.000000e+00'),
        ('rollout|layer|wps_layer_stack_head', 2, '5.903974e+07'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'loco_vis_tn/bf16/shared': (True, (
        ('rollout|encoder|rollout_encoder', 1, '5.885133e+07'),
        ('rollout|layer|rollout_layers_head', 1, '5.903974e+07'),
    )),
    'loco_vis_tn/bf16/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|encoder|fused_encoder', 2, '1.210900e+08'),
        ('rollout|token_ln|add_ln_fwd', 2, '0.000000e+00'),
        ('rollout|layer|wps_layer_stack_head', 2, '5.903974e+07'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'loco_vis_tn/f16/shared': (True, (
        ('rollout|encoder|rollout_encoder', 1, '5.885133e+07'),
        ('rollout|layer|rollout_layers_head', 1, '5.903974e+07'),
    )),
    'loco_vis_tn/f16/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|encoder|fused_encoder', 2, '1.210900e+08'),
        ('rollout|token_ln|add_ln_fwd', 2, '0.000000e+00'),
        ('rollout|layer|wps_layer_stack_head', 2, '5.903974e+07'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'loco_pe/f32/shared': (False, (
        ('rollout|encoder|rollout_encoder', 1, '5.885133e+07'),
        ('rollout|layer|rollout_layers_head', 1, '5.903974e+07'),
    )),
    'loco_pe/f32/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|encoder|fused_encoder', 2, '1.210900e+08'),
        ('rollout|layer|wps_layer_stack', 2, '5.584486e+07'),
        ('rollout|final_ln|add_ln_fwd', 2, '0.000000e+00'),
        ('rollout|pool|pool_fwd', 2, '0.000000e+00'),
        ('rollout|visual_seq_append_fcs.0.fwd|gemm_nt', 2, '1.048576e+06'),
        ('rollout|visual_seq_append_fcs.2.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|visual_seq_append_fcs.4.fwd|gemm_nt', 2, '2.867200e+04'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'loco_pe/bf16/shared': (True, (
        ('rollout|encoder|rollout_encoder', 1, '5.885133e+07'),
        ('rollout|layer|rollout_layers_head', 1, '5.903974e+07'),
    )),
    'loco_pe/bf16/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|encoder|fused_encoder', 2, '1.210900e+08'),
        ('rollout|layer|wps_layer_stack', 2, '5.584486e+07'),
        ('rollout|final_ln|add_ln_fwd', 2, '0.000000e+00'),
        ('rollout|pool|pool_fwd', 2, '0.000000e+00'),
        ('rollout|visual_seq_append_fcs.0.fwd|gemm_nt', 2, '1.048576e+06'),
        ('rollout|visual_seq_append_fcs.2.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|visual_seq_append_fcs.4.fwd|gemm_nt', 2, '2.867200e+04'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'loco_pe/f16/shared': (True, (
        ('rollout|encoder|rollout_encoder', 1, '5.885133e+07'),
        ('rollout|layer|rollout_layers_head', 1, '5.903974e+07'),
    )),
    'loco_pe/f16/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|encoder|fused_encoder', 2, '1.210900e+08'),
        ('rollout|layer|wps_layer_stack', 2, '5.584486e+07'),
        ('rollout|final_ln|add_ln_fwd', 2, '0.000000e+00'),
        ('rollout|pool|pool_fwd', 2, '0.000000e+00'),
        ('rollout|visual_seq_append_fcs.0.fwd|gemm_nt', 2, '1.048576e+06'),
        ('rollout|visual_seq_append_fcs.2.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|visual_seq_append_fcs.4.fwd|gemm_nt', 2, '2.867200e+04'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'loco_vis_pe/f32/shared': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|conv1.fwd|gemm_nt', 1, '2.949120e+07'),
        ('rollout|conv2.fwd|gemm_nt', 1, '1.887437e+07'),
        ('rollout|conv3.fwd|gemm_nt', 1, '9.437184e+06'),
        ('rollout|encoder.depth_up_conv.fwd|gemm_nt', 1, '1.048576e+06'),
        ('rollout|visual_trans_encoder.layers.0.self_attn.fwd|gemm_nt', 2, '6.291456e+06'),
        ('rollout|attn|attn_fwd', 4, '2.097152e+06'),
        ('rollout|visual_trans_encoder.layers.0.self_attn.out_proj.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|ln1|add_ln_fwd', 4, '0.000000e+00'),
        ('rollout|visual_trans_encoder.layers.0.linear1.fwd|gemm_nt', 2, '8.388608e+06'),
        ('rollout|visual_trans_encoder.layers.0.linear2.fwd|gemm_nt', 2, '8.388608e+06'),
        ('rollout|ln2|add_ln_fwd', 4, '0.000000e+00'),
        ('rollout|visual_trans_encoder.layers.1.self_attn.fwd|gemm_nt', 2, '6.291456e+06'),
        ('rollout|visual_trans_encoder.layers.1.self_attn.out_proj.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|visual_trans_encoder.layers.1.linear1.fwd|gemm_nt', 2, '8.388608e+06'),
        ('rollout|visual_trans_encoder.layers.1.linear2.fwd|gemm_nt', 2, '8.388608e+06'),
        ('rollout|final_ln|add_ln_fwd', 2, '0.000000e+00'),
        ('rollout|pool|pool_fwd', 2, '0.000000e+00'),
        ('rollout|visual_seq_append_fcs.0.fwd|gemm_nt', 2, '5.242880e+05'),
        ('rollout|visual_seq_append_fcs.2.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|visual_seq_append_fcs.4.fwd|gemm_nt', 2, '2.867200e+04'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'loco_vis_pe/f32/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|conv1.fwd|gemm_nt', 2, '5.898240e+07'),
        ('rollout|conv2.fwd|gemm_nt', 2, '3.774874e+07'),
        ('rollout|conv3.fwd|gemm_nt', 2, '1.887437e+07'),
        ('rollout|encoder.depth_up_conv.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|layer|wps_layer_stack', 2, '5.584486e+07'),
        ('rollout|final_ln|add_ln_fwd', 2, '0.000000e+00'),
        ('rollout|pool|pool_fwd', 2, '0.000000e+00'),
        ('rollout|visual_seq_append_fcs.0.fwd|gemm_nt', 2, '5.242880e+05'),
        ('rollout|visual_seq_append_fcs.2.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|visual_seq_append_fcs.4.fwd|gemm_nt', 2, '2.867200e+04'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'loco_vis_pe/bf16/shared': (True, (
        ('rollout|encoder|rollout_encoder', 1, '5.885133e+07'),
        ('rollout|layer|rollout_layers_head', 1, '5.903974e+07'),
    )),
    'loco_vis_pe/bf16/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|encoder|fused_encoder', 2, '1.210900e+08'),
        ('rollout|layer|wps_layer_stack', 2, '5.584486e+07'),
        ('rollout|final_ln|add_ln_fwd', 2, '0.000000e+00'),
        ('rollout|pool|pool_fwd', 2, '0.000000e+00'),
        ('rollout|visual_seq_append_fcs.0.fwd|gemm_nt', 2, '5.242880e+05'),
        ('rollout|visual_seq_append_fcs.2.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|visual_seq_append_fcs.4.fwd|gemm_nt', 2, '2.867200e+04'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'loco_vis_pe/f16/shared': (True, (
        ('rollout|encoder|rollout_encoder', 1, '5.885133e+07'),
        ('rollout|layer|rollout_layers_head', 1, '5.903974e+07'),
    )),
    'loco_vis_pe/f16/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|encoder|fused_encoder', 2, '1.210900e+08'),
        ('rollout|layer|wps_layer_stack', 2, '5.584486e+07'),
        ('rollout|final_ln|add_ln_fwd', 2, '0.000000e+00'),
        ('rollout|pool|pool_fwd', 2, '0.000000e+00'),
        ('rollout|visual_seq_append_fcs.0.fwd|gemm_nt', 2, '5.242880e+05'),
        ('rollout|visual_seq_append_fcs.2.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|visual_seq_append_fcs.4.fwd|gemm_nt', 2, '2.867200e+04'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'loco_max/f32/shared': (False, (
        ('rollout|encoder|rollout_encoder', 1, '5.885133e+07'),
        ('rollout|layer|rollout_layers_head', 1, '5.903974e+07'),
    )),
    'loco_max/f32/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|encoder|fused_encoder', 2, '1.210900e+08'),
        ('rollout|layer|wps_layer_stack_head', 2, '5.903974e+07'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'loco_max/bf16/shared': (True, (
        ('rollout|encoder|rollout_encoder', 1, '5.885133e+07'),
        ('rollout|layer|rollout_layers_head', 1, '5.903974e+07'),
    )),
    'loco_max/bf16/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|encoder|fused_encoder', 2, '1.210900e+08'),
        ('rollout|layer|wps_layer_stack_head', 2, '5.903974e+07'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'loco_max/f16/shared': (True, (
        ('rollout|encoder|rollout_encoder', 1, '5.885133e+07'),
        ('rollout|layer|rollout_layers_head', 1, '5.903974e+07'),
    )),
    'loco_max/f16/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|encoder|fused_encoder', 2, '1.210900e+08'),
        ('rollout|layer|wps_layer_stack_head', 2, '5.903974e+07'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'loco_vis_max/f32/shared': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|conv1.fwd|gemm_nt', 1, '2.949120e+07'),
        ('rollout|conv2.fwd|gemm_nt', 1, '1.887437e+07'),
        ('rollout|conv3.fwd|gemm_nt', 1, '9.437184e+06'),
        ('rollout|encoder.depth_up_conv.fwd|gemm_nt', 1, '1.048576e+06'),
        ('rollout|visual_append_layers.0.self_attn.fwd|gemm_nt', 2, '6.291456e+06'),
        ('rollout|attn|attn_fwd', 4, '2.097152e+06'),
        ('rollout|visual_append_layers.0.self_attn.out_proj.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|ln1|add_ln_fwd', 4, '0.000000e+00'),
        ('rollout|visual_append_layers.0.linear1.fwd|gemm_nt', 2, '8.388608e+06'),
        ('rollout|visual_append_layers.0.linear2.fwd|gemm_nt', 2, '8.388608e+06'),
        ('rollout|ln2|add_ln_fwd', 4, '0.000000e+00'),
        ('rollout|visual_append_layers.1.self_attn.fwd|gemm_nt', 2, '6.291456e+06'),
        ('rollout|visual_append_layers.1.self_attn.out_proj.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|visual_append_layers.1.linear1.fwd|gemm_nt', 2, '8.388608e+06'),
        ('rollout|visual_append_layers.1.linear2.fwd|gemm_nt', 2, '8.388608e+06'),
        ('rollout|pool|pool_fwd', 2, '0.000000e+00'),
        ('rollout|visual_seq_append_fcs.0.fwd|gemm_nt', 2, '5.242880e+05'),
        ('rollout|visual_seq_append_fcs.2.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|visual_seq_append_fcs.4.fwd|gemm_nt', 2, '2.867200e+04'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'loco_vis_max/f32/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|conv1.fwd|gemm_nt', 2, '5.898240e+07'),
        ('rollout|conv2.fwd|gemm_nt', 2, '3.774874e+07'),
        ('rollout|conv3.fwd|gemm_nt', 2, '1.887437e+07'),
        ('rollout|encoder.depth_up_conv.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|layer|wps_layer_stack_head', 2, '5.903974e+07'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'loco_vis_max/bf16/shared': (True, (
        ('rollout|encoder|rollout_encoder', 1, '5.885133e+07'),
        ('rollout|layer|rollout_layers_head', 1, '5.903974e+07'),
    )),
    'loco_vis_max/bf16/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|encoder|fused_encoder', 2, '1.210900e+08'),
        ('rollout|layer|wps_layer_stack_head', 2, '5.903974e+07'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'loco_vis_max/f16/shared': (True, (
        ('rollout|encoder|rollout_encoder', 1, '5.885133e+07'),
        ('rollout|layer|rollout_layers_head', 1, '5.903974e+07'),
    )),
    'loco_vis_max/f16/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|encoder|fused_encoder', 2, '1.210900e+08'),
        ('rollout|layer|wps_layer_stack_head', 2, '5.903974e+07'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'loco_tanh/f32/shared': (False, (
        ('rollout|encoder|rollout_encoder', 1, '5.885133e+07'),
        ('rollout|layer|rollout_layers_head', 1, '5.903974e+07'),
    )),
    'loco_tanh/f32/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|encoder|fused_encoder', 2, '1.210900e+08'),
        ('rollout|layer|wps_layer_stack_head', 2, '5.903974e+07'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'loco_tanh/bf16/shared': (False, (
        ('rollout|encoder|rollout_encoder', 1, '5.885133e+07'),
        ('rollout|layer|rollout_layers_head', 1, '5.903974e+07'),
    )),
    'loco_tanh/bf16/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|encoder|fused_encoder', 2, '1.210900e+08'),
        ('rollout|layer|wps_layer_stack_head', 2, '5.903974e+07'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'loco_tanh/f16/shared': (False, (
        ('rollout|encoder|rollout_encoder', 1, '5.885133e+07'),
        ('rollout|layer|rollout_layers_head', 1, '5.903974e+07'),
    )),
    'loco_tanh/f16/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|encoder|fused_encoder', 2, '1.210900e+08'),
        ('rollout|layer|wps_layer_stack_head', 2, '5.903974e+07'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'mlp_tanh/f32/shared': (False, (
        ('rollout|step|rollout_mlp', 1, '9.437184e+06'),
    )),
    'mlp_tanh/f32/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|base.seq_fcs.0.fwd|gemm_nt', 2, '7.618560e+05'),
        ('rollout|base.seq_fcs.2.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|seq_append_fcs.0.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|seq_append_fcs.2.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|seq_append_fcs.4.fwd|gemm_nt', 2, '2.867200e+04'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'mlp_tanh/bf16/shared': (False, (
        ('rollout|step|rollout_mlp', 1, '9.437184e+06'),
    )),
    'mlp_tanh/bf16/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|base.seq_fcs.0.fwd|gemm_nt', 2, '7.618560e+05'),
        ('rollout|base.seq_fcs.2.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|seq_append_fcs.0.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|seq_append_fcs.2.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|seq_append_fcs.4.fwd|gemm_nt', 2, '2.867200e+04'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'mlp_tanh/f16/shared': (False, (
        ('rollout|step|rollout_mlp', 1, '9.437184e+06'),
    )),
    'mlp_tanh/f16/own': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|base.seq_fcs.0.fwd|gemm_nt', 2, '7.618560e+05'),
        ('rollout|base.seq_fcs.2.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|seq_append_fcs.0.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|seq_append_fcs.2.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|seq_append_fcs.4.fwd|gemm_nt', 2, '2.867200e+04'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'cnn_s93/f32/shared/dense_split': (False, (
        ('rollout|step|rollout_cnn', 1, '1.344799e+08'),
    )),
    'cnn_s93/f32/own/dense_split': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|encoder.base.seq_fcs.0.fwd|gemm_nt', 2, '7.618560e+05'),
        ('rollout|encoder.base.seq_fcs.2.fwd|gemm_nt', 2, '2.097152e+06'),
        ('rollout|conv1.fwd|gemm_nt', 2, '5.898240e+07'),
        ('rollout|conv2.fwd|gemm_nt', 2, '3.774874e+07'),
        ('rollout|conv3.fwd|gemm_nt', 2, '1.887437e+07'),
        ('rollout|dense.stack|dense_stack_fwd', 2, '1.470874e+07'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'cnn_s93/bf16/shared/dense_split': (True, (
        ('rollout|encoder|rollout_encoder', 1, '5.937562e+07'),
        ('rollout|dense|rollout_linear', 2, '8.388608e+06'),
        ('rollout|head|rollout_head', 1, '2.228224e+06'),
    )),
    'cnn_s93/bf16/own/dense_split': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|encoder|fused_encoder', 2, '1.210900e+08'),
        ('rollout|dense.stack|dense_stack_fwd', 2, '1.470874e+07'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
    'cnn_s93/f16/shared/dense_split': (True, (
        ('rollout|encoder|rollout_encoder', 1, '5.937562e+07'),
        ('rollout|dense|rollout_linear', 2, '8.388608e+06'),
        ('rollout|head|rollout_head', 1, '2.228224e+06'),
    )),
    'cnn_s93/f16/own/dense_split': (False, (
        ('rollout|ctl|act_begin', 1, '0.000000e+00'),
        ('rollout|ingest|ingest', 1, '0.000000e+00'),
        ('rollout|encoder|fused_encoder', 2, '1.210900e+08'),
        ('rollout|dense.stack|dense_stack_fwd', 2, '1.470874e+07'),
        ('rollout|sample|act_finish', 1, '0.000000e+00'),
    )),
}


if __name__ == "__main__":
    dev = torch.device("cuda:0")
    print("ROUTES = {")
    for cfg in _configs():
        split, rows = collect(*cfg, dev)
        print("    %r: (%r, (" % (_key(*cfg), split))
        for r in rows:
            print("        %r," % (r,))
        print("    )),")
    print("}")
    sys.stdout.flush()
