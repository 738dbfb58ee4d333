"""Cases of the state-MLP net with Tanh activations (activation_func=nn.Tanh: the commented switch of the reference's PPO
starters, starter/ppo_state.py:91), shared by tests/golden/make_golden_tact.py, tests/test_tact_cpu.py and
tests/test_gpu_tact.py. Same fields as tests/util.CASES; kept apart from it because every parity test there runs over all of
util.CASES. The kind suffix `_tact` is vision4leg_amd/recipes.py::build_nets' (stripped after `_tanh`).

The oracle package has no Tanh forward. `tact_forward` restates the reference's arithmetic for this net (Net.forward over an
MLPBase, nets.py:52-55, base.py:33-44, with activation_func = Tanh) on top of oracle.ppo_oracle.linear, and is registered at
import as the oracle's forward of the two kinds — a dict entry at run time — so that PPOOracle and the helpers of
tests/test_gpu_parity.py take these cases as they are. tests/golden/make_golden_tact.py pins it to the unmodified reference.

Why these shapes:
  mlp_tact       the shipped geometry (S = 93, 256-wide) with a fixture from the reference; the rollout step takes the one-block
                 kernel in the 16-bit modes and the per-sample kernel in f32
  mlp_tact_tanh  the same with a TanhNormal head: the per-sample kernel in the 16-bit modes too
  mlp_tact_rag   ragged row tile (B = 22), 32- and 16-wide column-tile launches (widths 64 / 72 -> Np 64 / 80; A = 12 -> Np 16),
                 the general rollout route, a wide action
  mlp_tact_b300  gemm_nt_deep (M >= 256) with a ragged tail (300 = 9 x 32 + 12)

Seeds are 40 .. 43 in the order of the table, held to tests/wide_cases.py's rule ("Seeds"): the fp32 restatement and the same
restatement in float64 agree to ORACLE_F32_ERR_MAX on every parameter after the updates the GPU test runs
(tests/test_tact_cpu.py asserts it for every case)."""
import torch

from oracle import ppo_oracle as orc

TACT_CASES = {
    "mlp_tact": dict(kind="mlp_tact", S=93, A=6, seed=40, B=64, enc=[256, 256], head=[256, 256]),
    "mlp_tact_tanh": dict(kind="mlp_tact_tanh", S=93, A=6, seed=43, B=64, enc=[256, 256], head=[256, 256]),
    "mlp_tact_rag": dict(kind="mlp_tact", S=45, A=12, seed=41, B=22, enc=[128, 64], head=[72]),
    "mlp_tact_b300": dict(kind="mlp_tact", S=93, A=6, seed=42, B=300, enc=[256, 256], head=[256, 256]),
}

# the case the unmodified reference was run on: tests/golden/ppo_mlp_tact.npz
FIXTURE_CASES = ("mlp_tact",)

SATURATION = 9.02  # |pre-activation| from which fp32 tanh is exactly +-1 (1 - tanh(9.02) = 2.9e-8 < 2^-25)


def tact_forward(p, x, S=None, mode="f32", taps=None):
    """Net.forward with a Tanh MLPBase trunk and Tanh append layers: tanh(linear) per hidden layer, then the last linear.
    The contraction groups are mlp_forward's ("proprio" for the base, "heads" for the append layers)."""
    ne = orc._count(p, "base.seq_fcs.%d.weight")
    nh = orc._count(p, "seq_append_fcs.%d.weight") - 1
    for i in range(ne):
        x = torch.tanh(orc.linear(x, p["base.seq_fcs.%d.weight" % (2 * i)], p["base.seq_fcs.%d.bias" % (2 * i)], mode, "proprio"))
        if taps is not None:
            taps["eh%d" % i] = x
    for i in range(nh):
        x = torch.tanh(orc.linear(x, p["seq_append_fcs.%d.weight" % (2 * i)], p["seq_append_fcs.%d.bias" % (2 * i)], mode, "heads"))
    return orc.linear(x, p["seq_append_fcs.%d.weight" % (2 * nh)], p["seq_append_fcs.%d.bias" % (2 * nh)], mode, "heads")


orc.FORWARDS["mlp_tact"] = tact_forward
orc.FORWARDS["mlp_tact_tanh"] = tact_forward  # (PPOOracle reads the `_tanh` suffix: TanhNormal head)
