"""Cases with more than 8 action dimensions (joint-space control: one action per motor, a1.NUM_MOTORS = 12 — the reference's
vision4leg/envs/locomotion_gym_env.py:195-214), shared by tests/golden/make_golden_wide.py, tests/test_wide_actions_cpu.py and
tests/test_gpu_wide_actions.py. Same fields as tests/util.CASES; kept apart from it because every parity test there runs over
all of util.CASES.

Why these shapes: A = 9 is the first width past the capacity-8 loss code, A = 12 the 12-motor robot, A = 16 fills the padded
head row (no zero column left); B = 22 leaves a ragged last 16-row tile.

Seeds. The GPU tests hold the engine's fp32 mode to 2e-5 on every parameter after two updates AGAINST THE FP32 ORACLE. That asks
of the oracle that its own fp32 rounding does not decide the update: a ReLU pre-activation that lies within fp32 summation
noise of zero for one sample lets two correct fp32 evaluations disagree by ~lr in a whole weight row after the next Adam step.
So a case's seed must pass a check that involves the oracle alone: after both updates, the fp32 oracle and the same oracle
evaluated in float64 agree to ORACLE_F32_ERR_MAX on every parameter (tests/test_wide_actions_cpu.py asserts it for every
case). Healthy cases measure 1e-7 .. 2.2e-7 there, a moved decision >= 1e-5. The seeds are 30 .. 37 in the order of the
table; where one does not pass, the first of seed + 10, + 20, ... that does. cnn_a12: seed 35 measures 1.14e-4 (one unit of
encoder.visual_projector, second update), seed 45 1.8e-7."""

ORACLE_F32_ERR_MAX = 1e-6  # a factor 20 under the GPU tests' fp32 parameter bound, a factor 5 over what a healthy case measures

WIDE_CASES = {
    "loco_a9": dict(kind="loco", S=84, A=9, seed=30, B=22, enc=[256, 256], head=[256, 256], layers=2, ff=256),
    "loco_a12": dict(kind="loco", S=84, A=12, seed=31, B=32, enc=[256, 256], head=[256, 256], layers=2, ff=256),
    "loco_a16": dict(kind="loco", S=84, A=16, seed=32, B=32, enc=[256, 256], head=[256, 256], layers=2, ff=256),
    "loco_tanh_a12": dict(kind="loco_tanh", S=84, A=12, seed=33, B=32, enc=[256, 256], head=[256, 256], layers=2, ff=256),
    "loco_vis_a12": dict(kind="loco_vis", S=0, A=12, seed=34, B=32, enc=[], head=[256, 256], layers=2, ff=256),
    "cnn_a12": dict(kind="cnn", S=93, A=12, seed=45, B=32, enc=[256, 256], head=[256, 256], visual_dim=256),
    "mlp_a12": dict(kind="mlp", S=93, A=12, seed=36, B=64, enc=[256, 256], head=[256, 256]),
    "mlp_tanh_a16": dict(kind="mlp_tanh", S=93, A=16, seed=37, B=64, enc=[256, 256], head=[256, 256]),
}

# The production shape of the update: from n = 512 on the trainer launches the loss with 16 waves per block (1024-thread statistics
# block, actor_loss_heads_kernel<T, 16, CAP>), below it with 4 — the cases above all take the small launch. One update only: at this
# batch size the fp32 oracle's own error after a second update (1.1e-6 .. 2.8e-6 at seeds 38, 48, 58, 68: longer sums, no moved
# decision) is over ORACLE_F32_ERR_MAX, after the first it is under it.
BIG_CASES = {
    "loco_a12_b512": dict(kind="loco", S=84, A=12, seed=38, B=512, enc=[256, 256], head=[256, 256], layers=2, ff=256, updates=1),
}
ALL_CASES = {**WIDE_CASES, **BIG_CASES}

# the two cases the unmodified reference was run on: tests/golden/ppo_<name>.npz
FIXTURE_CASES = ("loco_a12", "mlp_a12")
