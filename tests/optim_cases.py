"""Weight decay on the HIP engine (PPO(optimizer_class=...)): the float64 restatement of torch's three Adam step variants and the
settings the optimiser tests share — tests/test_optim_cpu.py, tests/test_gpu_optim.py, tests/golden/make_golden_optim.py.

The restatement (`adam_step`, in oracle.ppo_oracle.adam_step's signature so that a test can put it in that function's place with
monkeypatch; `Adam`, ppo_ref64.Adam with the two decay modes) follows torch/optim/adam.py::_single_tensor_adam:

  none       m.lerp_(g, 1 - b1); v = b2 v + (1 - b2) g g; p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps)
  coupled    Adam(weight_decay=wd):  g <- g + wd p  first (adam.py:429), g being the gradient clip_grad_norm_ already scaled
  decoupled  AdamW:                  p <- p (1 - lr wd)  first (adam.py:419), then the plain step

tests/test_optim_cpu.py pins it to real torch.optim.Adam / AdamW in float64.

The isolated kernel test (tests/test_gpu_optim.py::test_clip_adam_decay_steps_vs_float64) is
tests/test_gpu_loss_adam.py::test_clip_adam_200_steps_vs_float64 with decay: that test's net (state MLP, A = 7: segments of 7 and 1
elements, an odd total), n = 4, its gradient generator, its three norm regimes and its learning rates, ISO_STEPS steps. `FlatWD` is that test's
rounding-bound model (`_Flat`) with the one fp32 rounding a decay mode adds:

  decoupled  p' = fl(p f), f = fl(1 - lr wd): the product's rounding and f's own are each <= EPS32 |p| (f <= 1); the model charges
             a rounding of a parameter 4 EPS32 |p| (its term for the final store), so one more 4 EPS32 |p| per step covers both.
             The bound accumulated so far shrinks by f <= 1: kept as it is.
  coupled    g' = fl(coef g + wd p), one fused rounding: <= EPS32 |g'|, |g'| <= coef |g| + wd |p|. The model's moment terms
             8 EPS32 (|m| + |g|) and 8 EPS32 (|v| + g^2) are taken with |g'| in |g|'s place; what is new is that g' inherits the
             parameter's own error: e_g = wd e_p + 4 EPS32 wd |p| (the second term: wd itself is rounded to fp32, and the
             product inside the fma is exact). It enters m as (1 - b1) e_g and v as (1 - b2) 2 |g'| e_g.
"""
import math

import numpy as np
import torch

import ppo_ref64 as ref

EPS = ref.EPS32
MODES_WD = ("coupled", "decoupled")
# The isolated test's decay settings (mode, wd). They are chosen from the float64 restatement alone, so that the test can tell a
# kernel with decay from one without (tests/test_optim_cpu.py::test_the_decay_is_far_above_the_isolated_tests_gate: at every
# compared step >= 90 % of every tensor is >= 50 gates away from the decay-free run). The gate is dominated by the model's bound
# on the Adam update, ~2e-4 lr in the first steps whatever |p| is, while decay moves an element by lr wd |p| per step, and the
# heads' last layers start at |p| ~ 1.5e-3. Measured smallest per-tensor share at 50 gates over steps 31 .. 41:
#   decoupled  wd 0.01, 0.1, 1: 0.0 (wd = 0.01 cannot pass anywhere: lr wd / (8 EPS32) = 24 gates at most); 5: 0.85; 10: 0.91;
#              20: 0.97; 30: 0.98
#   coupled    Adam normalises the step, so L2 decay shows as a turned direction, not as a size: 0.005: 0.83; 0.01: 0.91;
#              0.02: 0.94; 0.03: 0.92; 0.05: 0.87; 0.1: 0.74 (0.90 .. 0.94 over steps 8 .. 20, then the runs drift together again
#              in the shared encoder); 1 and 10: 0.0 (the small tensors collapse to zero with and without the gradient)
# Ordinary magnitudes (0.05, 0.1; 100 at lr 1e-4) are what the other tests of tests/test_gpu_optim.py run.
WDS = {"coupled": (0.01, 0.02), "decoupled": (10.0, 20.0)}
SETTINGS = [(m, wd) for m in MODES_WD for wd in WDS[m]]

# ---- the isolated test's settings (tests/test_gpu_loss_adam.py::test_clip_adam_200_steps_vs_float64's)
ISO_CASE = dict(kind="mlp", S=93, A=7, seed=57, B=64, enc=[256, 256], head=[256, 256])
ISO_STEPS = 42   # three periods of the learning-rate switch (14), four and a half of the regime cycle (9), four steps with 1e-20 / 1e18
#                  elements; the float64 mirror costs 0.14 s per step on the host, so 200 steps would be half a minute per case
ISO_SEED = 123
ISO_ZERO = "seq_append_fcs.2.bias"   # its first 7 elements get a zero gradient (as in the decay-free test) and start at zero, so
#                                      that no decay term moves them either: m = v = 0 and p = 0 throughout
REGIMES = ["big", "near", "small"]
SIGNAL = 50.0    # the decay must move a parameter by this many gates (tests/test_optim_cpu.py), on SIGNAL_SHARE of a tensor
SIGNAL_SHARE = 0.9


def iso_lrs(k):
    return (3e-4, 1e-3) if (k // 7) % 2 == 0 else (2e-3, 5e-5)


def iso_compared(k):
    """The last eleven steps. Earlier ones cannot separate decay from no decay by 50 gates: after one step the decoupled move is
    lr wd |p| against a gate of ~2e-4 lr, and the coupled runs differ only where sign(g) != sign(p), on half of the elements."""
    return k >= ISO_STEPS - 11


def iso_grads(rs, k, n_pf, n_vf, zero_off):
    """The gradients of step k exactly as the decay-free test draws them (same generator calls in the same order)."""
    import test_gpu_loss_adam as la
    gp = la._grads(rs, n_pf, REGIMES[(k // 3) % 3], k % 10 == 4)
    gv = la._grads(rs, n_vf, REGIMES[(k // 3 + 1) % 3], k % 10 == 9)
    gp[zero_off:zero_off + 7] = 0.0
    return gp.astype(np.float32), gv.astype(np.float32)


# ---- the restatement
def adam_step(params, grads, state, lr, step, betas=(0.9, 0.999), eps=1e-5, weight_decay=0.0, decoupled=False):
    """oracle.ppo_oracle.adam_step with torch's two kinds of weight decay, in the tensors' own dtype."""
    b1, b2 = betas
    step_size = lr / (1 - b1 ** step)
    bc2_sqrt = (1 - b2 ** step) ** 0.5
    with torch.no_grad():
        for p, g, (m, v) in zip(params, grads, state):
            if weight_decay != 0:
                if decoupled:
                    p.mul_(1 - lr * weight_decay)
                else:
                    g = g.add(p, alpha=weight_decay)
            m.lerp_(g, 1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            p.addcdiv_(m, (v.sqrt() / bc2_sqrt).add_(eps), value=-step_size)


def oracle_adam_step(weight_decay, decoupled):
    """-> a function to put in oracle.ppo_oracle.adam_step's place (monkeypatch.setattr): PPOOracle then steps with decay."""
    def step(params, grads, state, lr, step, betas=(0.9, 0.999), eps=1e-5):
        return adam_step(params, grads, state, lr, step, betas, eps, weight_decay, decoupled)
    return step


class Adam(ref.Adam):
    """ppo_ref64.Adam (clip_grad_norm_ + Adam over float64 tensors, own step count, skip) with weight decay."""

    def __init__(self, params, weight_decay=0.0, decoupled=False, **kw):
        super().__init__(params, **kw)
        self.weight_decay, self.decoupled = weight_decay, decoupled

    def step(self, grads, lr, skip=False):
        grads, norm = ref.clip_grad_norm([ref._d(g) for g in grads], self.max_norm)  # the norm never holds a decay term
        if skip:
            return norm
        self.steps += 1
        adam_step(self.params, grads, list(zip(self.m, self.v)), lr, self.steps, self.betas, self.eps, self.weight_decay,
                  self.decoupled)
        return norm


# ---- the isolated test's float64 mirror and gate
class FlatWD:
    """tests/test_gpu_loss_adam.py::_Flat with decay (module docstring): the float64 mirror of one optimiser's parameter set and
    the first-order fp32 error bounds of parameters and moments."""

    def __init__(self, hip, tensors, ep_store, weight_decay, decoupled):
        self.hip, self.t = hip, tensors
        self.wd, self.decoupled = weight_decay, decoupled
        self.opt = Adam(tensors, weight_decay, decoupled)
        self.em = [torch.zeros_like(p) for p in tensors]
        self.ev = [torch.zeros_like(p) for p in tensors]
        self.ep_store = ep_store
        for p in tensors:
            ep_store.setdefault(id(p), torch.zeros_like(p))

    @property
    def ep(self):
        return [self.ep_store[id(p)] for p in self.t]

    def split(self, flat):
        return [flat[o:o + p.numel()].view(p.shape) for o, p in zip(self.hip.grad_offsets, self.t)]

    def step(self, g_flat, lr, skip=False):
        gs = self.split(g_flat.double())
        before = [p.abs().clone() for p in self.t]
        norm = self.opt.step(gs, lr, skip)
        if skip:
            return norm
        coef = min(self.opt.max_norm / (norm + 1e-6), 1.0)
        b1, b2 = self.opt.betas
        k = self.opt.steps
        bc2 = np.sqrt(1 - b2 ** k)
        coupled = self.wd != 0 and not self.decoupled
        for i, (g, m, v, p) in enumerate(zip(gs, self.opt.m, self.opt.v, self.t)):
            gr = g.abs() * coef
            e_g = 0.0
            if coupled:
                gr = gr + self.wd * before[i]
                e_g = self.wd * self.ep_store[id(p)] + 4 * EPS * self.wd * before[i]
            self.em[i] = b1 * self.em[i] + 8 * EPS * (m.abs() + gr) + (1 - b1) * e_g
            self.ev[i] = b2 * self.ev[i] + 8 * EPS * (v.abs() + gr * gr) + (1 - b2) * 2 * gr * e_g
            den = v.sqrt() / bc2 + self.opt.eps
            e_den = torch.minimum(0.5 * self.ev[i] / v.sqrt().clamp_min(1e-300) / bc2, den)
            e_upd = lr / (1 - b1 ** k) * (self.em[i] + m.abs() * (e_den / den + 8 * EPS)) / den
            self.ep_store[id(p)] += 4 * EPS * p.abs() + e_upd
            if self.wd != 0 and self.decoupled:
                self.ep_store[id(p)] += 4 * EPS * before[i]
        return norm


def iso_mirrors(pf_hip, vf_hip, pf_tensors, vf_tensors, weight_decay, decoupled):
    """pf_tensors / vf_tensors: {name: float64 tensor}, the SAME tensor object under both for a parameter both nets own."""
    store = {}
    P = FlatWD(pf_hip, [pf_tensors[k] for k in pf_hip.param_names], store, weight_decay, decoupled)
    V = FlatWD(vf_hip, [vf_tensors[k] for k in vf_hip.param_names], store, weight_decay, decoupled)
    return P, V


def iso_cpu_nets():
    """The isolated test's nets built on the CPU (plan and parameters; no GPU work), ISO_ZERO set to zero."""
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    import util
    torch.manual_seed(ISO_CASE["seed"])
    pf, vf = util.build_nets(networks, policies, ISO_CASE)
    with torch.no_grad():
        pf.state_dict(keep_vars=True)[ISO_ZERO].view(-1)[:7].zero_()
    return pf, vf


def f64_params(pf, vf):
    """-> ({name: float64 copy} for pf, the same for vf), one copy per parameter TENSOR (shared ones are shared)."""
    memo = {}

    def f64(t):
        if id(t) not in memo:
            memo[id(t)] = t.detach().double().cpu().clone()
        return memo[id(t)]
    psd, vsd = pf.state_dict(keep_vars=True), vf.state_dict(keep_vars=True)
    return {k: f64(psd[k]) for k in pf.hip.param_names}, {k: f64(vsd[k]) for k in vf.hip.param_names}


# ---- whole-update fixtures (tests/golden/make_golden_optim.py writes them, tests/test_gpu_optim.py reads them)
GOLDEN_LR = 1e-4   # the parity tests' learning rate: their parameter tolerances (2.2e-4 (u + 1) in the 16-bit modes) are 2.2 lr
GOLDEN_WD = {"decoupled": 100.0, "coupled": 1.0}   # why these: make_golden_optim.py's docstring
GOLDEN_CASES = ("mlp_s93", "loco_s84")


def golden_name(case, mode_wd):
    return "ppo_optim_%s_%s" % (case, mode_wd)


def bound_50_steps(n_steps):
    """How far the restatement may sit from torch in float64 after n_steps: both do the same ~12 float64 operations per element
    and step in another order (x * (1 / a) against x / a, lerp's two forms), so each step adds at most 16 roundings of 2^-53
    relative to the magnitudes involved, and an Adam step is Lipschitz-1 in its state up to the factor 1 / (1 - b1) = 10 by which
    a moment error is held: 16 * 10 * n_steps * 2^-53."""
    return 160 * n_steps * 2.0 ** -53
