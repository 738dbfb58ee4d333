"""Cases of the A2C update (the reference's torchrl/algo/on_policy/a2c.py) and its restatement, shared by
tests/golden/make_golden_a2c.py, tests/test_a2c_cpu.py and tests/test_gpu_a2c.py. Same fields as tests/util.CASES; kept apart
from it because every parity test there runs over all of util.CASES.

The nets are state-MLP pairs WITHOUT a common parameter (`build_nets` below: GaussianContPolicyBasicBias + networks.Net, each
with its own MLPBase). The reference's A2C evaluates vf(obs) before pf_optimizer.step() and backpropagates vf_loss after it
(a2c.py:76-85), so it raises on the pairs vision4leg_amd/recipes.py::build_nets wires (one base / encoder module in both nets).

`A2COracle` restates A2C.update (a2c.py:46-107) over name -> tensor parameter dicts on top of oracle.ppo_oracle — its
FORWARDS[kind](..., mode) for the nets (tests/tact_cases.py registers the Tanh ones), torch autograd for the gradients
(PPOOracle._grads: the f16 flavour's scaled backward), two torch.optim optimisers — the way tests/vmpo_cases.py extends the
oracle without editing it. It runs in the oracle's modes ("f32", "bf16", "f16") on fp32 tensors and, handed float64 tensors
with mode "f32", in float64. tests/golden/make_golden_a2c.py pins it to the unmodified reference.

Why these shapes (the smallest at which this code can still go wrong):
  a2c_mlp        S=93 A=6 B=64 [256,256]   the shipped geometry; fixture from the reference
  a2c_mlp_tanh   the same, tanh_action      TanhNormal log-prob next to the plain Normal's entropy; fixture from the reference
  a2c_mlp_odd    S=45 A=12 B=23 [128,64]/[72]  odd n, a partial wave in the loss block, the capacity-16 loss code
  a2c_mlp_a1     A=1 B=2                    std/std over two elements, v_pred/std over two rows
  a2c_mlp_tact   Tanh activations, B=64     nets built as tests/tact_cases.py builds them
  a2c_mlp_b1024  B=1024, one update         the full 1024-thread loss blocks (tests/wide_cases.py BIG_CASES: the fp32
                                            restatement's own error after a second update at this size)

Seeds: 60 .. 65 in the order of the table, held to tests/wide_cases.py's rule ("Seeds"): after the updates the GPU test runs,
the fp32 restatement and the float64 restatement agree to ORACLE_F32_ERR_MAX on every parameter (tests/test_a2c_cpu.py asserts
it for every case); where a seed does not pass, the first of seed + 10, + 20, ... that does."""
import numpy as np
import torch

from oracle import ppo_oracle as orc
import tact_cases  # noqa: F401  (registers the oracle's forward of the `mlp_tact` kinds)
from wide_cases import ORACLE_F32_ERR_MAX  # noqa: F401

A2C_CASES = {
    "a2c_mlp": dict(kind="mlp", S=93, A=6, seed=60, B=64, enc=[256, 256], head=[256, 256]),
    "a2c_mlp_tanh": dict(kind="mlp_tanh", S=93, A=6, seed=61, B=64, enc=[256, 256], head=[256, 256]),
    "a2c_mlp_odd": dict(kind="mlp", S=45, A=12, seed=62, B=23, enc=[128, 64], head=[72]),
    "a2c_mlp_a1": dict(kind="mlp", S=45, A=1, seed=63, B=2, enc=[128, 64], head=[72]),
    "a2c_mlp_tact": dict(kind="mlp_tact", S=93, A=6, seed=64, B=64, enc=[256, 256], head=[256, 256]),
    "a2c_mlp_b1024": dict(kind="mlp", S=93, A=6, seed=65, B=1024, enc=[256, 256], head=[256, 256], updates=1),
}

# the cases the unmodified reference was run on: tests/golden/<name>.npz
FIXTURE_CASES = ("a2c_mlp", "a2c_mlp_tanh")

LR = 1e-4            # plr = vlr of every test (the parameter bounds of tests/test_gpu_vmpo.py::test_two_updates are sized for it)
ENTROPY_COEFF = 0.005

# the 12 keys of A2C.update's info in the reference's order (a2c.py:89-105)
INFO_KEYS = ["Training/policy_loss", "Training/vf_loss", "v_pred/mean", "v_pred/std", "v_pred/max", "v_pred/min",
             "std/mean", "std/std", "std/max", "std/min", "ent", "log_prob"]

BATCH_KEYS = ("obs", "acts", "advs", "estimate_returns")


def updates_of(case):
    return case.get("updates", 2)


def build_nets(networks, policies, case):
    """pf / vf of a state-MLP case as starter/ppo_state.py builds them, each keeping the MLPBase its constructor made (no
    `vf.base = pf.base`). `networks` / `policies`: vision4leg_amd.torchrl's modules or the unmodified reference's."""
    kind = case["kind"]
    net = {"append_hidden_shapes": list(case["head"]), "base_type": networks.MLPBase, "hidden_shapes": list(case["enc"])}
    pol = {}
    if kind.endswith("_tanh"):
        pol["tanh_action"] = True
        kind = kind[:-5]
    if kind.endswith("_tact"):
        net["activation_func"] = torch.nn.Tanh
        kind = kind[:-5]
    assert kind == "mlp", case["kind"]
    pf = policies.GaussianContPolicyBasicBias(input_shape=case["S"], output_shape=case["A"], **net, **pol)
    vf = networks.Net(input_shape=(case["S"],), output_shape=1, **net)
    return pf, vf


def seeded_nets(networks, policies, case):
    torch.manual_seed(case["seed"])
    return build_nets(networks, policies, case)


class A2COracle(orc.PPOOracle):
    """A2C.update over name -> tensor dicts (pf and vf hold no common tensor). No target policy: PPOOracle's third dict is
    pf's own."""

    def __init__(self, kind, pf, vf, S, mode="f32", entropy_coeff=ENTROPY_COEFF, max_norm=0.5, optimizer_class=torch.optim.Adam,
                 optimizer_kwargs=None):
        super().__init__(kind, pf, vf, pf, S, mode, entropy_coeff=entropy_coeff, max_norm=max_norm)
        assert not {id(v) for v in pf.values()} & {id(v) for v in vf.values()}
        self.optimizer_class, self.optimizer_kwargs = optimizer_class, dict(optimizer_kwargs or {})
        self.pf_opt = self.vf_opt = None

    def _opts(self, lr_pf, lr_vf):
        if self.pf_opt is None:  # a2c.py:30-40
            self.pf_opt = self.optimizer_class([self.pf[k] for k in self.pf_keys], lr=lr_pf, eps=1e-5, **self.optimizer_kwargs)
            self.vf_opt = self.optimizer_class([self.vf[k] for k in self.vf_keys], lr=lr_vf, eps=1e-5, **self.optimizer_kwargs)
        for opt, lr in ((self.pf_opt, lr_pf), (self.vf_opt, lr_vf)):
            opt.param_groups[0]["lr"] = lr

    @staticmethod
    def _step(opt, tensors, grads):
        for p, g in zip(tensors, grads):
            p.grad = g.detach().clone()
        opt.step()
        for p in tensors:
            p.grad = None

    def losses(self, obs, acts, advs_raw, est_rets):
        """a2c.py:61-77. -> (policy_loss, vf_loss, policy head output [n, A], values [n, 1], the 12-key info)."""
        for k in self.pf_keys:
            self.pf[k].requires_grad_(True)
        for k in self.vf_keys:
            self.vf[k].requires_grad_(True)
        out = self.fwd({k: v for k, v in self.pf.items() if k != "logstd"}, obs, self.S, self.mode)
        mean, std, _ = orc.gaussian(out, self.pf["logstd"])
        log_probs, ent = orc.log_prob_entropy(mean, std, acts, self.tanh_action)
        advs = (advs_raw - advs_raw.mean()) / (advs_raw.std() + 1e-5)                    # a2c.py:68
        policy_loss = (-log_probs * advs).mean() - self.entropy_coeff * ent.mean()       # a2c.py:73-74
        values = self.fwd(self.vf, obs, self.S, self.mode)
        vf_loss = torch.nn.functional.mse_loss(values, est_rets)                         # a2c.py:76-77
        v, s = values.detach(), std.detach()
        info = {"Training/policy_loss": policy_loss.item(), "Training/vf_loss": vf_loss.item(),
                "v_pred/mean": v.mean().item(), "v_pred/std": v.std().item(), "v_pred/max": v.max().item(), "v_pred/min": v.min().item(),
                "std/mean": s.mean().item(), "std/std": s.std().item(), "std/max": s.max().item(), "std/min": s.min().item(),
                "ent": ent.mean().item(), "log_prob": log_probs.mean().item()}
        return policy_loss, vf_loss, out, values, info

    def _release(self):
        for k in self.pf_keys:
            self.pf[k].requires_grad_(False)
        for k in self.vf_keys:
            self.vf[k].requires_grad_(False)

    def loss_grads(self, obs, acts, advs, est_rets):
        """One loss evaluation, nothing stepped: d(policy_loss)/d(head output) [n, A], /d(logstd) [A], d(vf_loss)/d(values)
        [n, 1] and the info."""
        policy_loss, vf_loss, out, values, info = self.losses(obs, acts, advs, est_rets)
        dout, dls = torch.autograd.grad(policy_loss, [out, self.pf["logstd"]])
        dval, = torch.autograd.grad(vf_loss, [values])
        self._release()
        return dout, dls.reshape(-1), dval, info

    def update(self, obs, acts, advs, est_rets, lr_pf, lr_vf):
        """obs [B, D], acts [B, A], advs / est_rets [B, 1]. Returns the 12-key info (a2c.py:89-105)."""
        self._opts(lr_pf, lr_vf)
        self.step += 1
        n = obs.shape[0]
        policy_loss, vf_loss, _, _, info = self.losses(obs, acts, advs, est_rets)
        gp = self._grads(policy_loss, self.pf, self.pf_keys, n)
        gv = self._grads(vf_loss, self.vf, self.vf_keys, n)
        self.last_grads["pf"], self.last_grads["vf"] = dict(zip(self.pf_keys, gp)), dict(zip(self.vf_keys, gv))
        gp, gn_pf = orc.clip_grad_norm(gp, self.max_norm)                                # a2c.py:81
        self._step(self.pf_opt, [self.pf[k] for k in self.pf_keys], gp)
        gv, gn_vf = orc.clip_grad_norm(gv, self.max_norm)                                # a2c.py:86
        self._step(self.vf_opt, [self.vf[k] for k in self.vf_keys], gv)
        self.grad_norms = (gn_pf.item(), gn_vf.item())
        return info


def batch_tensors(case, update, dtype=torch.float32):
    """util.make_batch(case, update) as the restatement's arguments: the fp32 values the engine gets, in `dtype`."""
    import util
    b = util.make_batch(case, update=update)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float32)).to(dtype)
    return tuple(t(b[k]) for k in BATCH_KEYS)


def host_batch(case, update):
    import util
    b = util.make_batch(case, update=update)
    return {k: b[k] for k in BATCH_KEYS}


def oracle_of(pf_sd, vf_sd, case, mode="f32", dtype=torch.float32, **kw):
    """An A2COracle on copies of two state_dicts."""
    opf = {k: v.detach().cpu().clone().to(dtype) for k, v in pf_sd.items()}
    ovf = {k: v.detach().cpu().clone().to(dtype) for k, v in vf_sd.items()}
    return A2COracle(case["kind"], opf, ovf, case["S"], mode, **kw)


def fresh_oracle(case, mode="f32", dtype=torch.float32, init=None):
    """An A2COracle on the case's seeded initial parameters (init: (pf state_dict, vf state_dict) to start from instead)."""
    if init is None:
        import vision4leg_amd.torchrl.networks as networks
        import vision4leg_amd.torchrl.policies as policies
        pf, vf = seeded_nets(networks, policies, case)
        init = (pf.state_dict(), vf.state_dict())
    return oracle_of(init[0], init[1], case, mode, dtype)
