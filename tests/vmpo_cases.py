"""Cases of the V-MPO update (the reference's torchrl/algo/on_policy/v_mpo.py) and its restatement, shared by
tests/golden/make_golden_vmpo.py, tests/test_vmpo_cpu.py and tests/test_gpu_vmpo.py. Same fields as tests/util.CASES; kept apart
from it because every parity test there runs over all of util.CASES.

`VMPOOracle` restates VMPO.update (v_mpo.py:58-184) over name -> tensor parameter dicts on top of oracle.ppo_oracle — its
FORWARDS[kind](..., mode) for the nets, torch autograd for the gradients (PPOOracle._grads: the f16 flavour's scaled backward),
torch.optim.Adam for the three optimisers — the way tests/tact_cases.py extends the oracle without editing it. It runs in the
oracle's modes ("f32", "bf16", "f16") on fp32 tensors and, handed float64 tensors with mode "f32", in float64.
tests/golden/make_golden_vmpo.py pins it to the unmodified reference.

Why these shapes (B rows -> m = ceil(B / 2) rows in the policy's pass):
  vmpo_mlp        64 -> 32    the shipped state-MLP geometry; fixture from the reference
  vmpo_mlp_odd    23 -> 12    odd n, a partial wave in the loss block, A = 12: the capacity-16 loss code
  vmpo_mlp_tanh   64 -> 32    TanhNormal log-prob next to the plain Normals' KL
  vmpo_loco       32 -> 16    the LocoTransformer's three-launch wave-per-sample route on 16 rows; fixture from the reference
  vmpo_cnn        32 -> 16    the NatureCNN net's dense stack with one row tile
  vmpo_mlp_b1024  1024 -> 512 the 1024-thread loss block, the selection over four blocks; one update (tests/wide_cases.py
                              BIG_CASES: the fp32 restatement's own error after a second update at this size)

Seeds: 50 .. 55 in the order of the table, held to tests/wide_cases.py's rule ("Seeds") — after the updates the GPU test runs,
the fp32 restatement and the float64 restatement agree to ORACLE_F32_ERR_MAX on every parameter and on eta and alpha — and to
V-MPO's own: the m-th and the (m + 1)-th largest normalised advantage of every update differ by more than TIE_GAP_MIN, so no
case sits on the selection's boundary. tests/test_vmpo_cpu.py asserts both for every case; where a seed does not pass, the first
of seed + 10, + 20, ... that does."""
import numpy as np
import torch

from oracle import ppo_oracle as orc
from wide_cases import ORACLE_F32_ERR_MAX  # noqa: F401

TIE_GAP_MIN = 1e-6

VMPO_CASES = {
    "vmpo_mlp": dict(kind="mlp", S=93, A=6, seed=50, B=64, enc=[256, 256], head=[256, 256]),
    "vmpo_mlp_odd": dict(kind="mlp", S=45, A=12, seed=51, B=23, enc=[128, 64], head=[72]),
    "vmpo_mlp_tanh": dict(kind="mlp_tanh", S=93, A=6, seed=52, B=64, enc=[256, 256], head=[256, 256]),
    "vmpo_loco": dict(kind="loco", S=84, A=6, seed=53, B=32, enc=[256, 256], head=[256, 256], layers=2, ff=256),
    "vmpo_cnn": dict(kind="cnn", S=93, A=6, seed=54, B=32, enc=[256, 256], head=[256, 256], visual_dim=256),
    "vmpo_mlp_b1024": dict(kind="mlp", S=93, A=6, seed=55, B=1024, enc=[256, 256], head=[256, 256], updates=1),
}

# the cases the unmodified reference was run on: tests/golden/<name>.npz
FIXTURE_CASES = ("vmpo_mlp", "vmpo_loco")

LR = 1e-4  # plr = vlr of every test (the parameter bounds of tests/test_gpu_parity.py::test_ppo_update are sized for it)

# the 19 keys of VMPO.update's info in the reference's order (v_mpo.py:119-134, 154-155, 173-176)
INFO_KEYS = [
    "advs/mean", "advs/std", "advs/max", "advs/min", "Training/vf_loss", "grad_norm/vf",
    "Training/policy_loss", "Training/alpha_loss", "Training/alpha", "Training/eta",
    "logprob/mean", "logprob/std", "logprob/max", "logprob/min", "KL/mean", "KL/std", "KL/max", "KL/min", "grad_norm/pf",
]


def updates_of(case):
    return case.get("updates", 2)


def tie_gap(advs):
    """The distance between the m-th and the (m + 1)-th largest normalised advantage of a minibatch (fp32, v_mpo.py:179)."""
    a = torch.as_tensor(advs, dtype=torch.float32).reshape(-1)
    a = (a - a.mean()) / (a.std() + 1e-5)
    s = torch.sort(a, descending=True)[0]
    m = (a.numel() + 1) // 2
    return float(s[m - 1] - s[m]) if m < a.numel() else float("inf")


class VMPOOracle(orc.PPOOracle):
    """VMPO.update over name -> tensor dicts (shared encoder entries are the same tensor objects in pf and vf, as for
    PPOOracle). dtype of eta / alpha follows the parameters'."""

    def __init__(self, kind, pf, vf, target_pf, S, mode="f32", eta_eps=0.02, alpha_eps=0.1, max_norm=0.5,
                 optimizer_class=torch.optim.Adam):
        super().__init__(kind, pf, vf, target_pf, S, mode, max_norm=max_norm)
        dt = pf["logstd"].dtype
        self.eta_eps, self.alpha_eps = eta_eps, alpha_eps
        self.eta = torch.tensor([1.0], dtype=dt).requires_grad_()        # v_mpo.py:28
        self.alpha = torch.tensor([0.1], dtype=dt).requires_grad_()      # v_mpo.py:32
        self.optimizer_class = optimizer_class
        self.pf_opt = self.vf_opt = self.param_opt = None

    def _opts(self, lr_pf, lr_vf):
        if self.pf_opt is None:  # a2c.py:30-40, v_mpo.py:35-39
            self.pf_opt = self.optimizer_class([self.pf[k] for k in self.pf_keys], lr=lr_pf, eps=1e-5)
            self.vf_opt = self.optimizer_class([self.vf[k] for k in self.vf_keys], lr=lr_vf, eps=1e-5)
            self.param_opt = self.optimizer_class([self.eta, self.alpha], lr=lr_pf, eps=1e-5)
        for opt, lr in ((self.pf_opt, lr_pf), (self.vf_opt, lr_vf), (self.param_opt, lr_pf)):
            opt.param_groups[0]["lr"] = lr

    @staticmethod
    def _step(opt, tensors, grads):
        for p, g in zip(tensors, grads):
            p.grad = g.detach().clone()
        opt.step()
        for p in tensors:
            p.grad = None

    def select(self, advs):
        """v_mpo.py:65-67 on the normalised advantages [B, 1] -> the kept row indices [m] (stable: ties to the earlier row)."""
        _, idx = torch.sort(advs, dim=0, descending=True, stable=True)
        return idx.reshape(-1).long().chunk(2, dim=0)[0]

    def actor_losses(self, obs, acts, advs, grad=True):
        """v_mpo.py:69-102 on the normalised advantages. -> (policy_loss, eta_loss, alpha_loss, log_probs, kl, head output)."""
        idx = self.select(advs)
        obs, acts, advs = obs[idx], acts[idx], advs[idx]
        if grad:
            for k in self.pf_keys:
                self.pf[k].requires_grad_(True)
        out = self.fwd({k: v for k, v in self.pf.items() if k != "logstd"}, obs, self.S, self.mode)
        mean, std, _ = orc.gaussian(out, self.pf["logstd"])
        log_probs, _ = orc.log_prob_entropy(mean, std, acts, self.tanh_action)
        with torch.no_grad():
            tmean = self.fwd({k: v for k, v in self.tpf.items() if k != "logstd"}, obs, self.S, self.mode)
            tmean, tstd, _ = orc.gaussian(tmean, self.tpf["logstd"])
        phis = torch.softmax(advs / self.eta.detach(), dim=0)
        # `dis` is a plain Normal also for tanh_action policies (continuous_policy.py:127-146)
        kl = torch.distributions.kl.kl_divergence(torch.distributions.Normal(mean, std),
                                                  torch.distributions.Normal(tmean, tstd)).sum(-1, keepdim=True)
        eta_loss = self.eta * self.eta_eps + self.eta * torch.log(torch.mean(torch.exp(advs / self.eta)))
        alpha_loss = self.alpha * self.alpha_eps - self.alpha * kl.detach().mean()
        policy_loss = (-phis * log_probs + self.alpha.detach() * kl).mean()
        return policy_loss, eta_loss, alpha_loss, log_probs, kl, out

    def loss_grads(self, obs, acts, advs_raw):
        """One loss evaluation's gradients, nothing stepped: d(policy_loss)/d(head output) [m, A], /d(logstd) [A],
        d(eta_loss)/d(eta), d(alpha_loss)/d(alpha), and the kept row indices."""
        advs = (advs_raw - advs_raw.mean()) / (advs_raw.std() + 1e-5)
        policy_loss, eta_loss, alpha_loss, _, _, out = self.actor_losses(obs, acts, advs)
        dout, dls = torch.autograd.grad(policy_loss, [out, self.pf["logstd"]])
        deta, dalpha = torch.autograd.grad(eta_loss + alpha_loss, [self.eta, self.alpha])
        for k in self.pf_keys:
            self.pf[k].requires_grad_(False)
        return dout, dls, deta.item(), dalpha.item(), self.select(advs)

    def update(self, obs, acts, advs, est_rets, old_values, lr_pf, lr_vf):
        """obs [B, D], acts [B, A], advs / est_rets [B, 1]; old_values is unused (v_mpo.py:164). Returns the 19-key info."""
        import torch.nn.functional as F
        self._opts(lr_pf, lr_vf)
        info = {}
        self.step += 1
        info["advs/mean"], info["advs/std"] = advs.mean().item(), advs.std().item()
        info["advs/max"], info["advs/min"] = advs.max().item(), advs.min().item()
        advs = (advs - advs.mean()) / (advs.std() + 1e-5)                                    # v_mpo.py:179
        # ---- critic (v_mpo.py:136-155)
        for k in self.vf_keys:
            self.vf[k].requires_grad_(True)
        values = self.fwd(self.vf, obs, self.S, self.mode)
        vf_loss = F.mse_loss(values, est_rets)
        g = self._grads(vf_loss, self.vf, self.vf_keys, obs.shape[0])
        self.last_grads["vf"] = dict(zip(self.vf_keys, g))
        g, gn = orc.clip_grad_norm(g, self.max_norm)
        self._step(self.vf_opt, [self.vf[k] for k in self.vf_keys], g)
        info["Training/vf_loss"], info["grad_norm/vf"] = vf_loss.item(), gn.item()
        # ---- actor (v_mpo.py:58-134)
        policy_loss, eta_loss, alpha_loss, log_probs, kl, _ = self.actor_losses(obs, acts, advs)
        m = log_probs.shape[0]
        gs = torch.autograd.grad(eta_loss + alpha_loss, [self.eta, self.alpha])
        g = self._grads(policy_loss, self.pf, self.pf_keys, m)
        self.last_grads["pf"] = dict(zip(self.pf_keys, g))
        self.last_grads["scalars"] = (gs[0].item(), gs[1].item())
        g, gn = orc.clip_grad_norm(g, self.max_norm)
        self._step(self.pf_opt, [self.pf[k] for k in self.pf_keys], g)
        self._step(self.param_opt, [self.eta, self.alpha], gs)
        with torch.no_grad():
            self.eta.copy_(torch.clamp(self.eta, min=1e-8))
            self.alpha.copy_(torch.clamp(self.alpha, min=1e-8))
        info["Training/policy_loss"], info["Training/alpha_loss"] = policy_loss.item(), alpha_loss.item()
        info["Training/alpha"], info["Training/eta"] = self.alpha.item(), self.eta.item()
        lp, k = log_probs.detach(), kl.detach()
        info["logprob/mean"], info["logprob/std"] = lp.mean().item(), lp.std().item()
        info["logprob/max"], info["logprob/min"] = lp.max().item(), lp.min().item()
        info["KL/mean"], info["KL/std"], info["KL/max"], info["KL/min"] = k.mean().item(), k.std().item(), k.max().item(), k.min().item()
        info["grad_norm/pf"] = gn.item()
        return info


def batch_tensors(case, update, dtype=torch.float32):
    """util.make_batch(case, update) as the restatement's arguments: the fp32 values the engine gets, in `dtype`."""
    import util
    b = util.make_batch(case, update=update)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float32)).to(dtype)
    return t(b["obs"]), t(b["acts"]), t(b["advs"]), t(b["estimate_returns"]), t(b["values"])


def fresh_oracle(case, mode="f32", dtype=torch.float32, init=None):
    """A VMPOOracle on the case's seeded initial parameters (init: (pf state_dict, vf state_dict) to start from instead)."""
    import util
    if init is None:
        import vision4leg_amd.torchrl.networks as networks
        import vision4leg_amd.torchrl.policies as policies
        torch.manual_seed(case["seed"])
        pf, vf = util.build_nets(networks, policies, case)
        init = (pf.state_dict(), vf.state_dict())
    opf = {k: v.detach().cpu().clone().to(dtype) for k, v in init[0].items()}
    ovf = util.share_encoder(opf, {k: v.detach().cpu().clone().to(dtype) for k, v in init[1].items()}, case["kind"])
    oracle = VMPOOracle(case["kind"], opf, ovf, {k: v.clone() for k, v in opf.items()}, case["S"], mode)
    oracle.sync_target()
    return oracle
