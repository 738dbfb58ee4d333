"""Float64 restatement of the last stage of a PPO minibatch update: the critic and actor losses of PPO.update_critic /
update_actor (torchrl/algo/on_policy/ppo.py:42-123, the advantage normalisation of :142-148), their gradients with respect to
the network outputs (value column, mean rows) and logstd, the 18 logged scalars, and clip_grad_norm_ followed by torch.optim.Adam
(ppo.py:73-75,118-120; torch/optim/adam.py::_single_tensor_adam); and of the sampling epilogue of a rollout step (sample_stage:
std, action, entropy; the stored action's log-prob is log_prob_entropy). Everything runs in float64 on the CPU, so it can serve
as the yardstick of kernels that compute in fp32. tests/test_ref64_cpu.py pins it against oracle/ppo_oracle.py."""
import math

import numpy as np
import torch

LOG_SIG_MIN, LOG_SIG_MAX = -5.0, 2.0  # torchrl/policies/continuous_policy.py:8-9
EPS32 = 2.0 ** -24                    # fp32 unit roundoff
# the multiple of sample_stage_bounds the GPU rollout-epilogue tests allow: 4 x what fp32 numpy needs for the stored log-prob
# (0.58, measured by tests/test_ref64_cpu.py::test_sample_stage_fp32_needs_less_than_the_gate), and no lower than 4
ROLLOUT_C = 4.0

STAT_KEYS = [
    "advs/mean", "advs/std", "advs/max", "advs/min", "Training/vf_loss", "grad_norm/vf",
    "Training/policy_loss", "logprob/mean", "logprob/std", "logprob/max", "logprob/min",
    "log_std/mean", "log_std/std", "log_std/max", "log_std/min", "ratio/max", "ratio/min",
    "grad_norm/pf",
]


def _d(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float64) if not torch.is_tensor(x) else x.detach().cpu().double())


def log_prob_entropy(mean, logstd, acts, tanh_action=False):
    """Normal(mean, exp(clamp(logstd))).log_prob(acts).sum(-1), .entropy().sum(-1) (continuous_policy.py:127-146, 486-492);
    tanh_action: TanhNormal.log_prob of the stored post-tanh actions (policies/distribution.py:38-51). -> (lp [n], ent [n],
    clamped log_std [A])."""
    log_std = torch.clamp(logstd, LOG_SIG_MIN, LOG_SIG_MAX)
    std = torch.exp(log_std).unsqueeze(0).expand_as(mean)
    corr = 0.0
    if tanh_action:
        corr = torch.log(1 - acts * acts + 1e-6)
        acts = torch.log((1 + acts) / (1 - acts)) / 2
    lp = -((acts - mean) ** 2) / (2 * std ** 2) - std.log() - math.log(math.sqrt(2 * math.pi)) - corr
    ent = 0.5 + 0.5 * math.log(2 * math.pi) + torch.log(std)
    return lp.sum(-1), ent.sum(-1), log_std


def sample_stage(mean, logstd, eps, tanh_action=False):
    """The sampling epilogue of a rollout step (GaussianContPolicyBase.explore, continuous_policy.py:85-125; TanhNormal.rsample,
    policies/distribution.py:61-80) on given standard-normal draws: std = exp(clamp(logstd)), pre = mean + std * eps,
    action = tanh(pre) | pre, ent = Normal(mean, std).entropy().sum(-1). mean / eps [n][A], logstd [A] (the raw parameter).
    -> float64 (std [n][A], pre [n][A], action [n][A], ent [n]). The log-prob of a stored action is
    log_prob_entropy(mean, logstd, action, tanh_action)."""
    mean, logstd, eps = _d(mean), _d(logstd), _d(eps)
    log_std = torch.clamp(logstd, LOG_SIG_MIN, LOG_SIG_MAX)
    std = torch.exp(log_std).unsqueeze(0).expand_as(mean)
    pre = mean + std * eps
    action = torch.tanh(pre) if tanh_action else pre
    ent = (0.5 + 0.5 * math.log(2 * math.pi) + log_std).sum().expand(mean.shape[0])
    return std, pre, action, ent


def sample_stage_bounds(mean, logstd, eps, acts, tanh_action=False):
    """The magnitudes that enter an fp32 evaluation of sample_stage / log_prob_entropy, per element or row, in float64: an fp32
    result may differ from the float64 one by c * EPS32 times these (c: the few roundings per operation).
    - "action" [n][A]: |mean| + |std * eps| (the two addends), tanh: + |action| (tanhf's own rounding)
    - "ent" [n]: sum_a 1.5 + |log sigma_a| (0.5 + log(2 pi) / 2 + log sigma, summed)
    - "logp" [n] of the STORED action `acts`: sum_a q + |log sigma| + 1 + |corr| + |term|, q = d^2 / (2 sigma^2), term the a-th
      summand of log pi (the running sum); tanh rows add the conditioning of the reference's own expressions in fp32:
      |d| (1 + |z|) / sigma^2 (z = atanh(a) = log((1 + a) / (1 - a)) / 2 carries an absolute error ~ EPS32 (1 + |z|) into d) and
      1 / (1 - a^2 + 1e-6) (the rounding of 1 - a * a under corr = log(1 - a^2 + 1e-6))."""
    mean, logstd, eps, acts = _d(mean), _d(logstd), _d(eps), _d(acts)
    log_std = torch.clamp(logstd, LOG_SIG_MIN, LOG_SIG_MAX).unsqueeze(0).expand_as(mean)
    std = torch.exp(log_std)
    b_act = mean.abs() + (std * eps).abs()
    z, corr = acts, torch.zeros_like(acts)
    if tanh_action:
        b_act = b_act + acts.abs()
        corr = torch.log(1 - acts * acts + 1e-6)
        z = torch.log((1 + acts) / (1 - acts)) / 2
    d = z - mean
    q = d * d / (2 * std * std)
    term = -q - log_std - math.log(math.sqrt(2 * math.pi)) - corr
    b_lp = q + log_std.abs() + 1.0 + corr.abs() + term.abs()
    if tanh_action:
        b_lp = b_lp + d.abs() * (1 + z.abs()) / (std * std) + 1 / (1 - acts * acts + 1e-6)
    return {"action": b_act, "ent": (1.5 + log_std.abs()).sum(-1), "logp": b_lp.sum(-1)}


def sample_stage_f32(mean, logstd, eps, tanh_action=False):
    """sample_stage and the stored action's log-prob restated in fp32 numpy, one rounding per operation, the terms summed over
    a = 0 .. A-1 in order: what a straightforward fp32 implementation computes; measured against the float64 functions above it
    says which multiple of sample_stage_bounds fp32 arithmetic itself needs. -> fp32 (action [n][A], ent [n], logp [n])."""
    f = np.float32
    mean, logstd, eps = (np.asarray(x, dtype=f) for x in (mean, logstd, eps))
    half_log_2pi = f(0.5 * math.log(2 * math.pi))
    ls = np.clip(logstd, f(LOG_SIG_MIN), f(LOG_SIG_MAX))
    sg = np.exp(ls)
    act = sg[None] * eps + mean
    x = act
    if tanh_action:
        act = np.tanh(act)
        x = np.log((f(1) + act) / (f(1) - act)) / f(2)
    d = x - mean
    lt = -(d * d) / (f(2) * sg * sg)[None] - np.log(sg)[None] - half_log_2pi
    et = f(0.5) + half_log_2pi + np.log(sg)
    corr = np.log(f(1) - act * act + f(1e-6)) if tanh_action else None
    lp, ent = np.zeros(mean.shape[0], dtype=f), np.zeros(mean.shape[0], dtype=f)
    for a in range(mean.shape[1]):
        ent = ent + et[a]
        lp = lp + lt[:, a]
        if tanh_action:
            lp = lp - corr[:, a]
    assert act.dtype == f and lp.dtype == f and ent.dtype == f
    return act, ent, lp


def normalise_advantages(advs):
    """ppo.py:142-148: the logged moments and (advs - mean) / (std + 1e-5), Bessel std."""
    st = {"advs/mean": advs.mean().item(), "advs/std": advs.std().item(), "advs/max": advs.max().item(),
          "advs/min": advs.min().item()}
    return (advs - advs.mean()) / (advs.std() + 1e-5), st


def critic_loss(values, rets, old_values=None, clip=0.2, clipped_value_loss=False):
    """PPO.update_critic's loss (ppo.py:94-112) on value column [n]."""
    if clipped_value_loss:
        vc = old_values + (values - old_values).clamp(-clip, clip)
        return 0.5 * torch.max((values - rets).pow(2), (vc - rets).pow(2)).mean()
    return torch.nn.functional.mse_loss(values, rets)


def actor_loss(mean, logstd, acts, logp_old, an, clip=0.2, ent_coef=0.005, tanh_action=False):
    """PPO.update_actor's loss (ppo.py:42-71) -> (policy_loss, log_probs [n], ratio [n], clamped log_std [A])."""
    lp, ent, log_std = log_prob_entropy(mean, logstd, acts, tanh_action)
    ratio = torch.exp(lp - logp_old)
    s1 = ratio * an
    s2 = torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * an
    loss = -torch.mean(torch.min(s2, s1)) - ent_coef * ent.mean()
    return loss, lp, ratio, log_std


def loss_stage(values, rets, old_values, mean, logstd, acts, logp_old, advs, clip=0.2, ent_coef=0.005,
               clipped_value_loss=False, tanh_action=False):
    """Both losses on fixed network outputs, everything float64. values/rets/old_values/logp_old/advs [n], mean/acts [n][A],
    logstd [A]. -> {"stats": the 16 logged scalars that do not need the parameter gradients, "dvalues": d vf_loss / d values [n],
    "dmean": d policy_loss / d mean [n][A], "dlogstd": [A], "lp", "ratio", "an": per-row intermediates}."""
    values, rets, mean, logstd = (_d(x).clone().requires_grad_(True) if i in (0, 2, 3) else _d(x)
                                  for i, x in enumerate((values, rets, mean, logstd)))
    old_values = _d(old_values) if old_values is not None else None
    acts, logp_old, advs = _d(acts), _d(logp_old), _d(advs)
    an, st = normalise_advantages(advs)
    vf_loss = critic_loss(values, rets, old_values, clip, clipped_value_loss)
    (dvalues,) = torch.autograd.grad(vf_loss, [values])
    loss, lp, ratio, log_std = actor_loss(mean, logstd, acts, logp_old, an, clip, ent_coef, tanh_action)
    dmean, dlogstd = torch.autograd.grad(loss, [mean, logstd])
    lp, ratio, ls = lp.detach(), ratio.detach(), log_std.detach()
    st.update({"Training/vf_loss": vf_loss.item(), "Training/policy_loss": loss.item(),
               "logprob/mean": lp.mean().item(), "logprob/std": lp.std().item(), "logprob/max": lp.max().item(),
               "logprob/min": lp.min().item(), "log_std/mean": ls.mean().item(), "log_std/std": ls.std().item(),
               "log_std/max": ls.max().item(), "log_std/min": ls.min().item(), "ratio/max": ratio.max().item(),
               "ratio/min": ratio.min().item()})
    return {"stats": st, "dvalues": dvalues, "dmean": dmean, "dlogstd": dlogstd, "lp": lp, "ratio": ratio, "an": an.detach()}


def clip_grad_norm(grads, max_norm):
    """torch.nn.utils.clip_grad_norm_ on a list of float64 tensors -> (clipped list, pre-clip norm)."""
    total = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in grads]))
    coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
    return [g * coef for g in grads], float(total)


class Adam:
    """clip_grad_norm_(max_norm) + torch.optim.Adam (no weight decay) over a list of float64 parameter tensors, with its own
    step count: step() with skip=True leaves parameters, moments and the count alone (GradScaler.step's skip)."""

    def __init__(self, params, max_norm=0.5, betas=(0.9, 0.999), eps=1e-5):
        self.params = params
        self.m = [torch.zeros_like(p) for p in params]
        self.v = [torch.zeros_like(p) for p in params]
        self.max_norm, self.betas, self.eps = max_norm, betas, eps
        self.steps = 0

    def step(self, grads, lr, skip=False):
        """-> the pre-clip gradient norm."""
        grads, norm = clip_grad_norm([_d(g) for g in grads], self.max_norm)
        if skip:
            return norm
        self.steps += 1
        b1, b2 = self.betas
        step_size = lr / (1 - b1 ** self.steps)
        bc2_sqrt = math.sqrt(1 - b2 ** self.steps)
        with torch.no_grad():
            for p, g, m, v in zip(self.params, grads, self.m, self.v):
                m.lerp_(g, 1 - b1)
                v.mul_(b2).addcmul_(g, g, value=1 - b2)
                p.addcdiv_(m, (v.sqrt() / bc2_sqrt).add_(self.eps), value=-step_size)
        return norm


def ppo_update(fwd, pf, vf, tpf, obs, acts, advs, rets, old_values, lr_pf, lr_vf, opt_pf, opt_vf, S, clip=0.2, ent_coef=0.005,
               clipped_value_loss=False, tanh_action=False):
    """One PPO.update (ppo.py:125-153) in float64 over name -> tensor parameter dicts (pf / vf may share tensor objects, the way
    the starters share one encoder; the critic step is visible to the actor's forward). fwd: an oracle forward
    (oracle/ppo_oracle.py FORWARDS[kind]) run in its exact flavour. opt_pf / opt_vf: Adam over [pf[k] for k in pf] /
    [vf[k] for k in vf]. -> (info dict of the 18 logged scalars, {"pf": grads, "vf": grads} before clipping)."""
    obs, acts, advs, rets = _d(obs), _d(acts), _d(advs).reshape(-1), _d(rets).reshape(-1)
    old_values = _d(old_values).reshape(-1) if old_values is not None else None
    an, info = normalise_advantages(advs)
    vkeys, pkeys = list(vf), list(pf)
    for k in vkeys:
        vf[k].requires_grad_(True)
    vf_loss = critic_loss(fwd(vf, obs, S, "f32").reshape(-1), rets, old_values, clip, clipped_value_loss)
    gv = torch.autograd.grad(vf_loss, [vf[k] for k in vkeys], allow_unused=True)
    gv = [torch.zeros_like(vf[k]) if g is None else g for g, k in zip(gv, vkeys)]
    for k in vkeys:
        vf[k].requires_grad_(False)
    info["Training/vf_loss"] = vf_loss.item()
    info["grad_norm/vf"] = opt_vf.step(gv, lr_vf)
    with torch.no_grad():
        tmean = fwd({k: v for k, v in tpf.items() if k != "logstd"}, obs, S, "f32")
        logp_old, _, _ = log_prob_entropy(tmean, tpf["logstd"], acts, tanh_action)
    for k in pkeys:
        pf[k].requires_grad_(True)
    mean = fwd({k: v for k, v in pf.items() if k != "logstd"}, obs, S, "f32")
    loss, lp, ratio, log_std = actor_loss(mean, pf["logstd"], acts, logp_old, an, clip, ent_coef, tanh_action)
    gp = torch.autograd.grad(loss, [pf[k] for k in pkeys], allow_unused=True)
    gp = [torch.zeros_like(pf[k]) if g is None else g for g, k in zip(gp, pkeys)]
    for k in pkeys:
        pf[k].requires_grad_(False)
    lp, ratio, ls = lp.detach(), ratio.detach(), log_std.detach()
    info["Training/policy_loss"] = loss.item()
    info["logprob/mean"], info["logprob/std"] = lp.mean().item(), lp.std().item()
    info["logprob/max"], info["logprob/min"] = lp.max().item(), lp.min().item()
    info["log_std/mean"], info["log_std/std"] = ls.mean().item(), ls.std().item()
    info["log_std/max"], info["log_std/min"] = ls.max().item(), ls.min().item()
    info["ratio/max"], info["ratio/min"] = ratio.max().item(), ratio.min().item()
    info["grad_norm/pf"] = opt_pf.step(gp, lr_pf)
    return info, {"pf": dict(zip(pkeys, gp)), "vf": dict(zip(vkeys, gv))}
