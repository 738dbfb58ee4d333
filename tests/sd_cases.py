"""Cases of PPO with policies.GaussianContPolicy — the Gaussian policy whose log sigma is state dependent (the reference's
torchrl/policies/continuous_policy.py:222-236: a networks.Net with 2 A outputs, `x.chunk(2, -1)` -> mean and per-sample log
sigma, clamped to [-5, 2]) — and its restatement, shared by tests/golden/make_golden_sd.py, tests/test_sd_cpu.py and
tests/test_gpu_sd.py. Same fields as tests/util.CASES (A is the number of ACTION dimensions: the head is 2 A wide); kept apart
from it because every parity test there runs over all of util.CASES.

The nets are state-MLP pairs as starter/ppo_state.py wires them (`vf.base = pf.base`): `build_nets` below works on
vision4leg_amd.torchrl's modules or on the unmodified reference's.

`SDOracle` restates PPO.update (ppo.py:42-153) for this class on top of oracle.ppo_oracle without editing it: PPOOracle's
critic half, its FORWARDS[kind](..., mode) for the nets (tests/tact_cases.py registers the Tanh ones), orc.log_prob_entropy on
the per-row std, PPOOracle._grads (the f16 flavour's scaled backward — here d(loss)/d(raw log sigma) passes the head's
contractions like d(loss)/d(mean), so the scaling covers it). It runs in the oracle's modes on fp32 tensors and, handed float64
tensors with mode "f32", in float64. tests/golden/make_golden_sd.py pins it to the unmodified reference.
`loss_stage64` is the float64 restatement of the loss launch alone (tests/test_gpu_sd.py's teacher-forced test).

Why these shapes (the smallest at which this code can still go wrong):
  sd_mlp         S=93 A=6 B=64 [256,256]/[256,256]  the shipped geometry; fixture from the reference
  sd_mlp_tanh    the same, tanh_action               TanhNormal log-prob on a per-row sigma; fixture from the reference
  sd_mlp_odd     S=45 A=5 B=23 [128,64]/[72]         odd A (the log-sigma half starts at an unaligned column), odd n, a partial
                                                     wave in the loss block, the general (layer-by-layer) routes
  sd_mlp_a8      A=8 B=64                            2 A fills the padded 16-column head row exactly
  sd_mlp_a1      A=1 B=2                             log_std/std finite over two elements (no NaN exemption for this policy)
  sd_mlp_tact    Tanh activations, B=64
  sd_mlp_b1024   B=1024, one update                  the 1024-thread loss block (tests/wide_cases.py BIG_CASES: the fp32
                                                     restatement's own error after a second update at this size)

Seeds: 70 .. 76 in the order of the table, held to tests/wide_cases.py's rule ("Seeds"): after the updates the GPU test runs,
the fp32 restatement and the float64 restatement agree to ORACLE_F32_ERR_MAX on every parameter; where a seed does not pass,
the first of seed + 10, + 20, ... that does. And no raw log sigma of the restatement lies within CLAMP_MARGIN of a clamp bound
in any update, so that a 16-bit forward cannot flip a clamp gate (tests/test_sd_cpu.py asserts both for every case)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ppo_oracle as orc
import tact_cases  # noqa: F401  (registers the oracle's forward of the `mlp_tact` kinds)
from wide_cases import ORACLE_F32_ERR_MAX  # noqa: F401

SD_CASES = {
    "sd_mlp": dict(kind="mlp", S=93, A=6, seed=70, B=64, enc=[256, 256], head=[256, 256]),
    "sd_mlp_tanh": dict(kind="mlp_tanh", S=93, A=6, seed=71, B=64, enc=[256, 256], head=[256, 256]),
    "sd_mlp_odd": dict(kind="mlp", S=45, A=5, seed=72, B=23, enc=[128, 64], head=[72]),
    "sd_mlp_a8": dict(kind="mlp", S=93, A=8, seed=73, B=64, enc=[256, 256], head=[256, 256]),
    "sd_mlp_a1": dict(kind="mlp", S=45, A=1, seed=74, B=2, enc=[128, 64], head=[72]),
    "sd_mlp_tact": dict(kind="mlp_tact", S=93, A=6, seed=75, B=64, enc=[256, 256], head=[256, 256]),
    "sd_mlp_b1024": dict(kind="mlp", S=93, A=6, seed=76, B=1024, enc=[256, 256], head=[256, 256], updates=1),
}

# the cases the unmodified reference was run on: tests/golden/ppo_<name>.npz
FIXTURE_CASES = ("sd_mlp", "sd_mlp_tanh")

LR = 1e-4            # plr = vlr of every test (the parameter bounds of tests/test_gpu_wide_actions.py::test_two_updates are sized for it)
CLIP_PARA = 0.2
ENTROPY_COEFF = 0.005
CLAMP_MARGIN = 0.25  # no raw log sigma of a whole-update case within this of -5 or 2
LOG_SIG_MIN, LOG_SIG_MAX = -5.0, 2.0

BATCH_KEYS = ("obs", "acts", "advs", "estimate_returns", "values")


def updates_of(case):
    return case.get("updates", 2)


def build_nets(networks, policies, case):
    """pf / vf of a case as starter/ppo_state.py builds them, GaussianContPolicy in GaussianContPolicyBasicBias' place
    (output_shape = 2 A, as in the reference) and `vf.base = pf.base`. `networks` / `policies`: vision4leg_amd.torchrl's
    modules or the unmodified reference's."""
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
    pf = policies.GaussianContPolicy(input_shape=case["S"], output_shape=2 * case["A"], **net, **pol)
    vf = networks.Net(input_shape=(case["S"],), output_shape=1, **net)
    vf.base = pf.base
    return pf, vf


def seeded_nets(networks, policies, case):
    torch.manual_seed(case["seed"])
    return build_nets(networks, policies, case)


def head(out):
    """GaussianContPolicy.forward behind the net (continuous_policy.py:231-236). -> mean, std, clamped log_std, raw log_std."""
    mean, raw = out.chunk(2, dim=-1)
    log_std = torch.clamp(raw, LOG_SIG_MIN, LOG_SIG_MAX)
    return mean, torch.exp(log_std), log_std, raw


class SDOracle(orc.PPOOracle):
    """PPO.update with a GaussianContPolicy: PPOOracle's critic half as it stands, the actor half on the per-row head."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.min_clamp_gap = float("inf")  # smallest distance of a raw log sigma to a clamp bound seen so far

    def policy(self, params, obs):
        return head(self.fwd(params, obs, self.S, self.mode))

    def update(self, obs, acts, advs, est_rets, old_values, lr_pf, lr_vf):
        info = {}
        self.step += 1
        info["advs/mean"] = advs.mean().item()
        info["advs/std"] = advs.std().item()
        info["advs/max"] = advs.max().item()
        info["advs/min"] = advs.min().item()
        advs = (advs - advs.mean()) / (advs.std() + 1e-5)                                    # ppo.py:148
        # ---- critic (ppo.py:94-123): PPOOracle.update's statements
        for k in self.vf_keys:
            self.vf[k].requires_grad_(True)
        values = self.fwd(self.vf, obs, self.S, self.mode)
        if self.clipped_value_loss:
            vc = old_values + (values - old_values).clamp(-self.clip_para, self.clip_para)
            vf_loss = 0.5 * torch.max((values - est_rets).pow(2), (vc - est_rets).pow(2)).mean()
        else:
            vf_loss = F.mse_loss(values, est_rets)
        g = self._grads(vf_loss, self.vf, self.vf_keys, obs.shape[0])
        self.last_grads["vf"] = dict(zip(self.vf_keys, g))
        g, gn = orc.clip_grad_norm(g, self.max_norm)
        orc.adam_step([self.vf[k] for k in self.vf_keys], g, self.vf_state, lr_vf, self.step)
        info["Training/vf_loss"] = vf_loss.item()
        info["grad_norm/vf"] = gn.item()
        # ---- actor (ppo.py:42-92) on GaussianContPolicy.update (continuous_policy.py:127-146, 228-236)
        for k in self.pf_keys:
            self.pf[k].requires_grad_(True)
        mean, std, log_std, raw = self.policy(self.pf, obs)
        log_probs, ent = orc.log_prob_entropy(mean, std, acts, self.tanh_action)
        with torch.no_grad():
            tmean, tstd, _, traw = self.policy(self.tpf, obs)
            target_log_probs, _ = orc.log_prob_entropy(tmean, tstd, acts, self.tanh_action)
            for r in (raw.detach(), traw):
                gap = torch.minimum((r - LOG_SIG_MIN).abs(), (r - LOG_SIG_MAX).abs()).min().item()
                self.min_clamp_gap = min(self.min_clamp_gap, gap)
        ratio = torch.exp(log_probs - target_log_probs)
        s1 = ratio * advs
        s2 = torch.clamp(ratio, 1.0 - self.clip_para, 1.0 + self.clip_para) * advs
        policy_loss = -torch.mean(torch.min(s2, s1)) - self.entropy_coeff * ent.mean()
        g = self._grads(policy_loss, self.pf, self.pf_keys, obs.shape[0])
        self.last_grads["pf"] = dict(zip(self.pf_keys, g))
        g, gn = orc.clip_grad_norm(g, self.max_norm)
        orc.adam_step([self.pf[k] for k in self.pf_keys], g, self.pf_state, lr_pf, self.step)
        info["Training/policy_loss"] = policy_loss.item()
        lp = log_probs.detach()
        info["logprob/mean"], info["logprob/std"] = lp.mean().item(), lp.std().item()
        info["logprob/max"], info["logprob/min"] = lp.max().item(), lp.min().item()
        ls = log_std.detach()                                                                # [n, A] (ppo.py:84-87)
        info["log_std/mean"], info["log_std/std"] = ls.mean().item(), ls.std().item()
        info["log_std/max"], info["log_std/min"] = ls.max().item(), ls.min().item()
        info["ratio/max"], info["ratio/min"] = ratio.max().item(), ratio.min().item()
        info["grad_norm/pf"] = gn.item()
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
    """An SDOracle on copies of two state_dicts (vf's `base.*` entries are pf's tensors, as the modules share them), its target
    policy synchronised."""
    import util
    opf = {k: v.detach().cpu().clone().to(dtype) for k, v in pf_sd.items()}
    ovf = util.share_encoder(opf, {k: v.detach().cpu().clone().to(dtype) for k, v in vf_sd.items()}, case["kind"])
    kw.setdefault("clip_para", CLIP_PARA)
    kw.setdefault("entropy_coeff", ENTROPY_COEFF)
    o = SDOracle(case["kind"], opf, ovf, {k: v.clone() for k, v in opf.items()}, case["S"], mode, **kw)
    o.sync_target()
    return o


def fresh_oracle(case, mode="f32", dtype=torch.float32, init=None, **kw):
    """An SDOracle on the case's seeded initial parameters (init: (pf state_dict, vf state_dict) to start from instead)."""
    if init is None:
        import vision4leg_amd.torchrl.networks as networks
        import vision4leg_amd.torchrl.policies as policies
        pf, vf = seeded_nets(networks, policies, case)
        init = (pf.state_dict(), vf.state_dict())
    return oracle_of(init[0], init[1], case, mode, dtype, **kw)


# ------------------------------------------------------------------------------------------ the loss launch alone, float64
F16_GRAD_CLAMP = 32768.0  # V4L_F16_GRAD_CLAMP (include/v4l_hip.h): the scaled loss-gradient rows stay inside +- this


def loss_stage64(rows, trows, logp_old, acts, advs, A, clip, ent_coef, tanh, gscale=1.0):
    """The actor loss launch of a GaussianContPolicy update (ppo.py:42-92 on continuous_policy.py:127-146, 228-236) in float64,
    by autograd, on given head rows. rows: [n, >= 2A] head outputs of the live policy (fp32 values); trows: the frozen target's,
    or None with logp_old [n] given (log pi_old stored at action time); acts [n, A]; advs [n] raw.
    -> dict: dout [n, 2A] = d(loss)/d(row) unscaled, stats (the 11 actor keys + advs/*), lp, ratio, an, raw, open (the clamp's
    gradient mask), sat (elements of dout * gscale beyond +-F16_GRAD_CLAMP, 0 for gscale == 1)."""
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    out = t(rows)[:, :2 * A].clone().requires_grad_(True)
    acts, advs = t(acts), t(advs).reshape(-1, 1)
    mean, std, log_std, raw = head(out)
    lp, ent = orc.log_prob_entropy(mean, std, acts, tanh)
    if trows is not None:
        tm, ts, _, _ = head(t(trows)[:, :2 * A])
        lpo, _ = orc.log_prob_entropy(tm, ts, acts, tanh)
    else:
        lpo = t(logp_old).reshape(-1, 1)
    amean, astd = advs.mean(), advs.std()
    an = (advs - amean) / (astd + 1e-5)
    ratio = torch.exp(lp - lpo)
    s1 = ratio * an
    s2 = torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * an
    loss = -torch.mean(torch.min(s2, s1)) - ent_coef * ent.mean()
    dout, = torch.autograd.grad(loss, [out])
    l, ls, r = lp.detach(), log_std.detach(), ratio.detach()
    stats = {"advs/mean": amean.item(), "advs/std": astd.item(), "advs/max": advs.max().item(), "advs/min": advs.min().item(),
             "Training/policy_loss": loss.item(),
             "logprob/mean": l.mean().item(), "logprob/std": l.std().item(), "logprob/max": l.max().item(), "logprob/min": l.min().item(),
             "log_std/mean": ls.mean().item(), "log_std/std": ls.std().item(), "log_std/max": ls.max().item(), "log_std/min": ls.min().item(),
             "ratio/max": r.max().item(), "ratio/min": r.min().item()}
    rawd = raw.detach()
    sat = int(((dout * gscale).abs() > F16_GRAD_CLAMP).sum().item()) if gscale != 1.0 else 0
    return {"dout": dout.numpy(), "stats": stats, "lp": l.reshape(-1).numpy(), "ratio": r.reshape(-1).numpy(),
            "an": an.reshape(-1).numpy(), "raw": rawd.numpy(), "open": ((rawd >= LOG_SIG_MIN) & (rawd <= LOG_SIG_MAX)).numpy(),
            "std": std.detach().numpy(), "mean": mean.detach().numpy(), "sat": sat}

