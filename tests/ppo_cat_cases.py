"""Cases of algo.PPODiscrete — the clipped-surrogate PPO update (the reference's torchrl/algo/on_policy/ppo.py:42-153) on
policies.CategoricalDisPolicy (torchrl/policies/discrete_policies.py:127-172) — and their restatement, shared by
tests/golden/make_golden_ppo_cat.py, tests/test_ppo_cat_cpu.py and tests/test_gpu_ppo_cat.py.

`CatPPOOracle` restates PPO.update for this class on top of oracle.ppo_oracle.PPOOracle the way tests/sd_cases.SDOracle does for
GaussianContPolicy: PPOOracle's critic half as it stands, the actor half on cat_cases.head (Categorical(probs=softmax(logits))),
PPOOracle._grads for the f16 flavour's scaled backward. It runs in the oracle's modes on fp32 tensors and, handed float64 tensors
with mode "f32", in float64. The reference's PPO reads out['log_std'] (ppo.py:53), which the class does not return, so the
returned info has the reference's 18 keys without the four log_std/* (INFO_KEYS). tests/golden/make_golden_ppo_cat.py pins it to
the unmodified reference. `loss_stage64` is the float64 restatement of the loss launch alone.

Why these shapes (the smallest at which this code can still go wrong):
  ppo_cat_mlp     S=93 K=6  B=64 [256,256]/[256,256], vf.base = pf.base   the shipped geometry as starter/ppo_state.py wires it;
                                                                         fixture from the reference
  ppo_cat_sep     the same, no common parameter                           the pair the A2C cases of tests/cat_cases.py use
  ppo_cat_k16     S=45 K=16 B=23 [128,64]/[72]                            the full head row, odd n, a partial wave in the loss block
  ppo_cat_k2      S=45 K=2  B=2  [128,64]/[72]                            the smallest distribution and the smallest batch
  ppo_cat_clipvf  as ppo_cat_mlp, clipped_value_loss=True
  ppo_cat_tact    as ppo_cat_mlp, Tanh activations

`scale`: cat_cases' (its docstring): the head's last layer is multiplied by it so that the largest probability of a batch lies
in P_MAX_RANGE and the smallest in P_MIN_RANGE (K = 2: cat_cases' exemption).

Conditions on the clip (asserted by tests/test_ppo_cat_cpu.py from the float64 restatement alone): in at least one update after
the first — in the first the live policy differs from the target by the critic's step on a common base at most, and every ratio
is within a few per cent of 1 — the share of rows whose surrogate has zero slope
(ratio * an > clamp(ratio) * an) lies in ZERO_SLOPE_RANGE for every case with B >= 23, and in that same update no ratio lies
within RATIO_GAP of 1 +- clip. Two updates at LR = 1e-4 move the sharpened logits by |dz| ~ scale x lr x |h| — enough for
ratios beyond the clip on some rows, not on 10 % of them: where the second update does not meet the condition the case runs a
third (`updates=3`), and where that does not either it takes its own learning rate (`lr`); the condition is never widened.

Seeds: 160 .. 165 in the order of the table, held to tests/wide_cases.py's rule ("Seeds"): after the updates the GPU test runs,
the fp32 and the float64 restatement agree to ORACLE_F32_ERR_MAX on every parameter; where a seed does not pass, the first of
seed + 10, + 20, ... that does: SEED_LOG."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ppo_oracle as orc
import cat_cases as cc
import tact_cases  # noqa: F401  (registers the oracle's forward of the `mlp_tact` kinds)
from cat_cases import P_MAX_RANGE, P_MIN_RANGE, make_acts, sharpen  # noqa: F401
from wide_cases import ORACLE_F32_ERR_MAX  # noqa: F401

_MLP = dict(kind="mlp", S=93, K=6, A=1, B=64, enc=[256, 256], head=[256, 256])
_SMALL = dict(kind="mlp", S=45, A=1, enc=[128, 64], head=[72])
PPO_CAT_CASES = {
    "ppo_cat_mlp": dict(_MLP, seed=160, shared=True, scale=600.0),
    "ppo_cat_sep": dict(_MLP, seed=161, shared=False, scale=1000.0),
    # two and three updates at LR leave every ratio of this batch inside the clip (23 rows, 16 classes: log pi moves slowly); at
    # 3e-4 the third update clips 3 of the 23 rows, the smallest rate of {1.5, 2, 2.5, 3}e-4 at which an update of the first
    # four does
    "ppo_cat_k16": dict(_SMALL, K=16, B=23, seed=162, shared=True, scale=800.0, lr=3e-4, updates=3),
    "ppo_cat_k2": dict(_SMALL, K=2, B=2, seed=163, shared=True, scale=850.0),
    "ppo_cat_clipvf": dict(_MLP, seed=164, shared=True, scale=600.0, clipped_value_loss=True),
    "ppo_cat_tact": dict(_MLP, kind="mlp_tact", seed=165, shared=True, scale=800.0),
}

# seed rule: worst |fp32 - float64| parameter after the case's updates at the kept seed, and what the seeds that were passed
# over measured (tests/test_ppo_cat_cpu.py::test_seed_rule prints the kept ones)
SEED_LOG = {
    "ppo_cat_mlp": (160, 1.17e-07), "ppo_cat_sep": (161, 2.24e-07), "ppo_cat_k16": (162, 3.42e-07), "ppo_cat_k2": (163, 1.58e-07),
    "ppo_cat_clipvf": (164, 1.14e-07), "ppo_cat_tact": (165, 2.33e-07),
    "passed over": {},  # every first seed passed
}

FIXTURE_CASE = "ppo_cat_mlp"  # the case the unmodified reference was run on: tests/golden/ppo_cat_mlp.npz
FIXTURE = "ppo_cat_mlp"

LR = 1e-4  # plr = vlr (the parameter bounds of tests/test_gpu_sd.py::test_two_updates are sized for it); a case's `lr` overrides
CLIP_PARA = 0.2
ENTROPY_COEFF = 0.005

# the reference PPO's 18 keys in its order without log_std/*: what PPODiscrete.update returns
INFO_KEYS = ["advs/mean", "advs/std", "advs/max", "advs/min", "Training/vf_loss", "grad_norm/vf", "Training/policy_loss",
             "logprob/mean", "logprob/std", "logprob/max", "logprob/min", "ratio/max", "ratio/min", "grad_norm/pf"]

BATCH_KEYS = tuple(cc.BATCH_KEYS) + ("values",)

ZERO_SLOPE_RANGE = (0.10, 0.90)
RATIO_GAP = 2e-3


def updates_of(case):
    return case.get("updates", 2)


def lr_of(case):
    return case.get("lr", LR)


def build_nets(networks, policies, case):
    """pf / vf of a case: CategoricalDisPolicy in GaussianContPolicyBasicBias' place, its last layer sharpened; shared:
    `vf.base = pf.base` as starter/ppo_state.py wires the pair, otherwise each net its own MLPBase (cat_cases.build_nets).
    `networks` / `policies`: vision4leg_amd.torchrl's modules or the unmodified reference's."""
    net = {"append_hidden_shapes": list(case["head"]), "base_type": networks.MLPBase, "hidden_shapes": list(case["enc"])}
    if case["kind"].endswith("_tact"):
        net["activation_func"] = torch.nn.Tanh
    pf = policies.CategoricalDisPolicy(input_shape=case["S"], output_shape=case["K"], **net)
    vf = networks.Net(input_shape=(case["S"],), output_shape=1, **net)
    if case["shared"]:
        vf.base = pf.base
    return sharpen(pf, case["scale"]), vf


def seeded_nets(networks, policies, case):
    torch.manual_seed(case["seed"])
    return build_nets(networks, policies, case)


def host_batch(case, update):
    """The host batch of an update as the collector's host buffer yields it: obs [B, S], acts [B] indices, advs,
    estimate_returns and values [B, 1] (util.make_batch's, with the Gaussian actions replaced)."""
    import util
    b = util.make_batch(case, update=update)
    out = {k: b[k] for k in BATCH_KEYS}
    out["acts"] = make_acts(case, update)
    return out


def batch_tensors(case, update, dtype=torch.float32):
    """host_batch as the restatement's arguments: the fp32 values the engine gets, in `dtype`; acts stay int64 [B]."""
    b = host_batch(case, update)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float32)).to(dtype)
    return t(b["obs"]), torch.tensor(b["acts"]), t(b["advs"]), t(b["estimate_returns"]), t(b["values"])


class CatPPOOracle(orc.PPOOracle):
    """PPO.update with a CategoricalDisPolicy: PPOOracle's critic half as it stands, the actor half on cat_cases.head.
    `seen` keeps, per update, what the conditions of the module docstring are stated on."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.seen = []

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
        # ---- actor (ppo.py:42-92) on CategoricalDisPolicy.update (discrete_policies.py:160-172)
        for k in self.pf_keys:
            self.pf[k].requires_grad_(True)
        probs, log_probs, ent = cc.head(self.fwd(self.pf, obs, self.S, self.mode), acts)
        with torch.no_grad():
            _, target_log_probs, _ = cc.head(self.fwd(self.tpf, obs, self.S, self.mode), acts)
        assert log_probs.shape == advs.shape
        ratio = torch.exp(log_probs - target_log_probs)
        s1 = ratio * advs
        s2 = torch.clamp(ratio, 1.0 - self.clip_para, 1.0 + self.clip_para) * advs
        policy_loss = -torch.mean(torch.min(s2, s1)) - self.entropy_coeff * ent.mean()       # ppo.py:69: ent.mean() per row
        g = self._grads(policy_loss, self.pf, self.pf_keys, obs.shape[0])
        self.last_grads["pf"] = dict(zip(self.pf_keys, g))
        g, gn = orc.clip_grad_norm(g, self.max_norm)
        orc.adam_step([self.pf[k] for k in self.pf_keys], g, self.pf_state, lr_pf, self.step)
        info["Training/policy_loss"] = policy_loss.item()
        lp = log_probs.detach()
        info["logprob/mean"], info["logprob/std"] = lp.mean().item(), lp.std().item()
        info["logprob/max"], info["logprob/min"] = lp.max().item(), lp.min().item()
        r = ratio.detach()
        info["ratio/max"], info["ratio/min"] = r.max().item(), r.min().item()
        info["grad_norm/pf"] = gn.item()
        p = probs.detach()
        gap = torch.minimum((r - (1.0 - self.clip_para)).abs(), (r - (1.0 + self.clip_para)).abs()).min().item()
        self.seen.append({"p_max": p.max().item(), "p_min": p.min().item(), "zero_slope": (s1 > s2).double().mean().item(),
                          "ratio_gap": gap})
        return {k: info[k] for k in INFO_KEYS}


def oracle_of(pf_sd, vf_sd, case, mode="f32", dtype=torch.float32, **kw):
    """A CatPPOOracle on copies of two state_dicts (shared: vf's `base.*` entries are pf's tensors, as the modules share them),
    its target policy synchronised."""
    import util
    opf = {k: v.detach().cpu().clone().to(dtype) for k, v in pf_sd.items()}
    ovf = {k: v.detach().cpu().clone().to(dtype) for k, v in vf_sd.items()}
    if case["shared"]:
        ovf = util.share_encoder(opf, ovf, case["kind"])
    kw.setdefault("clip_para", CLIP_PARA)
    kw.setdefault("entropy_coeff", ENTROPY_COEFF)
    kw.setdefault("clipped_value_loss", bool(case.get("clipped_value_loss", False)))
    o = CatPPOOracle(case["kind"], opf, ovf, {k: v.clone() for k, v in opf.items()}, case["S"], mode, **kw)
    o.sync_target()
    return o


def fresh_oracle(case, mode="f32", dtype=torch.float32, init=None, **kw):
    """A CatPPOOracle on the case's seeded initial parameters (init: (pf state_dict, vf state_dict) to start from instead)."""
    if init is None:
        import vision4leg_amd.torchrl.networks as networks
        import vision4leg_amd.torchrl.policies as policies
        pf, vf = seeded_nets(networks, policies, case)
        init = (pf.state_dict(), vf.state_dict())
    return oracle_of(init[0], init[1], case, mode, dtype, **kw)


def run_updates(oracle, case, dtype=torch.float32):
    """The case's updates (no target sync in between, as the GPU test runs them) -> the infos."""
    return [oracle.update(*batch_tensors(case, u, dtype), lr_of(case), lr_of(case)) for u in range(updates_of(case))]


# ------------------------------------------------------------------------------------------ the loss launch alone, float64
def loss_stage64(rows, trows, logp_old, acts, advs, K, clip, ent_coef):
    """The actor loss launch of a PPODiscrete update in float64 on given fp32 logits rows, in cat_edge_cases.loss64's manner.
    rows: [n, >= K] logits of the live policy; trows: the frozen target's, or None with logp_old [n] given (log pi_old stored at
    action time); acts [n] indices; advs [n] raw. -> cat_edge_cases.head64's fields of the live rows plus th (the target's, or
    None), lpo, ratio, an, amean, astd, hit, zero (rows whose surrogate has zero slope: ratio an > clamp(ratio) an), dlp, dz [n, K]
    = d(loss)/d(logits) as the kernel documents it, and stats (the 7 actor keys + advs/*)."""
    import cat_edge_cases as ce
    acts = np.asarray(acts, dtype=np.int64).reshape(-1)
    h = ce.head64(np.asarray(rows)[:, :K], acts)
    n = len(acts)
    th = None
    if trows is not None:
        th = ce.head64(np.asarray(trows)[:, :K], acts)
        lpo = th["lp"]
    else:
        lpo = np.asarray(logp_old, dtype=np.float32).astype(np.float64).reshape(-1)
    an, amean, astd = ce.adv_norm64(advs)
    a = np.asarray(advs, dtype=np.float32).astype(np.float64).reshape(-1)
    lp = h["lp"]
    ratio = np.exp(lp - lpo)
    pre, clp = ratio * an, np.clip(ratio, 1.0 - clip, 1.0 + clip) * an
    zero = pre > clp
    dlp = np.where(zero, 0.0, -an * ratio / n)
    hit = np.zeros((n, K))
    hit[np.arange(n), acts] = 1.0
    with np.errstate(invalid="ignore"):
        plg = np.where(h["p"] > 0, h["p"] * (h["lg"] + h["H"][:, None]), 0.0)
    dz = dlp[:, None] * (hit - h["p"]) + (ent_coef / n) * plg
    loss = -np.mean(np.minimum(pre, clp)) - ent_coef * h["H"].mean()
    stats = {"advs/mean": amean, "advs/std": astd, "advs/max": a.max(), "advs/min": a.min(), "Training/policy_loss": loss,
             "logprob/mean": lp.mean(), "logprob/std": lp.std(ddof=1), "logprob/max": lp.max(), "logprob/min": lp.min(),
             "ratio/max": ratio.max(), "ratio/min": ratio.min()}
    return dict(h, th=th, lpo=lpo, ratio=ratio, an=an, amean=amean, astd=astd, a=a, hit=hit, zero=zero, dlp=dlp, dz=dz, stats=stats)


def loss_stage_gates(R, stored, clip, ent_coef):
    """loss_stage64's dict -> absolute bounds: dz [n, K] and one per statistic. No measured number: u = EPS32 = 2^-24 times the
    magnitudes that enter a quantity, on top of cat_edge_cases.head_gates (its derivation of |d lg|, |d p|, |d H|) and
    tests/test_gpu_loss_adam.py's e_an = 8 u (|a| + |mean|) / std:
      lpo       stored: the fp32 value itself, no error; target: the target rows' own |d lg| at the action
      ratio = expf(lp - lpo)     rel(ratio) <= e_lp + e_lpo + u |lp - lpo| + C_FN u  =: e_r     (the difference, then expf)
      dlp = -inv_n an ratio      |d dlp| <= |dlp| (e_r + 3 u) + ratio e_an / n                 (inv_n and two products)
      A_j = dlp (hit - p_j)      |d A_j| <= |hit - p_j| |d dlp| + |dlp| |d p_j| + 2 u |A_j|
      B_j = dent p_j (lg_j + H)  |d B_j| <= (ent_coef / n) (|d p_j| |lg_j + H| + p_j (|d lg_j| + |d H|)) + 5 u |B_j|
      dz_j = A_j + B_j           + 2 u (|A_j| + |B_j|)     (the sum, or its contraction)
    A row whose ratio lies within RATIO_GAP of 1 +- clip could take the other branch in fp32; the tests' inputs hold none.
      sur = min(ratio an, clamp(ratio) an)   |d sur| <= ratio (|an| (e_r + 2 u) + e_an)
      policy_loss = -mean(sur) - ent_coef mean(H): double sums of fp32 terms, one rounding: + 8 u of the magnitudes
      logprob/*, ratio/*, advs/*: tests/test_gpu_sd.py::_check_loss_stage's expressions."""
    import cat_edge_cases as ce
    u = ce.EPS32
    g = ce.head_gates(R)
    n, K = R["p"].shape
    on = R["hit"] > 0
    e_lp = g["lg"][on]
    e_lpo = np.zeros(n) if stored else ce.head_gates(R["th"])["lg"][on]
    e_r = e_lp + e_lpo + u * np.abs(R["lp"] - R["lpo"]) + ce.C_FN * u
    e_an = 8 * u * (np.abs(R["a"]) + abs(R["amean"])) / R["astd"]
    ratio, an = R["ratio"], np.abs(R["an"])
    d_dlp = np.abs(R["dlp"]) * (e_r + 3 * u) + np.where(R["zero"], 0.0, ratio * e_an / n)
    hp = np.abs(R["hit"] - R["p"])
    A = np.abs(R["dlp"])[:, None] * hp
    lgH = np.abs(R["lg"] + R["H"][:, None])
    B = (ent_coef / n) * R["p"] * lgH
    dA = hp * d_dlp[:, None] + np.abs(R["dlp"])[:, None] * g["p"] + 2 * u * A
    dB = (ent_coef / n) * (g["p"] * lgH + R["p"] * (g["lg"] + g["H"][:, None])) + 5 * u * B
    g_dz = dA + dB + 2 * u * (A + B) + 1e-30
    s = R["stats"]
    e_sur = ratio * (an * (e_r + 2 * u) + e_an)
    stats = {
        "advs/mean": 2 * u * abs(s["advs/mean"]) + 1e-30,
        "advs/std": 8 * u * s["advs/std"] + 4 * u * abs(s["advs/mean"]) / np.sqrt(n),
        "advs/max": 0.0, "advs/min": 0.0,
        "Training/policy_loss": np.mean(e_sur) + ent_coef * np.mean(g["H"]) + 8 * u * (np.mean(ratio * an) + ent_coef * np.mean(R["H"])),
        "logprob/mean": np.mean(e_lp) + 2 * u * abs(s["logprob/mean"]),
        "logprob/std": 2 * np.max(e_lp) + 4 * u * s["logprob/std"],
        "logprob/max": np.max(e_lp), "logprob/min": np.max(e_lp),
        "ratio/max": np.max(e_r * ratio) + 2 * u * s["ratio/max"], "ratio/min": np.max(e_r * ratio) + 2 * u * s["ratio/min"],
    }
    return dict(dz=g_dz, stats=stats, e_r=e_r)
