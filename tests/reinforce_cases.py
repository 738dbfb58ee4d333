"""Cases of the REINFORCE update (the reference's torchrl/algo/on_policy/reinforce.py) and its restatement, shared by
tests/golden/make_golden_reinforce.py, tests/test_reinforce_cpu.py and tests/test_gpu_reinforce.py. Same fields as
tests/util.CASES; kept apart from it because every parity test there runs over all of util.CASES.

The policies are built as the starters build them (util.build_nets: the critic it returns is dropped — the reference's Reinforce
holds a ZeroNet, algo.Reinforce a networks.zero_critic(pf)). Unlike A2C, REINFORCE has no vf.backward(), so the vision kinds run.

`ReinforceOracle` restates Reinforce.update (reinforce.py:34-76) over a name -> tensor parameter dict on top of
oracle.ppo_oracle — its FORWARDS[kind](..., mode) for the nets (tests/tact_cases.py registers the Tanh ones), log_prob_entropy,
PPOOracle._grads (the f16 flavour's scaled backward), clip_grad_norm — and torch.optim.Adam built as the reference builds it,
`optimizer_class(params, lr=plr)`: eps is torch's default 1e-8, not the 1e-5 of A2C / PPO (orc.adam_step's eps argument would do
too; the torch class keeps `optimizer_class` testable, as in tests/a2c_cases.py). It runs in the oracle's modes ("f32", "bf16",
"f16") on fp32 tensors and, handed float64 tensors with mode "f32", in float64. tests/golden/make_golden_reinforce.py pins it to
the unmodified reference.

Why these shapes (the smallest at which this code can still go wrong):
  rf_mlp        mlp S=93 A=6 B=64 [256,256]/[256,256]   the shipped geometry; fixture from the reference
  rf_loco       loco S=84 A=6 B=32, 2 layers ff=256     a vision kind through forward / loss / backward; fixture from the reference
  rf_mlp_tanh   as rf_mlp, tanh_action                  TanhNormal log-prob next to the plain Normal's entropy
  rf_mlp_odd    mlp S=45 A=12 B=23 [128,64]/[72]        the capacity-16 loss code, odd n, a partial wave in the loss block
  rf_mlp_a1     mlp S=45 A=1 B=2 [128,64]/[72]          logprob/std and advs/std over two elements
  rf_cnn        cnn S=93 A=6 B=32 visual_dim=256        the NatureCNN kind
  rf_mlp_tact   as rf_mlp, Tanh activations
  rf_mlp_b1024  as rf_mlp, B=1024, one update           the 1024-thread loss block

Seeds: 80 .. 87 in the order of the table (rf_cnn: 85 -> 95), held to tests/wide_cases.py's rule ("Seeds"): after the updates the GPU test runs,
the fp32 restatement and the float64 restatement agree to ORACLE_F32_ERR_MAX on every parameter (tests/test_reinforce_cpu.py
asserts it for every case); where a seed does not pass, the first of seed + 10, + 20, ... that does. With eps 1e-8 an Adam step of
a parameter whose gradient is ~1e-8 is decided by fp32 rounding, so more seeds move than under eps 1e-5. Measured worst
|fp32 - float64| parameter distance per case and the seeds that were passed over are listed in SEED_LOG below."""
import numpy as np
import torch

from oracle import ppo_oracle as orc
import tact_cases  # noqa: F401  (registers the oracle's forward of the `mlp_tact` kinds)
from wide_cases import ORACLE_F32_ERR_MAX  # noqa: F401

REINFORCE_CASES = {
    "rf_mlp": dict(kind="mlp", S=93, A=6, seed=80, B=64, enc=[256, 256], head=[256, 256]),
    "rf_loco": dict(kind="loco", S=84, A=6, seed=81, B=32, enc=[256, 256], head=[256, 256], layers=2, ff=256),
    "rf_mlp_tanh": dict(kind="mlp_tanh", S=93, A=6, seed=82, B=64, enc=[256, 256], head=[256, 256]),
    "rf_mlp_odd": dict(kind="mlp", S=45, A=12, seed=83, B=23, enc=[128, 64], head=[72]),
    "rf_mlp_a1": dict(kind="mlp", S=45, A=1, seed=84, B=2, enc=[128, 64], head=[72]),
    "rf_cnn": dict(kind="cnn", S=93, A=6, seed=95, B=32, enc=[256, 256], head=[256, 256], visual_dim=256),
    "rf_mlp_tact": dict(kind="mlp_tact", S=93, A=6, seed=86, B=64, enc=[256, 256], head=[256, 256]),
    "rf_mlp_b1024": dict(kind="mlp", S=93, A=6, seed=87, B=1024, enc=[256, 256], head=[256, 256], updates=1),
}

# seed rule: what each case's seed measures (worst |fp32 - float64| parameter after the case's updates), and the table seeds
# that were passed over with what they measured. Filled from tests/test_reinforce_cpu.py::test_seed_rule's printout.
SEED_LOG = {
    "rf_mlp": (80, 2.75e-07), "rf_loco": (81, 1.99e-07), "rf_mlp_tanh": (82, 2.90e-07), "rf_mlp_odd": (83, 2.16e-07),
    "rf_mlp_a1": (84, 2.18e-07), "rf_cnn": (95, 6.39e-07), "rf_mlp_tact": (86, 7.50e-07), "rf_mlp_b1024": (87, 1.47e-07),
    "passed over": {"rf_cnn": (85, 8.87e-06)},  # (2.3e-7 under eps 1e-5: elements whose step eps decides)
}

# the cases the unmodified reference was run on: tests/golden/<name>.npz
FIXTURE_CASES = ("rf_mlp", "rf_loco")

LR = 1e-4            # plr of every test (the parameter bounds of tests/test_gpu_a2c.py::test_two_updates are sized for it)
ENTROPY_COEFF = 0.005
ADAM_EPS = 1e-8      # torch.optim.Adam's default: reinforce.py:26-29 hands optimizer_class no eps

# the 10 keys of Reinforce.update's info in the reference's order (reinforce.py:43-74)
INFO_KEYS = ["advs/mean", "advs/std", "advs/max", "advs/min", "Training/policy_loss", "ent",
             "logprob/mean", "logprob/std", "logprob/max", "logprob/min"]

BATCH_KEYS = ("obs", "acts", "advs", "estimate_returns")


def updates_of(case):
    return case.get("updates", 2)


def seeded_policy(networks, policies, case):
    """pf of a case as the starters build it (util.build_nets under the case's seed; its critic is dropped).
    `networks` / `policies`: vision4leg_amd.torchrl's modules or the unmodified reference's."""
    import util
    torch.manual_seed(case["seed"])
    pf, _ = util.build_nets(networks, policies, case)
    return pf


class ReinforceOracle(orc.PPOOracle):
    """Reinforce.update over a name -> tensor dict. No critic, no target policy: PPOOracle's other two dicts are an empty one and
    pf's own."""

    def __init__(self, kind, pf, S, mode="f32", entropy_coeff=ENTROPY_COEFF, max_norm=0.5, optimizer_class=torch.optim.Adam,
                 optimizer_kwargs=None):
        super().__init__(kind, pf, {}, pf, S, mode, entropy_coeff=entropy_coeff, max_norm=max_norm)
        self.optimizer_class, self.optimizer_kwargs = optimizer_class, dict(optimizer_kwargs or {})
        self.pf_opt = None

    def losses(self, obs, acts, advs_raw):
        """reinforce.py:38-61. -> (policy_loss, policy head output [n, A], the 10-key info without the loss)."""
        for k in self.pf_keys:
            self.pf[k].requires_grad_(True)
        # (reinforce.py:43-46 reads these four off the numpy batch, before the upload: numpy's std() is the population one)
        info = {"advs/mean": advs_raw.mean().item(), "advs/std": advs_raw.std(unbiased=False).item(),
                "advs/max": advs_raw.max().item(), "advs/min": advs_raw.min().item()}
        out = self.fwd({k: v for k, v in self.pf.items() if k != "logstd"}, obs, self.S, self.mode)
        mean, std, _ = orc.gaussian(out, self.pf["logstd"])
        log_probs, ent = orc.log_prob_entropy(mean, std, acts, self.tanh_action)
        advs = (advs_raw - advs_raw.mean()) / (advs_raw.std() + 1e-5)                    # reinforce.py:57
        assert log_probs.shape == advs.shape
        policy_loss = (-log_probs * advs).mean() - self.entropy_coeff * ent.mean()       # reinforce.py:60-61
        lp = log_probs.detach()
        info.update({"Training/policy_loss": policy_loss.item(), "ent": ent.mean().item(), "logprob/mean": lp.mean().item(),
                     "logprob/std": lp.std().item(), "logprob/max": lp.max().item(), "logprob/min": lp.min().item()})
        return policy_loss, out, info

    def _release(self):
        for k in self.pf_keys:
            self.pf[k].requires_grad_(False)

    def loss_grads(self, obs, acts, advs, est_rets=None):
        """One loss evaluation, nothing stepped: d(policy_loss)/d(head output) [n, A], /d(logstd) [A] and the info."""
        policy_loss, out, info = self.losses(obs, acts, advs)
        dout, dls = torch.autograd.grad(policy_loss, [out, self.pf["logstd"]])
        self._release()
        return dout, dls.reshape(-1), info

    def update(self, obs, acts, advs, est_rets, lr_pf):
        """obs [B, D], acts [B, A], advs [B, 1] (est_rets is in the batch and unused, as in the reference). Returns the 10-key
        info (reinforce.py:43-74)."""
        tensors = [self.pf[k] for k in self.pf_keys]
        if self.pf_opt is None:  # reinforce.py:26-29
            self.pf_opt = self.optimizer_class(tensors, lr=lr_pf, **self.optimizer_kwargs)
        self.pf_opt.param_groups[0]["lr"] = lr_pf
        self.step += 1
        policy_loss, _, info = self.losses(obs, acts, advs)
        gp = self._grads(policy_loss, self.pf, self.pf_keys, obs.shape[0])
        self.last_grads["pf"] = dict(zip(self.pf_keys, gp))
        gp, gn = orc.clip_grad_norm(gp, self.max_norm)                                   # reinforce.py:65
        for p, g in zip(tensors, gp):
            p.grad = g.detach().clone()
        self.pf_opt.step()
        for p in tensors:
            p.grad = None
        self.grad_norm = gn.item()
        return info


def loss_stage64(rows, logstd, acts, advs, A, ent_coef=ENTROPY_COEFF, tanh=False):
    """The REINFORCE loss launch alone (reinforce.py:52-61, 69-74) in float64, by autograd, on given head rows. rows: [n, >= A]
    head outputs of the policy (the fp32 values the engine's forward left); logstd [A] (raw: the clamp is part of the stage);
    acts [n, A]; advs [n] raw. -> d(loss)/d(head output) [n, A], d(loss)/d(logstd) [A], the 10-key info."""
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    out = t(rows)[:, :A].clone().requires_grad_(True)
    ls = t(logstd).reshape(1, A).clone().requires_grad_(True)
    acts, advs_raw = t(acts).reshape(-1, A), t(advs).reshape(-1, 1)
    mean, std, _ = orc.gaussian(out, ls.reshape(A))
    log_probs, ent = orc.log_prob_entropy(mean, std, acts, tanh)
    advs = (advs_raw - advs_raw.mean()) / (advs_raw.std() + 1e-5)
    policy_loss = (-log_probs * advs).mean() - ent_coef * ent.mean()
    dout, dls = torch.autograd.grad(policy_loss, [out, ls])
    lp = log_probs.detach()
    info = {"advs/mean": advs_raw.mean().item(), "advs/std": advs_raw.std(unbiased=False).item(), "advs/max": advs_raw.max().item(),
            "advs/min": advs_raw.min().item(), "Training/policy_loss": policy_loss.item(), "ent": ent.mean().item(),
            "logprob/mean": lp.mean().item(), "logprob/std": lp.std().item(), "logprob/max": lp.max().item(),
            "logprob/min": lp.min().item()}
    return dout, dls.reshape(-1), info


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


def oracle_of(pf_sd, case, mode="f32", dtype=torch.float32, **kw):
    """A ReinforceOracle on a copy of a state_dict."""
    opf = {k: v.detach().cpu().clone().to(dtype) for k, v in pf_sd.items()}
    return ReinforceOracle(case["kind"], opf, case["S"], mode, **kw)


def fresh_oracle(case, mode="f32", dtype=torch.float32, init=None):
    """A ReinforceOracle on the case's seeded initial parameters (init: a pf state_dict to start from instead)."""
    if init is None:
        import vision4leg_amd.torchrl.networks as networks
        import vision4leg_amd.torchrl.policies as policies
        init = seeded_policy(networks, policies, case).state_dict()
    return oracle_of(init, case, mode, dtype)
