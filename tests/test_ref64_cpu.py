"""CPU: the float64 loss / clip / Adam restatement the GPU loss-and-optimiser tests measure against (tests/ppo_ref64.py) is
pinned to the CPU oracle (oracle/ppo_oracle.py, itself pinned to the reference): on a small state-MLP, two PPO updates of the
oracle in f32 and of the restatement in float64 from the same parameters and batches must log the same 18 scalars, produce the
same parameter gradients and land on the same parameters, to fp32 noise. The second update runs against the frozen target of
the first, with a large learning rate, so its ratios leave the clip range on both sides. The sampling epilogue's restatement
(sample_stage) is pinned to the oracle's Gaussian head, and an fp32 restatement of it measures the constant of the GPU
rollout-epilogue tests' bounds (ppo_ref64.ROLLOUT_C)."""
import numpy as np
import pytest
import torch

import ppo_ref64 as ref
import util
from oracle import ppo_oracle as orc


def _nets(case):
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    torch.manual_seed(case["seed"])
    pf, vf = util.build_nets(networks, policies, case)
    opf = {k: v.detach().clone() for k, v in pf.state_dict().items()}
    ovf = util.share_encoder(opf, {k: v.detach().clone() for k, v in vf.state_dict().items()}, case["kind"])
    return opf, ovf


def _f64(p, kind):
    """float64 copies, keeping the shared-encoder tensor identity of the oracle's dicts."""
    out = {}
    memo = {}
    for k, v in p.items():
        if id(v) not in memo:
            memo[id(v)] = v.detach().double().clone()
        out[k] = memo[id(v)]
    return out


@pytest.mark.parametrize("A,clipped,tanh", [(3, False, False), (1, False, False), (2, True, False), (3, False, True)])
def test_ref64_matches_oracle(A, clipped, tanh):
    kind = "mlp_tanh" if tanh else "mlp"
    case = dict(kind=kind, S=13, A=A, seed=40 + A, B=24, enc=[32, 32], head=[32])
    opf, ovf = _nets(case)
    opf["logstd"].copy_(torch.linspace(-1.0, 0.5, A))
    oracle = orc.PPOOracle(kind, opf, ovf, {k: v.clone() for k, v in opf.items()}, case["S"], "f32",
                           clipped_value_loss=clipped)
    oracle.sync_target()
    # float64 side: its own parameter copies (pf / vf sharing the encoder tensors), frozen target, two Adams
    rpf = _f64(opf, kind)
    rvf = {k: (rpf[k] if ovf[k] is opf.get(k) else v.detach().double().clone()) for k, v in ovf.items()}
    rtpf = {k: v.clone() for k, v in rpf.items()}
    opt_pf = ref.Adam([rpf[k] for k in rpf])
    opt_vf = ref.Adam([rvf[k] for k in rvf])
    fwd = orc.FORWARDS["mlp"]
    rs = np.random.RandomState(A)
    lr = 3e-2  # large: the second update's ratios spread far beyond 1 +- clip
    for u in range(2):
        B = case["B"]
        obs = rs.randn(B, case["S"])
        acts = np.clip(0.6 * rs.randn(B, A), -0.95, 0.95)
        advs = 2.0 + rs.randn(B, 1)
        rets = rs.randn(B, 1)
        vals = rs.randn(B, 1) * 0.3
        t = lambda a: torch.tensor(a, dtype=torch.float32)
        oinfo = oracle.update(t(obs), t(acts), t(advs), t(rets), t(vals), lr, lr)
        q = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)  # the same fp32 inputs
        rinfo, rgrads = ref.ppo_update(fwd, rpf, rvf, rtpf, q(obs), q(acts), q(advs), q(rets), q(vals), lr, lr, opt_pf, opt_vf,
                                       case["S"], clipped_value_loss=clipped, tanh_action=tanh)
        for k in ref.STAT_KEYS:
            a, b = oinfo[k], rinfo[k]
            if A == 1 and k == "log_std/std":
                assert np.isnan(a) and np.isnan(b), (k, a, b)   # torch's std() of one element
                continue
            assert abs(a - b) <= 2e-5 * max(1.0, abs(b)), (u, k, a, b)
        if u == 1:
            assert rinfo["ratio/max"] > 1.3 and rinfo["ratio/min"] < 0.7, (rinfo["ratio/max"], rinfo["ratio/min"])
        for tag in ("pf", "vf"):
            for k, g in rgrads[tag].items():
                og = oracle.last_grads[tag][k]
                assert util.rel_err(og, g) <= 1e-4, (u, tag, k, util.rel_err(og, g))
        # one Adam step moves an element by ~lr: fp32 noise of the oracle stays far below 1e-4 of it
        for k in opf:
            d = (opf[k].double() - rpf[k]).abs().max().item()
            assert d <= 1e-4 * lr * (u + 1) + 1e-6, (u, "pf", k, d)
        for k in ovf:
            d = (ovf[k].double() - rvf[k]).abs().max().item()
            assert d <= 1e-4 * lr * (u + 1) + 1e-6, (u, "vf", k, d)


def test_loss_stage_gradients_match_finite_differences():
    """The output-level gradients loss_stage returns (d/d values, d/d mean, d/d logstd) against central differences of its own
    losses, on rows inside and outside both clip ranges and logstd entries below, inside and above the clamp."""
    rs = np.random.RandomState(7)
    n, A = 9, 4
    mean = 0.3 * rs.randn(n, A)
    logstd = np.array([-6.0, -1.0, 0.5, 3.0])
    acts = mean + np.exp(np.clip(logstd, -5.0, 2.0)) * rs.randn(n, A)
    lp, _, _ = ref.log_prob_entropy(torch.tensor(mean), torch.tensor(logstd), torch.tensor(acts))
    logp_old = lp.numpy() - rs.uniform(np.log(0.3), np.log(3.0), n)  # ratios 0.3 .. 3
    advs = 3.0 + rs.randn(n)
    vals, rets, old = rs.randn(n), rs.randn(n), rs.randn(n)
    for clipped in (False, True):
        out = ref.loss_stage(vals, rets, old, mean, logstd, acts, logp_old, advs, clipped_value_loss=clipped)

        def pl(m, ls):
            an, _ = ref.normalise_advantages(torch.tensor(advs))
            return ref.actor_loss(torch.tensor(m), torch.tensor(ls), torch.tensor(acts), torch.tensor(logp_old), an)[0].item()

        h = 1e-6
        for i in range(n):
            for a in range(A):
                mp, mm = mean.copy(), mean.copy()
                mp[i, a] += h
                mm[i, a] -= h
                fd = (pl(mp, logstd) - pl(mm, logstd)) / (2 * h)
                assert abs(fd - out["dmean"][i, a].item()) <= 1e-6 * max(1.0, abs(fd)), (i, a)
            vp, vm = vals.copy(), vals.copy()
            vp[i] += h
            vm[i] -= h
            cl = lambda v: ref.critic_loss(torch.tensor(v), torch.tensor(rets), torch.tensor(old), 0.2, clipped).item()
            fd = (cl(vp) - cl(vm)) / (2 * h)
            assert abs(fd - out["dvalues"][i].item()) <= 1e-6 * max(1.0, abs(fd)), i
        for a in (1, 2):  # inside the clamp: finite differences; outside it the gradient is exactly 0
            lp_, lm_ = logstd.copy(), logstd.copy()
            lp_[a] += h
            lm_[a] -= h
            fd = (pl(mean, lp_) - pl(mean, lm_)) / (2 * h)
            assert abs(fd - out["dlogstd"][a].item()) <= 1e-6 * max(1.0, abs(fd)), a
        assert out["dlogstd"][0].item() == 0.0 and out["dlogstd"][3].item() == 0.0


@pytest.mark.parametrize("A,tanh", [(16, False), (16, True), (1, False), (6, True)])
def test_sample_stage_matches_oracle(A, tanh):
    """ppo_ref64.sample_stage (+ log_prob_entropy on the action it returns) against the oracle's Gaussian head evaluated in
    float64 on the same numbers (oracle gaussian: clamp / exp / broadcast; oracle log_prob_entropy: takes that std), with a log
    sigma per column on both sides of both clamp bounds."""
    rs = np.random.RandomState(60 + A)
    n = 9
    mean = torch.tensor(rs.uniform(-1.5, 1.5, (n, A)))
    eps = torch.tensor(rs.randn(n, A))
    logstd = torch.tensor(util.logstd_columns(A, tanh)).double()
    std, pre, action, ent = ref.sample_stage(mean, logstd, eps, tanh)
    _, ostd, olog_std = orc.gaussian(mean, logstd)
    assert std.dtype == torch.float64 and torch.equal(std, ostd)
    opre = mean + ostd * eps
    assert torch.equal(pre, opre) and torch.equal(action, torch.tanh(opre) if tanh else opre)
    if tanh:
        assert action.abs().max().item() < 1.0
    lp, ent2, log_std = ref.log_prob_entropy(mean, logstd, action, tanh)
    olp, oent = orc.log_prob_entropy(mean, ostd, action, tanh)
    assert torch.equal(log_std, olog_std)
    # (log(exp(x)) against x, sums in another order: float64 rounding)
    assert (lp - olp.reshape(-1)).abs().max().item() <= 1e-12 * olp.abs().max().item()
    assert (ent - oent.reshape(-1)).abs().max().item() <= 1e-12 * oent.abs().max().item()
    assert (ent2 - oent.reshape(-1)).abs().max().item() <= 1e-12 * oent.abs().max().item()
    # the clamp is what the columns beyond a bound see
    at = lambda v: ref.sample_stage(mean[:, :1], torch.tensor([v]).double(), eps[:, :1], tanh)[0][0, 0].item()
    for a, v in enumerate(logstd.tolist()):
        assert std[0, a].item() == at(min(max(v, -5.0), 2.0))


def test_sample_stage_fp32_needs_less_than_the_gate():
    """What multiple of sample_stage_bounds does fp32 arithmetic itself need? sample_stage_f32 (numpy, one rounding per operation)
    against the float64 functions, on the log sigma columns the GPU rollout-epilogue tests use, mean ~ U[-1.5, 1.5], eps ~ N(0, 1),
    257 rows x 16 columns, seeds 0-2, with and without tanh. Measured on the CPU: the stored action's log-prob reaches 0.58
    (0.43 with tanh) of the bound at c = 1, the entropy 0.27 (0.44), the action 2.7 (1.6: numpy's expf is off by up to one ulp,
    which is 2 EPS32 of std * eps). The GPU tests' constant is ROLLOUT_C = max(4, 4 x the log-prob's worst ratio): the factor 4
    is for the device's 1-2 ulp expf / logf / tanhf against numpy's and for other multiply-add orders."""
    worst = {"action": 0.0, "ent": 0.0, "logp": 0.0}
    for tanh in (False, True):
        logstd = util.logstd_columns(16, tanh)
        for seed in range(3):
            rs = np.random.RandomState(seed)
            mean = rs.uniform(-1.5, 1.5, (257, 16)).astype(np.float32)
            eps = rs.randn(257, 16).astype(np.float32)
            act, ent, lp = ref.sample_stage_f32(mean, logstd, eps, tanh)
            if tanh:
                assert np.abs(act).max() < 1.0   # a condition on the inputs: the float64 log-prob of every stored action is finite
            _, _, act64, ent64 = ref.sample_stage(mean, logstd, eps, tanh)
            lp64, _, _ = ref.log_prob_entropy(torch.tensor(mean).double(), torch.tensor(logstd).double(),
                                              torch.tensor(act).double(), tanh)
            b = ref.sample_stage_bounds(mean, logstd, eps, act, tanh)
            for what, got, want in (("action", act, act64), ("ent", ent, ent64), ("logp", lp, lp64)):
                r = float((np.abs(got - want.numpy()) / (ref.EPS32 * b[what].numpy())).max())
                worst[what] = max(worst[what], r)
    print("\n[sample_stage fp32 / bound at c = 1] action %.3f ent %.3f logp %.3f" % (worst["action"], worst["ent"], worst["logp"]))
    assert np.isfinite(list(worst.values())).all() and worst["logp"] > 0.05  # (a measurement, not zeros)
    assert ref.ROLLOUT_C >= 4.0 and 4 * worst["logp"] <= ref.ROLLOUT_C
    assert max(worst.values()) <= ref.ROLLOUT_C  # (fp32 numpy itself passes every gate the GPU tests set)
