"""-m gpu: the sampling epilogue of every rollout-step route against the float64 restatement of tests/ppo_ref64.py, with a log sigma
and a mean that differ per action column.

The epilogue (clamp logstd, action = mean + std * eps [through tanh], log pi_old, entropy, filing at rollout slot t * E + i) exists
once per step kernel, and each copy maps lanes or MFMA columns to action dimensions in its own way. A freshly built policy has the
same log sigma in every column, far from both clamp bounds, and means ~ 1e-2: a kernel that reads column a's sigma from another
lane, skips the clamp or misplaces a bias column computes the same numbers on it. util.spread_policy_head gives every column its
own log sigma (below, at and above both clamp bounds, and inside) and its own O(1) mean.

Each test builds one net pair, attaches rollout arrays filled with a sentinel, runs two exploring steps and one deterministic
step on engine.HipActor (eager launches) and checks per step, against what the kernel itself consumed (actor.eps) and returned:
  a. std = exp(clamp(logstd, -5, 2)) within 4 EPS32 std (expf: 1 ulp), the same in every row, and bit-equal between a column
     beyond a clamp bound and the column at the bound;
  b. mean / value against the layer-by-layer pf(ob) / vf(ob) (test_gpu_parity.py::_actor_vs_separate's tolerances);
  c. action against sample_stage on the kernel's own mean and eps; the deterministic action bit-equals the mean (tanh: tanh of it);
  d. entropy against sum_a 0.5 + log(2 pi) / 2 + clamp(logstd_a), all rows equal;
  e. the stored log pi_old against log_prob_entropy(mean, the raw logstd parameter, the stored action) in float64;
  f. slots [s E, (s + 1) E) of acts / vals bit-equal to the step's outputs, every other slot of acts / vals / logp untouched.
c - e are bounds on fp32 rounding: ROLLOUT_C * EPS32 * sample_stage_bounds (the magnitudes that enter each quantity). The
constant is measured, not chosen from the kernels: tests/test_ref64_cpu.py::test_sample_stage_fp32_needs_less_than_the_gate runs
an fp32 numpy restatement on the same log sigma columns (257 x 16, seeds 0-2) and finds the stored log-prob at 0.58 of the bound
at c = 1 without tanh, 0.43 with (entropy 0.27 / 0.44, action 2.7 / 1.6); ROLLOUT_C = max(4, 4 x 0.58) = 4. No row is excluded
from any comparison; the tanh cases assert |action| < 1 on every stored element (log sigma capped at 0 is what makes the float64
reference finite there). Every ratio (error / bound, worst of the three steps) goes to util.record("rollout_epilogue/<id>/<what>").

Routes follow step_route (csrc/v4l_hip.hip); the second step runs under the library's profiler and must log the label family
that tests/test_gpu_rollout_route.py's table holds for a configuration of the same route (on the layer-by-layer route the
phase|op part: a linear layer's GEMM kernel follows the row count; labels carry no template arguments
and rollout_mlp2_kernel / rollout_mlp_kernel share the label rollout_mlp: which of the two runs follows from step_route's
conditions, stated next to each case).

infer_layer_kernel's copy of the epilogue (csrc/infer.h) has no case: its only launch site (forward_t's block-cooperative layer
pass in csrc/v4l_hip.hip) passes a zeroed InfFinish, so no step_route outcome reaches it with fin.ctl set."""
import numpy as np
import pytest
import torch

import ppo_ref64 as ref
import util
from test_gpu_parity import _build
from test_gpu_rollout_route import ROUTES, profile_step

pytestmark = pytest.mark.gpu

EPS, C = ref.EPS32, ref.ROLLOUT_C
SENTINEL = -7.0
GEOMETRY = {"mlp": "mlp_s93", "mlp_tanh": "mlp_tanh", "cnn": "cnn_s93", "cnn_vis": "cnn_vis", "loco": "loco_s84",
            "loco_tanh": "loco_tanh", "loco_vis": "loco_vis"}   # the shipped 256-wide nets of util.CASES


def _cases():
    """(route, kind, mode, shared_encoder, E, A, logstd override | None, dense_split, key of ROUTES with this route's labels)"""
    out = []
    add = lambda route, kind, mode, shared, E, A, like, logstd=None, split=False: out.append(
        (route, kind, mode, shared, E, A, logstd, split, like))
    # MLP_ONE_BLOCK (rollout_mlp2_kernel): state MLP, 16-bit mode, E <= 64, A <= 16, no tanh. One block per net, all E rows as
    # 16-row MFMA tiles: E = 5 a single ragged tile, E = 64 the limit (four full tiles); sigma per column from sg_s[k]
    for A, ls in ((1, [-6.5]), (1, [0.3]), (6, None), (16, None)):
        add("mlp_one_block", "mlp", "bf16", True, 5, A, "mlp_s93/bf16/shared", ls)
    for A in (6, 16):
        add("mlp_one_block", "mlp", "bf16", True, 64, A, "mlp_s93/bf16/shared")
    for E in (5, 64):
        add("mlp_one_block", "mlp", "f16", True, E, 6, "mlp_s93/f16/shared")
    # MLP_PER_SAMPLE (rollout_mlp_kernel, one block per (sample, net), thread 0 loops over the columns): fp32 mode; E = 65, the
    # first count past the one-block limit; a tanh policy (the one-block kernel has no tanh epilogue)
    add("mlp_per_sample", "mlp", "f32", True, 5, 6, "mlp_s93/f32/shared")
    for A in (6, 16):
        add("mlp_per_sample", "mlp", "bf16", True, 65, A, "mlp_s93/bf16/shared")
    add("mlp_per_sample", "mlp_tanh", "bf16", True, 5, 6, "mlp_tanh/bf16/shared")
    # CNN_DENSE (rollout_encoder2_kernel + rollout_dense_kernel): NatureCNN, 16-bit, E <= 64, no tanh. cnn: the fuse net's
    # launch (projector stage, FUSE = true), cnn_vis: the vision-only launch (FUSE = false). The finishing block walks the
    # rows 16 at a time, a (row, column) pair per lane: E = 5 one ragged tile, E = 33 a second tile holding one row
    for kind, like in (("cnn", "cnn_s93"), ("cnn_vis", "cnn_vis")):
        for E in (5, 33):
            for A in (6, 16):
                add("cnn_dense", kind, "bf16", True, E, A, like + "/bf16/shared")
        add("cnn_dense", kind, "f16", True, 33, 6, like + "/f16/shared")
    # CNN_DENSE as separate launches (V4L_ROLLOUT_DENSE_SPLIT=1): rollout_linear_kernel x 2 + rollout_head_kernel, thread i = env i
    for A in (6, 16):
        add("cnn_dense_split", "cnn", "bf16", True, 33, A, "cnn_s93/bf16/shared/dense_split", split=True)
    # CNN_PER_SAMPLE (rollout_cnn_kernel): fp32 mode; E = 65, the first count past the dense limit
    add("cnn_per_sample", "cnn", "f32", True, 5, 6, "cnn_s93/f32/shared")
    add("cnn_per_sample", "cnn", "bf16", True, 65, 6, "cnn_s93/f32/shared")
    # STACK_TOK17 (16-bit) / STACK_F32ENC (fp32) (rollout_stack_kernel, 2 * round_up(E, 4) blocks, lane a of wave 0 = column a):
    # E = 5 leaves three padded block pairs that must file nothing; tanh policies stay on this kernel
    for A, ls in ((1, [-6.5]), (1, [0.3]), (6, None), (16, None)):
        add("stack", "loco", "bf16", True, 5, A, "loco_s84/bf16/shared", ls)
    add("stack", "loco", "f16", True, 5, 6, "loco_s84/f16/shared")
    add("stack", "loco", "f32", True, 5, 6, "loco_s84/f32/shared")
    add("stack", "loco_tanh", "bf16", True, 5, 6, "loco_tanh/bf16/shared")
    # STACK_TOK16: the vision-only Transformer's 16-token instantiation
    add("stack_tok16", "loco_vis", "bf16", True, 5, 6, "loco_vis/bf16/shared")
    # GENERAL (shared_encoder = False: layer by layer + act_begin_kernel / act_finish_kernel, one 256-thread block looping
    # i += 256): E = 257 runs the second trip, on the cheapest net; a tanh policy on the LocoTransformer
    for mode in ("f32", "bf16"):
        add("general", "mlp", mode, False, 257, 6, "mlp_s93/%s/own" % mode)
    add("general", "loco_tanh", "bf16", False, 5, 6, "loco_tanh/bf16/own")
    return out


def _id(c):
    route, kind, mode, _, E, A, ls, _, _ = c
    return "%s-%s-%s-E%d-A%d%s" % (route, kind, mode, E, A, "" if ls is None else "-ls%g" % ls[0])


def _ratio(err, bound):
    """max of err / bound; an element with err == 0 passes whatever its bound (0 / 0: eps = 0 at mean = 0)."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    return float(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300)).max())


@pytest.mark.parametrize("cfg", _cases(), ids=[_id(c) for c in _cases()])
def test_rollout_epilogue(cfg, device, monkeypatch):
    from vision4leg_amd import engine
    route, kind, mode, shared, E, A, ls_override, split, like = cfg
    if split:
        monkeypatch.setenv("V4L_ROLLOUT_DENSE_SPLIT", "1")
    else:
        monkeypatch.delenv("V4L_ROLLOUT_DENSE_SPLIT", raising=False)
    case = dict(util.CASES[GEOMETRY[kind]], A=A)
    tanh = kind.endswith("_tanh")
    pf, vf = _build(case, mode, device)
    logstd, bias = util.spread_policy_head(pf, ls_override)
    assert len(set(bias.tolist())) == A and logstd.shape == (A,)
    ls64 = logstd.astype(np.float64)
    net = pf.hip
    net.ensure_bound()
    T = 3
    slots = (T + 1) * E  # one step's worth of slots past the last step: a spill behind the rollout would land there
    state, image = net.alloc_rollout(slots, device)
    acts = torch.full((slots, A), SENTINEL, device=device)
    vals, logp = torch.full((slots,), SENTINEL, device=device), torch.full((slots,), SENTINEL, device=device)
    want_acts, want_vals, want_logp = acts.clone(), vals.clone(), logp.clone()
    obs = torch.tensor(util.obs_rows(np.random.RandomState(3), T * E, case), dtype=torch.float32, device=device)
    actor = engine.HipActor(pf.hip, vf.hip, E, shared_encoder=shared, graph=False)
    actor.attach((state, image, acts, vals, logp))
    actor.seek(0)
    tol = 1e-5 if mode == "f32" else 4e-3  # (b): _actor_vs_separate's
    worst = {}
    f64 = lambda t: t.detach().double().cpu().numpy()
    for s in range(T):
        det = s == T - 1
        ob = obs[s * E:(s + 1) * E]
        torch.manual_seed(100 + s)
        if s == 1:  # the route, by the labels one step logs
            got, want = ([r[0] for r in rows] for rows in (profile_step(actor, ob), ROUTES[like][1]))
            if route == "general":  # which GEMM kernel a linear layer takes depends on the row count: phase|op there
                assert got[-1] == want[-1] == "rollout|sample|act_finish"
                got, want = ([x.rsplit("|", 1)[0] for x in v] for v in (got, want))
            assert got == want, (like, got)
        else:
            actor.step(ob, deterministic=det)
        torch.cuda.synchronize()
        out = {k: v.clone() for k, v in actor._out.items()}
        eps = actor.eps.clone()
        assert tuple(eps.shape) == (E, A) and (bool((eps == 0).all()) == det)
        sl = slice(s * E, (s + 1) * E)
        mean, std, action, ent, value = (f64(out[k]) for k in ("mean", "std", "action", "ent", "value"))
        ent, value = ent.reshape(E), value.reshape(E)
        stored_a, stored_lp = f64(acts[sl]), f64(logp[sl])
        with torch.no_grad():
            sep_mean, _, _ = pf(ob)
            sep_value = vf(ob)
        sep_mean, sep_value = f64(sep_mean), f64(sep_value).reshape(E)
        std64, _, act64, ent64 = (x.numpy() for x in ref.sample_stage(mean, ls64, f64(eps), tanh))
        lp64 = ref.log_prob_entropy(torch.tensor(mean), torch.tensor(ls64), torch.tensor(stored_a), tanh)[0].numpy()
        b = {k: v.numpy() for k, v in ref.sample_stage_bounds(mean, ls64, f64(eps), stored_a, tanh).items()}
        r = {"std": _ratio(np.abs(std - std64), 4 * EPS * std64),
             "mean": _ratio(np.abs(mean - sep_mean).max(), tol * max(1.0, np.abs(sep_mean).max())),
             "value": _ratio(np.abs(value - sep_value).max(), tol * max(1.0, np.abs(sep_value).max())),
             "action": _ratio(np.abs(action - act64), C * EPS * b["action"]),
             "ent": _ratio(np.abs(ent - ent64), C * EPS * b["ent"]),
             "logp": _ratio(np.abs(stored_lp - lp64), C * EPS * b["logp"])}
        print("\n[rollout epilogue %s step %d%s] error / bound: %s" % (_id(cfg), s, " (deterministic)" if det else "",
                                                                     " ".join("%s %.3f" % kv for kv in r.items())))
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
            util.record("rollout_epilogue/%s/%s" % (_id(cfg), k), worst[k])
        # condition on the inputs (tanh): every stored action strictly inside (-1, 1), the float64 reference finite
        if tanh:
            assert np.abs(stored_a).max() < 1.0
        assert np.isfinite(lp64).all() and np.isfinite(stored_lp).all()
        # a. std
        assert r["std"] <= 1.0, (s, std[0], std64[0])
        assert (std == std[:1]).all()
        for bound, beyond in ((ref.LOG_SIG_MIN, ls64 < ref.LOG_SIG_MIN), (ref.LOG_SIG_MAX, ls64 > ref.LOG_SIG_MAX)):
            at = np.flatnonzero(ls64 == bound)
            for a in np.flatnonzero(beyond) if len(at) else []:
                assert std[0, a] == std[0, at[0]], (s, a, ls64[a], std[0, a], std[0, at[0]])
        # b. mean / value
        assert r["mean"] <= 1.0 and r["value"] <= 1.0, (s, r["mean"], r["value"])
        # c. action
        assert r["action"] <= 1.0, (s, r["action"])
        if det and not tanh:
            assert torch.equal(out["action"], out["mean"])
        # d. entropy
        assert r["ent"] <= 1.0, (s, ent[0], ent64[0])
        assert (ent == ent[0]).all()
        # e. stored log pi_old
        assert r["logp"] <= 1.0, (s, r["logp"], stored_lp, lp64)
        # f. filing: this step's slots hold its outputs, every other slot what it held before
        want_acts[sl], want_vals[sl], want_logp[sl] = out["action"], out["value"].view(E), logp[sl]
        assert torch.equal(acts, want_acts) and torch.equal(vals, want_vals) and torch.equal(logp, want_logp), s
        assert bool((logp[sl] != SENTINEL).all())
        assert bool((acts[(s + 1) * E:] == SENTINEL).all()) and bool((vals[(s + 1) * E:] == SENTINEL).all())
        assert bool((logp[(s + 1) * E:] == SENTINEL).all())


def test_graph_replay_advances_the_cursor_past_padded_blocks(device):
    """Graph replays cannot take the step index from the host (their arguments are frozen): the last block of the step's last
    kernel advances the device-side cursor. rollout_stack_kernel runs 2 * round_up(E, 4) blocks of which the padded ones leave at
    entry, so "last" is the 2 E-th arrival, not the grid size's: with E = 5 (16 blocks, 10 arrivals) a count against the grid
    size never closes the first step and every step files at slot 0. Four replayed steps must file at slots [s E, (s + 1) E) and
    leave the sentinel everywhere else."""
    from vision4leg_amd import engine
    E, T = 5, 4
    case = util.CASES["loco_s84"]
    A = case["A"]
    pf, vf = _build(case, "bf16", device)
    util.spread_policy_head(pf)
    net = pf.hip
    net.ensure_bound()
    slots = (T + 1) * E
    state, image = net.alloc_rollout(slots, device)
    acts = torch.full((slots, A), SENTINEL, device=device)
    vals, logp = torch.full((slots,), SENTINEL, device=device), torch.full((slots,), SENTINEL, device=device)
    want_acts, want_vals = acts.clone(), vals.clone()
    obs = torch.tensor(util.obs_rows(np.random.RandomState(3), T * E, case), dtype=torch.float32, device=device)
    actor = engine.HipActor(pf.hip, vf.hip, E, shared_encoder=True, graph=True)
    actor.attach((state, image, acts, vals, logp))
    actor.seek(0)
    for s in range(T):
        torch.manual_seed(100 + s)
        out = {k: v.clone() for k, v in actor.step(obs[s * E:(s + 1) * E]).items()}
        torch.cuda.synchronize()
        sl = slice(s * E, (s + 1) * E)
        want_acts[sl], want_vals[sl] = out["action"], out["value"].view(E)
        assert torch.equal(acts, want_acts) and torch.equal(vals, want_vals), s
        assert bool((logp[:(s + 1) * E] != SENTINEL).all()) and bool((logp[(s + 1) * E:] == SENTINEL).all()), s
