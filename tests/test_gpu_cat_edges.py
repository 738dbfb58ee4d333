"""-m gpu: the categorical head, sampler, loss and rollout-epilogue kernels (csrc/elem.h: cat_head_kernel, cat_sample_kernel,
a2c_cat_loss_kernel / reinforce_cat_loss_kernel, act_finish_cat_kernel) on saturated rows and at the batch sizes where their
launches change, against the float64 reference of tests/cat_edge_cases.py.

tests/test_gpu_cat.py keeps every probability in [1e-6, 0.99] and every batch at 64 rows or fewer. Here the rows are those of a
policy that has trained for a while — logit gaps of 20 .. 500, probabilities below fp32 eps and exactly 0, a last class the
policy has given up — plus hand-built rows (gaps of 0 .. 1e4, exact ties), and the sizes straddle the 256-row blocks of the head
and sampler kernels, the 256 -> 1024 thread switch of the loss launches at n = 512 with the second trip of their row loops, and
the second trip of the one-block rollout epilogue past E = 256.

Every comparison is teacher-forced on the engine's OWN fp32 logits (read from the forward or the `out` workspace view), so no
gate depends on the compute mode: each is EPS32 = 2^-24 times the magnitudes that enter the quantity (cat_edge_cases "Gates";
tests/test_cat_edges_cpu.py holds an fp32 numpy restatement of the kernels to the same gates). 16-bit forwards move the logits,
so each test re-asserts the row kinds on the logits it got, at half the CPU share.

The sampler: a uniform of 1 - 2^-24 (torch.rand returns multiples of 2^-24) on a row whose fp32 running sum ends at or below it
finds no running sum that exceeds it. cat_pick then returns the last class of POSITIVE probability; it used to return K - 1,
a class of probability exactly 0 on the hard cases, whose log pi of -150 and below the rollout step filed. The p(action) > 0
statements of test_sampler_fallback_and_ties and test_rollout_step_on_saturated_rows are the ones that arithmetic fails.

Worst error / gate per quantity goes to util.record("cat_edges/...")."""
import os

import numpy as np
import pytest
import torch

import test_gpu_parity as par
import util
import cat_cases as cc
import cat_edge_cases as ce
from cat_edge_cases import EDGE_CASES

pytestmark = pytest.mark.gpu

MODES = par.MODES
NAMES = list(EDGE_CASES)
LEARNERS = ("a2c", "rf")
SENT = -7.0
GPU_SHARE = ce.KIND_SHARE / 2


class _Coll:
    epoch_frames = 1


def _build(case, mode, dev):
    os.environ["V4L_COMPUTE"] = mode
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    pf, vf = ce.seeded_nets(networks, policies, case)
    return pf.to(dev), vf.to(dev)


def _agent(learner, case, mode, device):
    """tests/test_gpu_cat.py::_agent on an edge case's pair."""
    from vision4leg_amd.torchrl.algo import A2C, Reinforce
    pf, vf = _build(case, mode, device)
    args = dict(plr=cc.LR, tau=0.95, shuffle=True, entropy_coeff=ce.ENT_COEF, env=None, replay_buffer=None, collector=_Coll(),
                logger=None, device=device, discount=0.99, num_epochs=1500, batch_size=case["B"], save_dir=None)
    if learner == "a2c":
        return A2C(pf=pf, vf=vf, vlr=cc.LR, **args), pf, vf
    agent = Reinforce(pf=pf, **args)
    return agent, pf, agent.vf


def _up(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)


def _own_logits(pf, name, device):
    """The engine's padded logits rows [POOL_N][16] of the case's pool observations (a clone: the forward's output is a workspace
    view), with the row kinds re-asserted on them."""
    K = EDGE_CASES[name]["K"]
    obs = _up(ce.batch(name, ce.POOL_N)["obs"], device)
    hip = pf.hip
    st, im, _ = hip.stage(obs)
    out = hip.forward(st, im, ce.POOL_N).clone()
    torch.cuda.synchronize()
    assert tuple(out.shape) == (ce.POOL_N, 16) and bool((out[:, K:] == 0).all())
    ce.check_kinds(name, out[:, :K].cpu().numpy(), GPU_SHARE)
    return out


def _record(tag, worst):
    for k, v in worst.items():
        util.record("cat_edges/%s/%s_err_over_gate" % (tag, k), v)


# ------------------------------------------------------------------------------------------ head
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_head_on_saturated_rows(name, mode, device):
    """hip.cat_head on padded [n][16] rows — the crafted rows (cat_edge_cases.crafted_logits: gaps of 0, 16, 17, 88, 104, 200,
    1e4, exact ties; their padding columns hold 9e9, which the kernel must not read into the distribution), then the case's own
    logits — at n = 1, 255, 256, 257 and 4097: probabilities, the log-prob of EVERY index and the entropy against head64
    through the gates; p.sum(1) within K EPS32 of 1; nothing NaN or Inf; and, through the C entry with sentinel-filled buffers
    three rows longer than n, nothing written past row n."""
    from vision4leg_amd import engine
    case = EDGE_CASES[name]
    K = case["K"]
    pf, _ = _build(case, mode, device)
    worst = {}
    with torch.cuda.device(device):
        hip = pf.hip
        own = _own_logits(pf, name, device)
        crafted = np.full((len(ce.crafted_logits(K)), 16), 9e9, dtype=np.float32)
        crafted[:, :K] = ce.crafted_logits(K)
        pool = torch.cat([_up(crafted, device), own])
        for n in ce.HEAD_NS:
            rows = pool[torch.arange(n, device=device) % len(pool)].contiguous()
            z = rows[:, :K].cpu().numpy()
            h = ce.head64(z)
            g = ce.head_gates(h)
            lg = np.empty((n, K))
            for j in range(K):
                acts = torch.full((n,), float(j), device=device)
                probs, ent, logp = hip.cat_head(rows, n, acts)
                lg[:, j] = logp.double().cpu().numpy()
            p, ent = probs.double().cpu().numpy(), ent.double().cpu().numpy()
            assert np.isfinite(p).all() and np.isfinite(lg).all() and np.isfinite(ent).all()
            r = ce.head_ratios(p, lg, ent, h)
            print("\n[%s %s n=%d] error / gate: %s" % (name, mode, n, " ".join("%s %.3f" % kv for kv in r.items())))
            for k, v in r.items():
                worst[k] = max(worst.get(k, 0.0), v)
            assert max(r.values()) <= 1.0, (n, r)
            assert np.abs(p.sum(axis=1) - 1.0).max() <= K * ce.EPS32
            assert (p >= 0).all() and (ent >= 0).all() and (lg <= 0).all()
            # nothing past row n: the C entry on buffers of n + 3 rows
            pb = torch.full(((n + 3) * K,), SENT, device=device)
            eb, lb = torch.full((n + 3,), SENT, device=device), torch.full((n + 3,), SENT, device=device)
            engine.check(hip.L.v4l_cat_head(engine._ptr(rows), engine._ptr(acts), n, K, engine._ptr(pb), engine._ptr(eb),
                                            engine._ptr(lb), engine._stream()), "v4l_cat_head")
            torch.cuda.synchronize()
            assert torch.equal(pb[:n * K].view(n, K), probs) and torch.equal(lb[:n], logp)
            assert bool((pb[n * K:] == SENT).all()) and bool((eb[n:] == SENT).all()) and bool((lb[n:] == SENT).all())
    _record("head/%s/%s" % (name, mode), worst)


# ------------------------------------------------------------------------------------------ sampler
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_sampler_fallback_and_ties(name, mode, device):
    """engine.cat_sample on the crafted probability rows (exact in fp32: the stated index on every row, 3 — not K - 1 — on
    [1/4, 1/4, 1/4, 1/4 - 2^-24, 0 ..] at u = 1 - 2^-24) and on the case's own probabilities with u = 0, u = 1 - 2^-24 and
    seeded uniforms at n = 1, 256, 257, 4097: the index equals pick64 outside the 1e-6 band, lies between the picks of u -+ 1e-6
    on every row, and EVERY returned index has p > 0. The deterministic pick is the first maximum, also on rows with exact ties."""
    from vision4leg_amd import engine
    case = EDGE_CASES[name]
    K = case["K"]
    pf, _ = _build(case, mode, device)
    with torch.cuda.device(device):
        p, u, want = ce.crafted_probs(K)
        got = engine.cat_sample(_up(p, device), _up(u, device)).cpu().numpy()
        print("\n[%s %s] crafted rows: got %s, want %s" % (name, mode, got.tolist(), want.tolist()))
        tp, first = ce.tie_probs(K)
        assert engine.cat_sample(_up(tp, device), deterministic=True).cpu().numpy().tolist() == first.tolist()
        own = _own_logits(pf, name, device)
        probs = pf.hip.cat_head(own, ce.POOL_N)[0]
        inside = 0
        for n in ce.SAMPLE_NS:
            rows = probs[torch.arange(n, device=device) % ce.POOL_N].contiguous()
            rows_np = rows.cpu().numpy()
            det = engine.cat_sample(rows, deterministic=True).cpu().numpy()
            assert (det == rows_np.argmax(axis=1)).all()
            for what, un in (("0", np.zeros(n, dtype=np.float32)), ("1-2^-24", np.full(n, ce.U_MAX, dtype=np.float32)),
                             ("seeded", cc.uniforms(case, n)), ("mixed", ce.mixed_uniforms(case, n))):
                idx = engine.cat_sample(rows, _up(un, device)).cpu().numpy()
                wi, dist = ce.pick64(rows_np, un)
                clear = dist > ce.BAND
                lo, hi = ce.pick_range(rows_np, un)
                assert idx.min() >= 0 and idx.max() < K
                assert (rows_np[np.arange(n), idx] > 0).all(), (n, what, int((rows_np[np.arange(n), idx] == 0).sum()))
                assert (idx[clear] == wi[clear]).all(), (n, what)
                assert ((lo <= idx) & (idx <= hi)).all(), (n, what)
                if what == "seeded" and n == 4097:
                    inside = float((~clear).mean())
        print("   seeded uniforms, n = 4097: %.4f of the rows inside the boundary band" % inside)
        assert inside <= ce.BAND_SHARE
        # (last: with the K - 1 fall-back the statement above it that trips is p > 0 on the case's own rows)
        assert got.dtype == np.int64 and got.tolist() == want.tolist()
    util.record("cat_edges/sampler/%s/%s/band_share" % (name, mode), inside)


# ------------------------------------------------------------------------------------------ loss stage
def _loss_cases():
    return [(learner, name) for learner in LEARNERS for name in NAMES]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("learner,name", _loss_cases())
def test_loss_stage_vs_float64(learner, name, mode, device):
    """a2c_cat_loss_kernel / reinforce_cat_loss_kernel through the trainer's eager phases (begin -> [a2c_critic_grads] ->
    actor_grads, nothing stepped: tests/test_gpu_cat.py::test_loss_grads' sequence), one trainer sized for the largest n serving
    the sizes of cat_edge_cases.LOSS_NS in increasing order. Against loss64 on the logits (and values) the launches left in the
    workspace, through the gates: the d(out) rows unscaled by grad_scale, columns K .. 15 exactly zero, each row's sum, every slot
    of the learner's record and the mirrored slots of the PPO record. f16: rows the reference puts beyond 32768 / grad_scale are
    compared with the clamp and counted in record slot 23, as tests/test_gpu_loss_adam.py does; the count is zero where no
    reference row reaches the clamp."""
    from vision4leg_amd import _lib
    from vision4leg_amd.engine import HipTrainer
    ns = ce.LOSS_NS[name]
    case = ce.sized(EDGE_CASES[name], max(ns))
    K = case["K"]
    agent, pf, vf = _agent(learner, case, mode, device)
    tr = agent.trainer
    rec_keys = _lib.A2C_INFO_KEYS if learner == "a2c" else _lib.REINFORCE_INFO_KEYS
    S = _lib.STAT_KEYS.index
    worst = {}
    for n in ns:
        b = ce.batch(name, n)
        with torch.cuda.device(device):
            hip = pf.hip
            hip.ensure_bound()
            st, im = hip.alloc_rollout(n, device)
            hip.ingest(_up(b["obs"], device), st, im)
            ro = HipTrainer.rollout(st, im, _up(b["acts"], device).reshape(n, 1), _up(b["advs"], device).reshape(n),
                                    _up(b["rets"], device).reshape(n))
            stats = torch.zeros(1, _lib.V4L_STATS, dtype=torch.float32, device=device)
            tr._pre(n)
            tr.begin(None, stats, cc.LR, cc.LR)
            values = None
            if learner == "a2c":
                second = torch.zeros(1, _lib.V4L_A2C_STATS, dtype=torch.float32, device=device)
                tr.a2c_critic_grads(ro, n, second)
                values = vf.hip.ws_view(n, "out", n, 16, tr.ws)[:, 0].double().cpu().numpy()
                tr.a2c_actor_grads(ro, n, second)
            else:
                second = torch.zeros(1, _lib.V4L_REINFORCE_STATS, dtype=torch.float32, device=device)
                tr.reinforce_actor_grads(ro, n, second)
            torch.cuda.synchronize()
            out = hip.ws_view(n, "out", n, 16, tr.ws).cpu()
            gs = float(hip.grad_scale(n))
            rows = hip.ws_view(n, "dout", n, 16, tr.ws).double().cpu().numpy() / gs
            rec = second[0].double().cpu().numpy()
            ppo_rec = tr.stats_cur().double().cpu().numpy()
        assert bool((out[:, K:] == 0).all()) and (rows[:, K:] == 0).all()
        z = out[:, :K].numpy()
        if n >= 64:
            ce.check_kinds(name, z, GPU_SHARE)
            sub, zero = ce.acts_kinds(z, b["acts"])
            assert sub >= 1 and (zero >= 1 or "c" not in ce.REQUIRED[name])
        R = ce.loss64(z, b["acts"], b["advs"], values=values, rets=b["rets"])
        G = ce.loss_gates(R, b["advs"], values=values, rets=b["rets"])
        r = {}
        # the d(out) rows; f16: clamped at +-32768 / grad_scale, rows within their own gate of the clamp not compared
        rm, clamp = R["dz"], 32768.0 / gs
        sat = np.abs(rm) > clamp
        amb = np.abs(np.abs(rm) - clamp) <= G["dz"]
        if gs != 1.0:
            rm = np.where(sat, np.sign(rm) * clamp, rm)
        r["dz"] = ce.ratio(np.where(amb, 0.0, np.abs(rows[:, :K] - rm)), G["dz"])
        whole = ~(sat | amb).any(axis=1)
        r["rowsum"] = ce.ratio(np.abs(rows[whole, :K].sum(axis=1)), G["rowsum"][whole])
        nsat = int(ppo_rec[_lib.ST_F16_SAT])
        if gs == 1.0 or not (sat | amb).any():
            assert nsat == 0, nsat
        else:
            assert int(sat[~amb].sum()) <= nsat <= int((sat | amb).sum()), (nsat, int(sat.sum()))
        assert np.isfinite(rows).all() and np.isfinite(rec).all()
        # the learner's record
        for j, k in enumerate(rec_keys):
            if k in R[learner]:
                r[k] = ce.ratio(abs(rec[j] - R[learner][k]), G[learner][k])
            else:
                assert k.startswith("std/") and rec[j] == 0.0, k
        assert set(R[learner]) <= set(rec_keys) and (rec[len(rec_keys):] == 0).all()
        # the PPO record's mirror of it
        rk = rec_keys.index
        assert ppo_rec[S("Training/policy_loss")] == rec[rk("Training/policy_loss")]
        assert ppo_rec[S("logprob/mean")] == rec[rk("log_prob" if learner == "a2c" else "logprob/mean")]
        r["ppo/advs/mean"] = ce.ratio(abs(ppo_rec[S("advs/mean")] - R["amean"]), G["rf"]["advs/mean"])
        r["ppo/advs/std"] = ce.ratio(abs(ppo_rec[S("advs/std")] - R["astd"]), G["bessel_std"])     # torch's (Bessel) std here
        assert ppo_rec[S("advs/max")] == R["rf"]["advs/max"] and ppo_rec[S("advs/min")] == R["rf"]["advs/min"]
        if learner == "a2c":
            assert ppo_rec[S("Training/vf_loss")] == rec[rk("Training/vf_loss")]
        else:
            for k in ("advs/mean", "advs/max", "advs/min", "logprob/std", "logprob/max", "logprob/min"):
                assert ppo_rec[S(k)] == rec[rk(k)], k
        for k in ("log_std/mean", "log_std/std", "log_std/max", "log_std/min", "ratio/max", "ratio/min"):
            assert ppo_rec[S(k)] == 0.0, k
        print("\n[%s %s %s n=%d] grad_scale %g, clamped %d; error / gate: %s"
              % (learner, name, mode, n, gs, nsat, " ".join("%s %.3f" % kv for kv in r.items())))
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
        assert max(r.values()) <= 1.0, (n, {k: v for k, v in r.items() if v > 1.0})
    _record("loss/%s/%s/%s" % (learner, name, mode), worst)


# ------------------------------------------------------------------------------------------ rollout step
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("E", ce.ROLLOUT_ES)
def test_rollout_step_on_saturated_rows(E, mode, device):
    """RolloutActor.step (GENERAL route: act_finish_cat_kernel, one 256-thread block looping over E) on edge_hard's pair at
    E = 1, 65, 256, 257, with the uniforms supplied through the actor's bound `_draw`: a step of mixed uniforms (1 - 2^-24, 0 and
    seeded ones across the rows), a step of 1 - 2^-24 on every row, and a deterministic step. Against the step's OWN logits (the
    `out` view of the actor's workspace): the action equals pick64 of their probabilities outside the band and lies between the
    picks of u -+ 1e-6 on every row; p(action) > 0 on EVERY row; the filed log pi and the entropy against head64 through the
    gates; the deterministic action has the largest probability; value and filing as tests/test_gpu_cat.py::test_rollout_step
    checks them (its tolerance for the value of two routes: 1e-5 f32, 4e-3 16-bit, of max(1, |v|))."""
    from vision4leg_amd.torchrl.policies import RolloutActor
    name = "edge_hard"
    case = EDGE_CASES[name]
    K = case["K"]
    pf, vf = _build(case, mode, device)
    pool = ce.batch(name, ce.POOL_N)["obs"]
    T = 3
    worst = {}
    with torch.cuda.device(device):
        net = pf.hip
        net.ensure_bound()
        _own_logits(pf, name, device)   # (the row kinds on this mode's logits)
        slots = (T + 1) * E
        state, image = net.alloc_rollout(slots, device)
        acts = torch.full((slots, 1), SENT, device=device)
        vals, logp = torch.full((slots,), SENT, device=device), torch.full((slots,), SENT, device=device)
        ra = RolloutActor(pf, vf, E)
        actor = ra._actor
        assert actor.route() == "GENERAL" and tuple(actor.eps.shape) == (E, 1) and not actor.graph
        actor.attach((state, image, acts, vals, logp))
        actor.seek(0)
        fill = {}
        actor._draw = lambda buf: buf.copy_(fill["u"].view_as(buf))
        tol = 1e-5 if mode == "f32" else 4e-3
        for s in range(T):
            det = s == T - 1
            ob = _up(pool[(np.arange(E) + s * E) % ce.POOL_N], device)
            sl = slice(s * E, (s + 1) * E)
            un = ce.mixed_uniforms(case, E) if s == 0 else np.full(E, ce.U_MAX, dtype=np.float32)
            fill["u"] = _up(un, device)
            actor.step(ob, deterministic=det)
            torch.cuda.synchronize()
            out = {k: v.clone() for k, v in actor._out.items()}
            used = actor.eps.clone().view(E).cpu().numpy()
            assert (used == (-1.0 if det else un)).all()
            logits = net.ws_view(E, "out", E, 16, actor.ws).clone()
            assert bool((logits[:, K:] == 0).all())
            action = out["action"].view(E).cpu().numpy()
            assert (action == np.round(action)).all() and action.min() >= 0 and action.max() < K
            a = action.astype(np.int64)
            probs = net.cat_head(logits, E)[0].cpu().numpy()
            sep_value = vf(ob).view(E)
            torch.cuda.synchronize()
            h = ce.head64(logits[:, :K].cpu().numpy(), a)
            g = ce.head_gates(h)
            picked = probs[np.arange(E), a]
            assert (picked > 0).all(), (s, int((picked == 0).sum()), h["lp"].min())
            if det:
                assert (picked == probs.max(axis=1)).all()
            else:
                want, dist = ce.pick64(probs, un)
                lo, hi = ce.pick_range(probs, un)
                assert (a[dist > ce.BAND] == want[dist > ce.BAND]).all() and ((lo <= a) & (a <= hi)).all()
            r = {"logp": ce.ratio(np.abs(logp[sl].double().cpu().numpy() - h["lp"]), g["lg"][np.arange(E), a]),
                 "ent": ce.ratio(np.abs(out["ent"].view(E).double().cpu().numpy() - h["H"]), g["H"])}
            print("\n[rollout E=%d %s step %d%s] lowest log pi filed %.2f; error / gate: %s"
                  % (E, mode, s, " (deterministic)" if det else "", h["lp"].min(), " ".join("%s %.3f" % kv for kv in r.items())))
            for k, v in r.items():
                worst[k] = max(worst.get(k, 0.0), v)
            assert max(r.values()) <= 1.0, (s, r)
            assert (out["value"].view(E) - sep_value).abs().max().item() <= tol * max(1.0, sep_value.abs().max().item())
            # filing: this step's slots hold what the step returned, the later ones the sentinel
            assert torch.equal(acts[sl], out["action"]) and torch.equal(vals[sl], out["value"].view(E)) and bool((logp[sl] != SENT).all())
            assert bool((acts[(s + 1) * E:] == SENT).all()) and bool((vals[(s + 1) * E:] == SENT).all()) and bool((logp[(s + 1) * E:] == SENT).all())
    _record("rollout/E%d/%s" % (E, mode), worst)
