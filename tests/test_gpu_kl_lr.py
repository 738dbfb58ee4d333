"""-m gpu: PPO(desired_kl=...), the KL-adaptive learning rates decided on the device. kl_adapt_kernel forms
approx_kl per update, takes the decision and writes both rates into the control block, where the next update's opening launch
reads them — through the captured epoch graph, per-update replays, eager launches and host batches. Cases, their validity
conditions and the semantics restated over the CPU oracle: tests/kl_lr_cases.py (tests/test_kl_lr_cpu.py asserts the conditions)."""
import numpy as np
import pytest
import torch

import util
import kl_cases as kc
import kl_lr_cases as lc
import test_gpu_kl_stop as ks  # its net / agent builders, state readers and edge rollout, unchanged
from vision4leg_amd import _lib

pytestmark = pytest.mark.gpu

MODES = lc.MODES
HOWS = ks.HOWS
ST_LP_MEAN = ks.ST_LP_MEAN
NEW_KEYS = ["approx_kl", "lr_decision", "lr/pf", "lr/vf"]


def _agent(name, mode, dev, armed=True, guard=False, **over):
    c = dict(lc.CASES[name], **over)
    pf, vf = ks._nets(lc.geometry(name), mode, dev)
    lc.init_policy(pf, name)
    kw = dict(desired_kl=c["desired_kl"], kl_lr_factor=c["factor"], kl_lr_min=c["lr_min"], kl_lr_max=c["lr_max"]) if armed else {}
    agent = ks._ppo(pf, vf, dev, lc.B, c["plr"], c["vlr"], skip_nonfinite_steps=guard, **kw)
    sd = lambda net: {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    agent.init = (sd(agent.pf), sd(agent.vf))
    agent.rates0 = (c["plr"], c["vlr"])
    return agent


def _reset(agent):
    """Back to the state the agent was built in: parameters, zeroed moments, zero step counts, the starting rates."""
    ks._reset(agent)
    agent.pf_optimizer.param_groups[0]["lr"], agent.vf_optimizer.param_groups[0]["lr"] = agent.rates0
    agent.lr_changes = {"down": 0, "up": 0}


def _run(agent, how, dat, rows, monkeypatch, warm=True):
    """One run over `rows` from the agent's initial state through `how`. -> (records [U][24] (host path: [U][18]), the [U][4]
    columns (approx_kl, decision, lr_pf, lr_vf) or None, skip flags [U][2] or None)."""
    from vision4leg_amd.engine import HipTrainer
    case, obs, acts, advs, rets = dat[:5]
    dev = agent.device
    armed, guard = agent.desired_kl is not None, agent.skip_nonfinite_steps
    agent.trainer.sync_target()
    if how == "host":
        st, ad, fl = [], [], []
        for r in rows:
            info = agent.update({"obs": obs[r], "acts": acts[r], "advs": advs[r], "estimate_returns": rets[r], "values": rets[r]})
            st.append([info[k] for k in util.STAT_KEYS])
            if guard:
                fl.append([info["skipped/pf"], info["skipped/vf"]])
            if armed:
                ad.append([info[k] for k in NEW_KEYS])
        return np.array(st, np.float32), (np.array(ad, np.float32) if armed else None), (np.array(fl) if guard else None)
    monkeypatch.setenv("V4L_EPOCH_GRAPH", "1" if how == "epoch-graph" else "0")
    agent.use_graph = how != "eager"
    net = agent.pf.hip
    net.ensure_bound()
    state, image = net.alloc_rollout(lc.T * lc.E, dev)
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=dev)
    net.ingest(t(obs), state, image)
    ro = HipTrainer.rollout(state, image, t(acts), t(advs), t(rets), t(rets))
    rows_t = torch.tensor(np.stack(rows), device=dev)

    def once():
        stats = torch.zeros(len(rows), 24, device=dev)
        skip = torch.full((len(rows), 2), -1, dtype=torch.int32, device=dev) if guard else None
        ad = torch.full((len(rows), 4), -7.0, device=dev) if armed else None
        agent.run_updates(ro, rows_t, stats, skip, ad)
        torch.cuda.synchronize()
        return stats.cpu().numpy(), (ad.cpu().numpy() if armed else None), (skip.cpu().numpy() if guard else None)
    agent.once = once
    if how == "epoch-graph" and warm:  # a configuration's first run goes update by update; the next one is the whole-run graph's replay
        once()
        _reset(agent)
        agent.trainer.sync_target()
    return once()


_ORACLE = {}


def _oracle(name, mode, adaptive=True):
    key = (name, mode, adaptive)
    if key not in _ORACLE:  # computed once, shared, never changed
        opf, ovf = lc.cpu_nets(name)
        _ORACLE[key] = lc.oracle_run(name, mode, opf, ovf, lc.data(name), lc.CASES[name]["desired_kl"] if adaptive else None)
    return _ORACLE[key]


# ---- 1. armed but inert equals off
@pytest.mark.parametrize("mode", MODES)
def test_armed_but_inert_equals_off(mode, device, monkeypatch):
    """desired_kl = 1e9 (no estimate reaches 0.5e9: every decision is +1) with kl_lr_min = kl_lr_max = plr = vlr, so that both
    clamps hold the rates where they are, against desired_kl = None through the epoch graph: records, parameters and all four
    moment buffers are bit-identical; the columns report the estimate, +1 and the unchanged rates."""
    monkeypatch.setenv("V4L_COMPUTE", mode)
    name, lr = "mlp_all_three", 2e-4
    dat = lc.data(name)
    over = dict(plr=lr, vlr=lr, desired_kl=1e9, lr_min=lr, lr_max=lr)
    on, off = _agent(name, mode, device, **over), _agent(name, mode, device, armed=False, **over)
    s_on, ad, _ = _run(on, "epoch-graph", dat, dat[5], monkeypatch)
    s_off, none, _ = _run(off, "epoch-graph", dat, dat[5], monkeypatch)
    assert none is None and np.array_equal(s_on, s_off)
    ks._same(ks._state(on), ks._state(off))
    U = len(dat[5])
    assert on.trainer.adam_steps() == off.trainer.adam_steps() == (U, U)
    assert np.isfinite(ad[:, 0]).all() and (ad[:, 1] == 1).all() and (ad[:, 2:] == np.float32(lr)).all()
    assert on.trainer.lrs() == (lr, lr) and on.pf_optimizer.lr == lr and on.vf_optimizer.lr == lr
    assert on.lr_changes == {"down": 0, "up": 0}  # (run_updates itself counts nothing: the epoch's reader does)


def test_armed_update_is_the_off_update_plus_one_launch(device):
    """The profiler's labels of one update with stored log pi_old on loco_s84 (f16): off 22 launches, as before; armed the same
    list plus one kl_adapt launch."""
    import test_gpu_update_route as route
    from vision4leg_amd.engine import HipTrainer

    def labels(kw):
        def run():
            case = dict(util.CASES["loco_s84"], B=6)
            n = case["B"]
            pf, vf = ks._nets(case, "f16", device)
            agent = ks._ppo(pf, vf, device, n, 1e-4, 1e-4, **kw)
            agent.use_graph = False
            net = pf.hip
            net.ensure_bound()
            state, image = net.alloc_rollout(n, device)
            b = util.make_batch(case)
            net.ingest(torch.tensor(b["obs"], dtype=torch.float32, device=device), state, image)
            t32 = lambda a: torch.tensor(np.asarray(a).reshape(-1), dtype=torch.float32, device=device)
            ro = HipTrainer.rollout(state, image, torch.tensor(b["acts"], dtype=torch.float32, device=device), t32(b["advs"]),
                                    t32(b["estimate_returns"]), t32(b["values"]), torch.full((n,), -6.0, device=device))
            rows = torch.arange(n, dtype=torch.int32, device=device).view(1, n)
            agent.trainer.sync_target()
            agent.run_updates(ro, rows, torch.zeros(1, 24, device=device))
            return route._profiled(lambda: agent.run_updates(ro, rows, torch.zeros(1, 24, device=device)))
        return route._with_env("f16", {}, run)
    off, on = labels({}), labels(dict(desired_kl=1e9))
    assert sum(r[1] for r in off) == 22, off
    new = [r for r in on if "kl_adapt" in r[0]]
    assert len(new) == 1 and new[0][1] == 1, new
    assert tuple(r for r in on if "kl_adapt" not in r[0]) == off


# ---- 2. the four paths agree
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", lc.PLAIN)
def test_the_four_paths_agree(name, mode, device, monkeypatch):
    """Epoch graph, per-update replays, eager launches and host batches: records, the four columns, the final state and
    trainer.lrs() are equal bit for bit, and the optimisers carry those rates."""
    monkeypatch.setenv("V4L_COMPUTE", mode)
    dat = lc.data(name)
    res = {}
    for how in HOWS:
        a = _agent(name, mode, device)
        st, ad, _ = _run(a, how, dat, dat[5], monkeypatch)
        res[how] = (st, ad, ks._state(a), a.trainer.lrs())
        assert (a.pf_optimizer.param_groups[0]["lr"], a.vf_optimizer.param_groups[0]["lr"]) == res[how][3], how
    ref = res[HOWS[0]]
    assert set(np.unique(ref[1][:, 1])) <= {-1.0, 0.0, 1.0} and len(set(ref[1][:, 1])) >= 1
    assert np.array_equal(ref[1][-1, 2:], np.array(ref[3], np.float32))  # the last row's rates are the control block's, rounded
    for how in HOWS[1:]:
        assert np.array_equal(res[how][1], ref[1]), (how, res[how][1], ref[1])
        assert np.array_equal(res[how][0][:, :18], ref[0][:, :18]), how  # (the host path returns the 18 logger values)
        ks._same(res[how][2], ref[2])
        assert res[how][3] == ref[3], (how, res[how][3], ref[3])


def test_graph_counts(device, monkeypatch):
    """Epoch-graph path (f16): the first run of a shape goes update by update (one single-update capture), the second captures the
    whole run, a third at unchanged settings captures nothing; a changed desired_kl drops both graphs and they are captured again.
    The early stop's graphs are not used."""
    monkeypatch.setenv("V4L_COMPUTE", "f16")
    name = "mlp_all_three"
    dat = lc.data(name)
    a = _agent(name, "f16", device)
    U = len(dat[5])
    _run(a, "epoch-graph", dat, dat[5], monkeypatch, warm=False)
    assert a.trainer.kl_adapt_graph_counts() == (1, U - 1)
    a.once()
    assert a.trainer.kl_adapt_graph_counts() == (2, U)
    a.once()
    assert a.trainer.kl_adapt_graph_counts() == (2, U + 1)
    a.desired_kl = 2 * a.desired_kl
    a.once()
    assert a.trainer.kl_adapt_graph_counts() == (3, 2 * U)
    a.once()
    assert a.trainer.kl_adapt_graph_counts() == (4, 2 * U + 1)
    assert a.trainer.kl_graph_counts() == (0, 0)


# ---- 3. against the restatement
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", lc.PLAIN)
def test_against_the_restatement(name, mode, device, monkeypatch):
    """Decisions equal the oracle's; |approx_kl - oracle's| <= kl_tol per update; trainer.lrs() and the optimisers' rates EQUAL
    the restatement's doubles; the final parameters within tests/test_gpu_kl_stop.py::test_against_the_oracle's gates (1e-7 mean
    abs in f32, 2e-5 U in the 16-bit modes) times max(1, largest policy rate of the oracle run / the starting one) — an Adam step
    moves an element by at most its rate — and in f32 ten times closer to this oracle than to the fixed-rate one."""
    monkeypatch.setenv("V4L_COMPUTE", mode)
    c = lc.CASES[name]
    dat = lc.data(name)
    a = _agent(name, mode, device)
    st, ad, _ = _run(a, "epoch-graph", dat, dat[5], monkeypatch)
    ref = _oracle(name, mode)
    print("   %s %s decisions %s oracle %s" % (name, mode, ad[:, 1].tolist(), ref["d"].tolist()))
    for u in range(c["U"]):
        tol = kc.kl_tol(mode, ref["infos"][u]["logprob/mean"])
        d = abs(float(ad[u, 0]) - ref["kl"][u])
        print("   update %d: approx_kl %.6f oracle %.6f |d| %.2e (bound %.2e) rates %s" % (u, ad[u, 0], ref["kl"][u], d, tol, ad[u, 2:]))
        util.record("kl_lr/%s/%s/approx_kl_err_u%d" % (name, mode, u), d)
    assert ad[:, 1].tolist() == ref["d"].tolist()
    for u in range(c["U"]):
        assert abs(float(ad[u, 0]) - ref["kl"][u]) <= kc.kl_tol(mode, ref["infos"][u]["logprob/mean"]), u
    assert np.array_equal(ad[:, 2:], ref["lrs"][1:].astype(np.float32))
    want = tuple(ref["lrs"][-1].tolist())
    assert a.trainer.lrs() == want, (a.trainer.lrs(), want)
    assert (a.pf_optimizer.param_groups[0]["lr"], a.vf_optimizer.param_groups[0]["lr"]) == want
    scale = max(1.0, ref["lrs"][:-1, 0].max() / c["plr"])
    d = ks._mean_abs(a, ref["pf"], ref["vf"])
    util.record("kl_lr/%s/%s/mean_abs_param_err" % (name, mode), d)
    print("   mean |param - adaptive oracle| = %.3e (%s; gate scale %.2f)" % (d, mode, scale))
    if mode == "f32":
        fixed = _oracle(name, mode, adaptive=False)
        d_fixed = ks._mean_abs(a, fixed["pf"], fixed["vf"])
        print("   mean |param - fixed-rate oracle| = %.3e" % d_fixed)
        assert d <= 1e-7 * scale, d
        assert d * 10 <= d_fixed, (d, d_fixed)
    else:
        assert d <= 2e-5 * c["U"] * scale, d


# ---- 4. the kernel at its edges
EDGE_N = ks.EDGE_N
SLOTS = ks.SLOTS
LR0 = (1e-4, 3e-5)


def _one(agent, ro, rowidx, n, desired, lr=LR0, factor=1.5, lr_min=1e-5, lr_max=1e-2, guard=False, sync=True):
    """One eager armed update -> (record [24], columns [4], trainer.lrs(), skip flags [2] or None) as the device wrote them."""
    tr, dev = agent.trainer, agent.device
    stats = torch.zeros(1, 24, device=dev)
    ad = torch.full((1, 4), -7.0, device=dev)
    skip = torch.full((1, 2), -1, dtype=torch.int32, device=dev) if guard else None
    if sync:
        tr.sync_target()
    cur = torch.cuda.current_stream(dev)
    tr.stream.wait_stream(cur)
    with torch.cuda.stream(tr.stream):
        tr._pre(n)
        tr.begin(rowidx, stats, lr[0], lr[1], skip)
        tr.kl_adapt_arm(ad, desired, factor, lr_min, lr_max)
        tr.kl_adapt_update_next(ro, n, graph=False)
        lrs = tr.lrs()
    cur.wait_stream(tr.stream)
    torch.cuda.synchronize()
    return stats[0].cpu().numpy(), ad[0].cpu().numpy(), lrs, (skip[0].cpu().numpy() if guard else None)


def _check_rule(ad, lrs, want, tol, desired, lr=LR0, factor=1.5, lr_min=1e-5, lr_max=1e-2):
    """The decision the float64 value takes (it keeps `tol` from both thresholds: the inputs' business) and both next rates."""
    assert abs(float(ad[0]) - want) <= tol, (ad[0], want, tol)
    assert min(abs(want - 0.5 * desired), abs(want - 2.0 * desired)) > tol, (want, desired, tol)
    d = lc.decide(want, desired)
    nxt = tuple(lc.next_rate(r, d, factor, lr_min, lr_max) for r in lr)
    assert ad[1] == d, (ad, want, desired)
    assert lrs == nxt and np.array_equal(ad[2:], np.array(nxt, np.float32)), (lrs, nxt, ad)
    return d


def _three(agent, ro, rowidx, n, want_of, tol_of, seen, sync=True):
    """Three updates on the same rows. want_of(rec) -> the float64 approx_kl of an update from its record. The first runs with
    desired_kl = 1e9 (+1). Its float64 value w and tolerance t set the other two, so that the thresholds keep their distance from
    a value that one Adam step at 1e-4 barely moves: w > 4 t: desired_kl = w (inside the band, 0) and w / 8 (-1); otherwise (the
    noise floor, or a negative estimate) 4 (|w| + 2 t) both times: +1 at a threshold of the estimate's own size."""
    rec, ad, lrs, _ = _one(agent, ro, rowidx, n, 1e9, sync=sync)
    w = want_of(rec)
    t = tol_of(w, rec)
    seen.add(_check_rule(ad, lrs, w, t, 1e9))
    for desired in ((w, w / 8.0) if w > 4 * t else (4 * (abs(w) + 2 * t),) * 2):
        rec, ad, lrs, _ = _one(agent, ro, rowidx, n, desired, sync=sync)
        want = want_of(rec)
        seen.add(_check_rule(ad, lrs, want, tol_of(want, rec), desired))


@pytest.mark.parametrize("mode", MODES)
def test_stored_branch_at_block_edges(mode, device, monkeypatch):
    """n in {2, 255, 256, 257, 1025}, rowidx null and permuted, stored log pi_old: approx_kl against float64
    mean(logp_old[rows]) - float64(record's logprob/mean) within (1e-5 f32, 4e-3 16-bit) x max(1, |want|); the decision and both
    next rates follow from that value, at three settings of desired_kl."""
    monkeypatch.setenv("V4L_COMPUTE", mode)
    case = dict(util.CASES["mlp_s93"], B=max(EDGE_N))
    pf, vf = ks._nets(case, mode, device)
    agent = ks._ppo(pf, vf, device, max(EDGE_N), 1e-4, 1e-4, desired_kl=1e9)
    _, _, logp, ro = ks._edge_rollout(agent, case, 5)
    lp64 = logp.double().cpu().numpy()
    rs = np.random.RandomState(6)
    rel = 1e-5 if mode == "f32" else 4e-3
    seen = set()
    for n in EDGE_N:
        for permuted in (False, True):
            rows = rs.permutation(SLOTS)[:n].astype(np.int32) if permuted else np.arange(n, dtype=np.int32)
            rowidx = torch.tensor(rows, device=device).view(1, n) if permuted else None
            old = lp64[rows].mean()
            _three(agent, ro(True), rowidx, n, lambda rec: old - float(rec[ST_LP_MEAN]), lambda want, rec: rel * max(1.0, abs(want)), seen)
    print("   decisions seen: %s" % sorted(seen))
    assert 1 in seen and seen <= {-1, 0, 1}, seen


# (GaussianContPolicy takes at most 8 action dimensions — mean and log-std share the 16-column head row: its A = 12 is 8 here,
# the largest it builds)
RECOMPUTED = [(head, A, tanh) for head, As in (("normal", (1, 6, 12)), ("sd", (1, 6, 8))) for A in As for tanh in (False, True)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("head,A,tanh", RECOMPUTED, ids=["%s-a%d%s" % (h, A, "-tanh" if t else "") for h, A, t in RECOMPUTED])
def test_recomputed_branch_at_block_edges(head, A, tanh, mode, device, monkeypatch):
    """No stored log pi_old: the kernel forms the frozen target's log-probability from the target's head rows (both head kinds,
    A in {1, 6, 12}, TanhNormal on and off), n in {2, 255, 256, 257, 1025} permuted rows. approx_kl against
    float64(target_pf.update(obs, acts)["log_prob"]).mean() - float64(record's logprob/mean) within (1e-5 f32, 4e-3 16-bit) x
    max(1, |mean log pi_old|, |want|); the decision and both next rates follow from that value."""
    monkeypatch.setenv("V4L_COMPUTE", mode)
    kind = "mlp_tanh" if tanh else "mlp"
    case = dict(kind=kind, S=93, A=A, seed=80 + A, B=max(EDGE_N), enc=[256, 256], head=[256, 256])
    pf, vf = ks._nets(case, mode, device, ks._sd_build if head == "sd" else None)
    if head == "sd":
        import test_gpu_sd as tsd
        w, b = tsd._last(pf)
        with torch.no_grad():
            b[:A].copy_(torch.linspace(-1.0, 1.0, A) if tanh else torch.linspace(-1.5, 1.5, A))
            b[A:].copy_(torch.tensor(util.loss_rows_logstd(A, tanh)))
    else:
        util.spread_policy_head(pf, logstd=util.loss_rows_logstd(A, tanh))
    agent = ks._ppo(pf, vf, device, max(EDGE_N), 1e-4, 1e-4, desired_kl=1e9)
    obs, acts, _, ro = ks._edge_rollout(agent, case, 7, tanh)
    # the target is frozen here; the live policy's means then move by 0.1, so that the estimate is not at its noise floor
    agent.trainer.sync_target()
    torch.cuda.synchronize()
    import test_gpu_sd as tsd
    with torch.no_grad():
        tsd._last(pf)[1][:A].add_(0.1)
    pf.mark_params_changed()
    rs = np.random.RandomState(8)
    rel = 1e-5 if mode == "f32" else 4e-3
    seen = set()
    for n in EDGE_N:
        rows = rs.permutation(SLOTS)[:n].astype(np.int32)
        idx = torch.tensor(rows.astype(np.int64), device=device)
        with torch.no_grad():
            old = agent.target_pf.update(obs[idx], acts[idx])["log_prob"].double().mean().item()
        assert np.isfinite(old)
        _three(agent, ro(False), torch.tensor(rows, device=device).view(1, n), n, lambda rec: old - float(rec[ST_LP_MEAN]),
               lambda want, rec: rel * max(1.0, abs(old), abs(want)), seen, sync=False)
    print("   %s A=%d tanh=%s %s: decisions seen %s" % (head, A, tanh, mode, sorted(seen)))
    assert 1 in seen and seen <= {-1, 0, 1}, seen


# ---- 5. rule edges
@pytest.mark.parametrize("mode", MODES)
def test_nan_advantage_with_the_guard(mode, device, monkeypatch):
    """A NaN advantage in the first minibatch, guard on: that policy step is skipped and flagged ([1, 0]); the estimate does not
    depend on the advantages, stays finite and takes the decision the rule gives — decisions, rates and step counts are those
    of the restatement with both semantics."""
    monkeypatch.setenv("V4L_COMPUTE", mode)
    name = "mlp_nan_guard"  # (its data carry the NaN, its oracle run the guard)
    dat = lc.data(name)
    a = _agent(name, mode, device, guard=True)
    st, ad, skip = _run(a, "epoch-graph", dat, dat[5], monkeypatch)
    ref = _oracle(name, mode)
    assert not lc.validity(name, mode, ref), lc.validity(name, mode, ref)
    assert skip[0].tolist() == [1, 0] and (skip[1:] == 0).all(), skip
    assert np.isfinite(ad[:, 0]).all() and ad[:, 1].tolist() == ref["d"].tolist()
    assert a.trainer.lrs() == tuple(ref["lrs"][-1].tolist())
    U = len(dat[5])
    assert a.trainer.adam_steps() == (U - 1, U) == (ref["steps"]["pf"], ref["steps"]["vf"])
    assert all(torch.isfinite(v).all() for v in ks._state(a).values())


def _edge_agent(mode, device):
    case = dict(util.CASES["mlp_s93"], B=256)
    pf, vf = ks._nets(case, mode, device)
    agent = ks._ppo(pf, vf, device, 256, 1e-4, 1e-4, desired_kl=1.0, skip_nonfinite_steps=True)
    _, _, logp, ro = ks._edge_rollout(agent, case, 5)
    return agent, logp, ro(True)


@pytest.mark.parametrize("mode", MODES)
def test_nan_estimate_holds_the_rates(mode, device, monkeypatch):
    """One stored log pi_old of the minibatch is NaN: approx_kl is NaN, compares false twice, d = 0 and both rates stay; the
    policy's gradient is not finite and the guard skips and flags that step."""
    monkeypatch.setenv("V4L_COMPUTE", mode)
    agent, logp, ro = _edge_agent(mode, device)
    logp[3] = float("nan")
    before = ks._state(agent)
    rec, ad, lrs, skip = _one(agent, ro, None, 256, 1.0, guard=True)
    assert np.isnan(ad[0]) and ad[1] == 0 and lrs == LR0 and np.array_equal(ad[2:], np.array(LR0, np.float32))
    assert skip.tolist() == [1, 0] and agent.trainer.adam_steps() == (0, 1)
    after = ks._state(agent)
    assert all(torch.equal(after[k], before[k]) for k in after if k.startswith("pf/") and "base" not in k)


@pytest.mark.parametrize("mode", MODES)
def test_clamps(mode, device, monkeypatch):
    """Stored log pi_old set 3 above / below the policy's own mean log-probability makes approx_kl ~ +3 / -3 against desired_kl =
    1: d = -1 / +1. A rate on kl_lr_min stays there on -1 and one on kl_lr_max on +1, while the other optimiser's rate moves:
    the two clamp independently."""
    monkeypatch.setenv("V4L_COMPUTE", mode)
    agent, logp, ro = _edge_agent(mode, device)
    logp.fill_(0.0)
    rec, ad, _, _ = _one(agent, ro, None, 256, 1e9, guard=True)
    lp = float(rec[ST_LP_MEAN])
    assert np.isfinite(lp) and abs(float(ad[0]) + lp) <= 4e-3 * max(1.0, abs(lp))
    for shift, d, lr, lo, hi, want in (
            (3.0, -1, (1e-5, 3e-5), 1e-5, 1e-2, (1e-5, 3e-5 / 1.5)),      # pf on kl_lr_min stays; vf falls
            (3.0, -1, (3e-5, 1e-5), 1e-5, 1e-2, (3e-5 / 1.5, 1e-5)),      # the other way round
            (3.0, -1, (1.2e-5, 1.2e-5), 1e-5, 1e-2, (1e-5, 1e-5)),        # both reach it
            (-3.0, 1, (2e-4, 3e-5), 1e-5, 2e-4, (2e-4, 3e-5 * 1.5)),      # pf on kl_lr_max stays; vf grows
            (-3.0, 1, (3e-5, 2e-4), 1e-5, 2e-4, (3e-5 * 1.5, 2e-4)),
            (-3.0, 1, (1.9e-4, 1.9e-4), 1e-5, 2e-4, (2e-4, 2e-4))):
        logp.fill_(lp + shift)
        rec, ad, lrs, skip = _one(agent, ro, None, 256, 1.0, lr=lr, lr_min=lo, lr_max=hi, guard=True)
        assert abs(float(ad[0]) - shift) < 0.5 and ad[1] == d, (shift, ad)
        assert lrs == want and np.array_equal(ad[2:], np.array(want, np.float32)), (lr, lrs, want)
        assert skip.tolist() == [0, 0]
        lp = float(rec[ST_LP_MEAN])


# ---- 6. persistence across epochs, 7. resume
def _epochs_agent(case, seed, dev, **kw):
    import test_gpu_resume as rsm
    return rsm._agent(case, seed, dev, desired_kl=0.01, **kw)


def test_rates_persist_across_epochs(device, monkeypatch):
    """Two epochs through update_per_epoch on the resident buffer (f16): the second begin() receives the first epoch's final rates
    as the device left them, not the linear schedule's; the logger's infos carry the four keys; lr_changes matches the records."""
    import test_gpu_resume as rsm
    monkeypatch.setenv("V4L_COMPUTE", "f16")
    case = util.CASES["mlp_s93"]
    a = _epochs_agent(case, case["seed"], device)
    np.random.seed(5)
    down = up = 0
    after = []
    for epoch in range(2):
        rsm._epoch(a, case, epoch)
        after.append(a.trainer.lrs())
        rec = a._kl_buf.cpu().numpy()
        assert rec.shape == (rsm.U, 4)
        down += int((rec[:, 1] == -1).sum()); up += int((rec[:, 1] == 1).sum())
        assert np.array_equal(rec[-1, 2:], np.array(after[-1], np.float32))
        assert (a.pf_optimizer.param_groups[0]["lr"], a.vf_optimizer.param_groups[0]["lr"]) == after[-1]
    print("   rates handed to begin(): %s; after the epochs: %s; lr_changes %s" % (a.lrs, after, a.lr_changes))
    assert a.lrs[0] == (rsm.LR, 2 * rsm.LR)  # epoch 0 opens with plr / vlr
    assert a.lrs[1] == after[0] and after[0] != a.lrs[0]
    sched = (rsm.LR - rsm.LR * (1 / float(rsm.NUM_EPOCHS)), 2 * rsm.LR - 2 * rsm.LR * (1 / float(rsm.NUM_EPOCHS)))
    assert a.lrs[1] != sched
    assert a.lr_changes == {"down": down, "up": up} and down + up > 0
    infos = a.logger.updates
    assert len(infos) == 2 * rsm.U and all(sorted(i) == sorted(util.STAT_KEYS + NEW_KEYS) for i in infos)
    assert [i["lr_decision"] for i in infos[rsm.U:]] == rec[:, 1].tolist()
    assert [np.float32(i["lr/pf"]) for i in infos[rsm.U:]] == rec[:, 2].tolist()


@pytest.mark.parametrize("mode", MODES)
def test_resume_continues_the_rates(mode, device, tmp_path, monkeypatch):
    """save_train_state=True: one epoch, save_checkpoint, then a new PPO(resume=...) over nets from another seed and one more
    epoch: rates, parameters and moments are bit-equal to the uninterrupted two-epoch run."""
    import test_gpu_resume as rsm
    monkeypatch.setenv("V4L_COMPUTE", mode)
    case = util.CASES["mlp_s93"]
    ckpt = str(tmp_path)
    a = _epochs_agent(case, case["seed"], device, save_train_state=True)
    np.random.seed(5)
    for epoch in range(2):
        rsm._epoch(a, case, epoch)
    b1 = _epochs_agent(case, case["seed"], device, save_train_state=True)
    np.random.seed(5)
    rsm._epoch(b1, case, 0)
    b1.save_checkpoint(ckpt, 0)
    saved = b1.trainer.lrs()
    del b1
    np.random.seed(999)
    b2 = _epochs_agent(case, case["seed"] + 100, device, save_train_state=True, resume=(ckpt, 0))
    assert b2.start_epoch == 1
    assert (b2.pf_optimizer.param_groups[0]["lr"], b2.vf_optimizer.param_groups[0]["lr"]) == saved == a.lrs[1]
    rsm._epoch(b2, case, 1)
    assert b2.lrs == [a.lrs[1]] and b2.lrs[0] != (rsm.LR, 2 * rsm.LR)
    assert b2.trainer.lrs() == a.trainer.lrs()
    rsm._assert_same(rsm._state(a), rsm._state(b2))
    assert torch.equal(a.records[1], b2.records[0]) and torch.equal(a._kl_buf.cpu(), b2._kl_buf.cpu())
    assert a.logger.updates[rsm.U:] == b2.logger.updates
