"""-m gpu: PPO(target_kl=...), the KL early stop decided on the device. kl_stop_kernel writes approx_kl and the
latch per update; a set latch makes every later clip_adam_kernel launch of the run skip as a guarded non-finite step does —
through the captured epoch graph, per-update replays, eager launches and host batches. Cases, their validity conditions and the
semantics restated over the CPU oracle: tests/kl_cases.py (tests/test_kl_stop_cpu.py asserts the conditions)."""
import os

import numpy as np
import pytest
import torch

import util
import kl_cases as kc
from vision4leg_amd import _lib

pytestmark = pytest.mark.gpu

MODES = kc.MODES
HOWS = ["epoch-graph", "per-update", "eager", "host"]
ST_LP_MEAN = _lib.STAT_KEYS.index("logprob/mean")


def _nets(case, mode, dev, build=None):
    os.environ["V4L_COMPUTE"] = mode
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    torch.manual_seed(case["seed"])
    pf, vf = (build or util.build_nets)(networks, policies, case)
    return pf.to(dev), vf.to(dev)


def _ppo(pf, vf, dev, batch, plr, vlr, **kw):
    from vision4leg_amd.torchrl.algo import PPO

    class Coll: epoch_frames = kc.T * kc.E
    return PPO(pf=pf, vf=vf, plr=plr, vlr=vlr, clip_para=0.2, opt_epochs=3, tau=0.95, entropy_coeff=0.005, collector=Coll(),
               device=dev, batch_size=batch, **kw)


def _agent(name, mode, dev, target_kl, guard=False):
    c = kc.CASES[name]
    pf, vf = _nets(kc.geometry(name), mode, dev)
    kc.init_policy(pf, name)
    agent = _ppo(pf, vf, dev, kc.B, c["plr"], c["vlr"], target_kl=target_kl, skip_nonfinite_steps=guard)
    sd = lambda net: {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    agent.init = (sd(agent.pf), sd(agent.vf))
    return agent


def _reset(agent):
    """Back to the state the agent was built in: parameters, zeroed moments, zero step counts (a warm-up run leaves no trace)."""
    tr = agent.trainer
    agent.pf.load_state_dict(agent.init[0])
    agent.vf.load_state_dict(agent.init[1])
    for net in agent.networks:
        net.mark_params_changed()
    z = torch.zeros_like
    tr.load_adam_state(z(tr.m_pf), z(tr.v_pf), z(tr.m_vf), z(tr.v_vf), steps=(0, 0), updates=0)


def _state(agent):
    tr = agent.trainer
    out = {"pf/" + k: v.detach().cpu().clone() for k, v in agent.pf.state_dict().items()}
    out.update({"vf/" + k: v.detach().cpu().clone() for k, v in agent.vf.state_dict().items()})
    out.update({k: getattr(tr, k).detach().cpu().clone() for k in ("m_pf", "v_pf", "m_vf", "v_vf")})
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _run(agent, how, dat, rows, monkeypatch):
    """One run over `rows` from the agent's initial state through `how`. -> (records [U'][24], kl [U'][2] or None, skip flags
    [U'][2] or None); U' = len(rows), on the host path the updates up to the one that reported the stop (the loops end there)."""
    from vision4leg_amd.engine import HipTrainer
    case, obs, acts, advs, rets = dat[:5]
    dev = agent.device
    armed, guard = agent.target_kl is not None, agent.skip_nonfinite_steps
    agent.trainer.sync_target()
    if how == "host":
        st, kl, fl = [], [], []
        for r in rows:
            info = agent.update({"obs": obs[r], "acts": acts[r], "advs": advs[r], "estimate_returns": rets[r], "values": rets[r]})
            st.append([info[k] for k in util.STAT_KEYS])
            if guard:
                fl.append([info["skipped/pf"], info["skipped/vf"]])
            if armed:
                kl.append([info["approx_kl"], info["kl_stop"]])
                if info["kl_stop"]:
                    break
        return np.array(st, np.float32), (np.array(kl, np.float32) if armed else None), (np.array(fl) if guard else None)
    monkeypatch.setenv("V4L_EPOCH_GRAPH", "1" if how == "epoch-graph" else "0")
    agent.use_graph = how != "eager"
    net = agent.pf.hip
    net.ensure_bound()
    state, image = net.alloc_rollout(kc.T * kc.E, dev)
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=dev)
    net.ingest(t(obs), state, image)
    ro = HipTrainer.rollout(state, image, t(acts), t(advs), t(rets), t(rets))
    rows_t = torch.tensor(np.stack(rows), device=dev)

    def once():
        stats = torch.zeros(len(rows), 24, device=dev)
        skip = torch.full((len(rows), 2), -1, dtype=torch.int32, device=dev) if guard else None
        kl = torch.full((len(rows), 2), -1.0, device=dev) if armed else None
        agent.run_updates(ro, rows_t, stats, skip, kl)
        torch.cuda.synchronize()
        return stats.cpu().numpy(), (kl.cpu().numpy() if armed else None), (skip.cpu().numpy() if guard else None)
    if how == "epoch-graph":  # a configuration's first run goes update by update; the next one is the whole-run graph's replay
        once()
        _reset(agent)
        agent.trainer.sync_target()
    return once()


_ORACLE = {}


def _oracle(name, mode, target, rows=None, nan_update=None, guard=False):
    key = (name, mode, target, None if rows is None else len(rows), nan_update, guard)
    if key not in _ORACLE:  # computed once, shared, never changed
        opf, ovf = kc.cpu_nets(name)
        dat = kc.data(name, nan_update)
        _ORACLE[key] = kc.oracle_run(name, mode, opf, ovf, dat, target, rows=None if rows is None else dat[5][:rows], guard=guard)
    return _ORACLE[key]


def _u_star(kl):
    assert set(np.unique(kl[:, 1])) <= {0.0, 1.0}, kl[:, 1]
    on = np.nonzero(kl[:, 1])[0]
    assert len(on), kl
    assert (kl[on[0]:, 1] == 1).all(), kl[:, 1]  # once set, the latch stays set
    return int(on[0])


# ---- 1. on without a trip equals off
@pytest.mark.parametrize("mode", MODES)
def test_armed_without_a_trip_equals_off(mode, device, monkeypatch):
    """target_kl = 1e9 against None through the epoch graph: records, parameters, all four moment buffers and adam_steps() are
    bit-identical; the approx_kl column is filled, the latch column is 0."""
    monkeypatch.setenv("V4L_COMPUTE", mode)
    name = "loco_s84"
    dat = kc.data(name)
    on, off = _agent(name, mode, device, 1e9), _agent(name, mode, device, None)
    s_on, kl, _ = _run(on, "epoch-graph", dat, dat[5], monkeypatch)
    s_off, none, _ = _run(off, "epoch-graph", dat, dat[5], monkeypatch)
    assert none is None and np.array_equal(s_on, s_off)
    _same(_state(on), _state(off))
    U = len(dat[5])
    assert on.trainer.adam_steps() == off.trainer.adam_steps() == (U, U) and on.trainer.step == off.trainer.step == U
    assert (kl[:, 1] == 0).all() and np.isfinite(kl[:, 0]).all() and on.last_kl_stop is None and on.kl_stops == 0


def test_armed_update_is_the_off_update_plus_one_launch(device):
    """The profiler's labels of one update with stored log pi_old on loco_s84 (f16): off 22 launches, as before; armed the same
    list plus one kl_stop launch."""
    import test_gpu_update_route as route
    from vision4leg_amd.engine import HipTrainer

    def labels(target):
        def run():
            case = dict(util.CASES["loco_s84"], B=6)
            n = case["B"]
            pf, vf = _nets(case, "f16", device)
            agent = _ppo(pf, vf, device, n, 1e-4, 1e-4, target_kl=target)
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
    off, on = labels(None), labels(1e9)
    assert sum(r[1] for r in off) == 22, off
    new = [r for r in on if "kl_stop" in r[0]]
    assert len(new) == 1 and new[0][1] == 1, new
    assert tuple(r for r in on if "kl_stop" not in r[0]) == off


# ---- 2. a stopped run leaves no trace after the stop
_PATHS = {}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("name", sorted(kc.CASES))
def test_stopped_run_leaves_no_trace(name, how, mode, device, monkeypatch):
    """A runs all U updates and stops at the u* its own flags report (== the oracle's); A' runs rows [:u* + 1] only: the same
    parameters, moments and step counts, bit for bit. adam_steps() == (u*, u* + 1). Against agents with the option off: what the
    critic does not share with the policy (policy head, logstd) and its moments equal those after rows [:u*], what the policy
    does not share with the critic those after rows [:u* + 1] — the one deviation: the critic's step of update u* is taken."""
    monkeypatch.setenv("V4L_COMPUTE", mode)
    c = kc.CASES[name]
    dat = kc.data(name)
    rows, U = dat[5], c["U"]
    a = _agent(name, mode, device, c["target_kl"])
    st, kl, _ = _run(a, how, dat, rows, monkeypatch)
    us = _u_star(kl)
    assert us == _oracle(name, mode, c["target_kl"])["u_star"]
    assert (kl[:us, 0] <= kc.FACTOR * c["target_kl"]).all() and kl[us, 0] > kc.FACTOR * c["target_kl"]
    assert a.trainer.adam_steps() == (us, us + 1)
    if how == "host":  # the loops ended with the update that reported the stop
        assert len(kl) == us + 1 and a.trainer.step == us + 1
    else:
        assert len(kl) == U and a.trainer.step == U
    sa = _state(a)
    assert all(torch.isfinite(v).all() for v in sa.values())
    a2 = _agent(name, mode, device, c["target_kl"])
    st2, kl2, _ = _run(a2, how, dat, rows[:us + 1], monkeypatch)
    assert np.array_equal(kl2, kl[:us + 1]) and np.array_equal(st2, st[:us + 1])
    _same(sa, _state(a2))
    assert a2.trainer.adam_steps() == (us, us + 1)
    # against the option off
    shared = "base." if kc.geometry(name)["kind"].startswith("mlp") else "encoder."
    offs = {}
    for k in (us, us + 1):
        b = _agent(name, mode, device, None)
        _run(b, how, dat, rows[:k], monkeypatch)
        offs[k] = (_state(b), b)
    hip = {"pf": a.pf.hip, "vf": a.vf.hip}
    for tag, k in (("pf", us), ("vf", us + 1)):
        so = offs[k][0]
        own = [p for p in hip[tag].param_names if not p.startswith(shared)]
        assert own, tag
        for p in own:
            assert torch.equal(sa["%s/%s" % (tag, p)], so["%s/%s" % (tag, p)]), (tag, p)
            i = hip[tag].param_names.index(p)
            o, cnt = hip[tag].grad_offsets[i], sa["%s/%s" % (tag, p)].numel()
            for mom in ("m_", "v_"):
                assert torch.equal(sa[mom + tag][o:o + cnt], so[mom + tag][o:o + cnt]), (tag, p, mom)
    # (the control: the stop changed something — the policy's own tensors differ from the run that went on)
    assert not torch.equal(sa["pf/logstd"], offs[us + 1][0]["pf/logstd"])
    _PATHS[name, mode, how] = (st[:us + 1], kl[:us + 1], sa)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(kc.CASES))
def test_the_four_paths_agree(name, mode, device, monkeypatch):
    """Epoch graph, per-update replays, eager launches and host batches: records, approx_kl and flag columns up to u* and the final
    state are equal bit for bit (the results test_stopped_run_leaves_no_trace left; recomputed when it did not run)."""
    monkeypatch.setenv("V4L_COMPUTE", mode)
    c = kc.CASES[name]
    dat = kc.data(name)
    res = {}
    for how in HOWS:
        if (name, mode, how) not in _PATHS:
            a = _agent(name, mode, device, c["target_kl"])
            st, kl, _ = _run(a, how, dat, dat[5], monkeypatch)
            us = _u_star(kl)
            _PATHS[name, mode, how] = (st[:us + 1], kl[:us + 1], _state(a))
        res[how] = _PATHS[name, mode, how]
    ref = res[HOWS[0]]
    for how in HOWS[1:]:
        assert np.array_equal(res[how][1], ref[1]), (how, res[how][1], ref[1])
        assert np.array_equal(res[how][0][:, :18], ref[0][:, :18]), how  # (the host path returns the 18 logger values)
        _same(res[how][2], ref[2])


# ---- 3. against the oracle
def _mean_abs(agent, opf, ovf):
    tot = cnt = 0.0
    for net, onet in ((agent.pf, opf), (agent.vf, ovf)):
        for k, v in net.state_dict().items():
            d = (v.detach().cpu() - onet[k]).abs()
            tot += d.sum().item(); cnt += d.numel()
    return tot / cnt


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(kc.CASES))
def test_against_the_oracle(name, mode, device, monkeypatch):
    """Per update |approx_kl - oracle's| <= 2 x test_ppo_update's info tolerance x max(1, |logprob/mean|); the final parameters
    within tests/test_gpu_skip_nonfinite.py::test_actor_only_skip_matches_the_oracle's gates of the oracle with the same
    semantics (1e-7 mean abs in f32, 2e-5 U in the 16-bit modes), and in f32 ten times closer to it than to the oracle that never
    stops."""
    monkeypatch.setenv("V4L_COMPUTE", mode)
    c = kc.CASES[name]
    dat = kc.data(name)
    a = _agent(name, mode, device, c["target_kl"])
    st, kl, _ = _run(a, "epoch-graph", dat, dat[5], monkeypatch)
    ref = _oracle(name, mode, c["target_kl"])
    assert kl[:, 1].tolist() == ref["latch"].tolist()
    for u in range(c["U"]):
        tol = kc.kl_tol(mode, ref["infos"][u]["logprob/mean"])
        d = abs(float(kl[u, 0]) - ref["kl"][u])
        print("   %s %s update %d: approx_kl %.6f oracle %.6f |d| %.2e (bound %.2e)" % (name, mode, u, kl[u, 0], ref["kl"][u], d, tol))
        util.record("kl_stop/%s/%s/approx_kl_err_u%d" % (name, mode, u), d)
        assert d <= tol, (u, kl[u, 0], ref["kl"][u], tol)
    d = _mean_abs(a, ref["pf"], ref["vf"])
    util.record("kl_stop/%s/%s/mean_abs_param_err" % (name, mode), d)
    print("   mean |param - stopping oracle| = %.3e (%s)" % (d, mode))
    if mode == "f32":
        never = _oracle(name, mode, None)
        d_never = _mean_abs(a, never["pf"], never["vf"])
        print("   mean |param - never-stopping oracle| = %.3e" % d_never)
        assert d <= 1e-7, d
        assert d * 10 <= d_never, (d, d_never)
    else:
        assert d <= 2e-5 * c["U"], d


# ---- 4. the kernel's arithmetic at its edges
EDGE_N = [2, 255, 256, 257, 1025]
SLOTS = 1100


def _one_armed_update(agent, ro, rowidx, n):
    """One eager update of an armed run that cannot trip -> (record [24], kl [2]) as the device wrote them."""
    tr, dev = agent.trainer, agent.device
    stats = torch.zeros(1, 24, device=dev)
    kl = torch.full((1, 2), -1.0, device=dev)
    tr.sync_target()
    cur = torch.cuda.current_stream(dev)
    tr.stream.wait_stream(cur)
    with torch.cuda.stream(tr.stream):
        tr._pre(n)
        tr.begin(rowidx, stats, 1e-4, 1e-4, None)
        tr.kl_arm(kl, 1e9)
        tr.kl_update_next(ro, n, graph=False)
    cur.wait_stream(tr.stream)
    torch.cuda.synchronize()
    return stats[0].cpu().numpy(), kl[0].cpu().numpy()


def _edge_rollout(agent, case, seed, tanh=False):
    from vision4leg_amd.engine import HipTrainer
    dev = agent.device
    rs = np.random.RandomState(seed)
    net = agent.pf.hip
    net.ensure_bound()
    state, image = net.alloc_rollout(SLOTS, dev)
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=dev)
    obs = t(util.obs_rows(rs, SLOTS, case))
    net.ingest(obs, state, image)
    acts = rs.randn(SLOTS, case["A"])
    acts = t(np.tanh(0.5 * acts) if tanh else 0.5 * acts)
    advs, rets = t(rs.randn(SLOTS)), t(rs.randn(SLOTS))
    # stored log pi_old: any numbers of a log-prob's size; spread over four decades so that the double-precision sum matters
    logp = t(-6.0 + rs.randn(SLOTS) * np.where(rs.rand(SLOTS) < 0.1, 30.0, 0.3))
    return obs, acts, logp, lambda stored: HipTrainer.rollout(state, image, acts, advs, rets, rets, logp if stored else None)


@pytest.mark.parametrize("mode", MODES)
def test_stored_branch_at_block_edges(mode, device, monkeypatch):
    """n in {2, 255, 256, 257, 1025} (one thread's rows, a partial last wave, the 256-thread block full and one row over, the
    1024-thread block one row over), rowidx null and permuted, stored log pi_old: approx_kl == float64 mean(logp_old[rows]) -
    float64(record's logprob/mean) within 2^-22 x max(1, |both means|) — one fp32 rounding of the result plus the record's."""
    monkeypatch.setenv("V4L_COMPUTE", mode)
    case = dict(util.CASES["mlp_s93"], B=max(EDGE_N))
    pf, vf = _nets(case, mode, device)
    agent = _ppo(pf, vf, device, max(EDGE_N), 1e-4, 1e-4, target_kl=1e9)
    _, _, logp, ro = _edge_rollout(agent, case, 5)
    lp64 = logp.double().cpu().numpy()
    rs = np.random.RandomState(6)
    for n in EDGE_N:
        for permuted in (False, True):
            rows = rs.permutation(SLOTS)[:n].astype(np.int32) if permuted else np.arange(n, dtype=np.int32)
            rowidx = torch.tensor(rows, device=device).view(1, n) if permuted else None
            rec, kl = _one_armed_update(agent, ro(True), rowidx, n)
            old, new = lp64[rows].mean(), float(rec[ST_LP_MEAN])
            want = old - new
            bound = 2.0 ** -22 * max(1.0, abs(old), abs(new))
            print("   n %4d %s: approx_kl %.7f want %.7f |d| %.2e (bound %.2e)" % (n, "perm" if permuted else "null", kl[0], want,
                                                                                  abs(kl[0] - want), bound))
            assert kl[1] == 0.0
            assert abs(float(kl[0]) - want) <= bound, (n, permuted, kl[0], want, bound)


@pytest.mark.parametrize("mode", MODES)
def test_stored_branch_on_the_fused_route_through_the_epoch_graph(mode, device, monkeypatch):
    """loco_s84 with stored log pi_old: the policy's pass is the fused forward-loss-backward launch, fb_loss_finish_kernel writes
    the record's logprob/mean beside the weight-grad launches, and the KL launch follows the backward. Three updates of 32
    permuted rows, twice (the second run is the whole-run graph's replay, counted): approx_kl == float64 mean(logp_old[rows]) -
    float64(record's logprob/mean) within 2^-22 x max(1, |both means|), both times, with the same bits."""
    from vision4leg_amd.engine import HipTrainer
    monkeypatch.setenv("V4L_COMPUTE", mode)
    monkeypatch.setenv("V4L_EPOCH_GRAPH", "1")
    case = dict(util.CASES["loco_s84"], B=32)
    pf, vf = _nets(case, mode, device)
    agent = _ppo(pf, vf, device, 32, 1e-4, 1e-4, target_kl=1e9)
    slots, U, n = 64, 3, 32
    rs = np.random.RandomState(9)
    net = pf.hip
    net.ensure_bound()
    state, image = net.alloc_rollout(slots, device)
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=device)
    net.ingest(t(util.obs_rows(rs, slots, case)), state, image)
    logp = t(-6.0 + rs.randn(slots) * np.where(rs.rand(slots) < 0.1, 30.0, 0.3))
    ro = HipTrainer.rollout(state, image, t(0.1 * rs.randn(slots, case["A"])), t(rs.randn(slots)), t(rs.randn(slots)),
                            t(rs.randn(slots)), logp)
    rows = np.stack([rs.permutation(slots)[:n] for _ in range(U)]).astype(np.int32)
    lp64 = logp.double().cpu().numpy()
    agent.trainer.sync_target()
    seen = []
    for rep in range(2):
        stats, kl = torch.zeros(U, 24, device=device), torch.full((U, 2), -1.0, device=device)
        agent.run_updates(ro, torch.tensor(rows, device=device), stats, None, kl)
        torch.cuda.synchronize()
        rec, k = stats.cpu().numpy(), kl.cpu().numpy()
        for u in range(U):
            old, new = lp64[rows[u]].mean(), float(rec[u, ST_LP_MEAN])
            bound = 2.0 ** -22 * max(1.0, abs(old), abs(new))
            assert k[u, 1] == 0.0 and abs(float(k[u, 0]) - (old - new)) <= bound, (rep, u, k[u, 0], old - new, bound)
        seen.append(k)
    captures, replays = agent.trainer.kl_graph_counts()
    assert captures >= 2 and replays >= U, (captures, replays)  # single-update graph, then the whole run's


def _sd_build(networks, policies, case):
    import sd_cases as sc
    return sc.build_nets(networks, policies, case)


RECOMPUTED = [("normal", A, tanh) for A in (1, 8, 9, 16) for tanh in (False, True)] + [("sd", 1, False), ("sd", 8, False)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("head,A,tanh", RECOMPUTED, ids=["%s-a%d%s" % (h, A, "-tanh" if t else "") for h, A, t in RECOMPUTED])
def test_recomputed_branch(head, A, tanh, mode, device, monkeypatch):
    """No stored log pi_old: the kernel forms the frozen target's log-probability from the target's head rows. mean(log pi_old) =
    approx_kl + the record's logprob/mean against target_pf.update(obs, acts)["log_prob"].mean() by the two-route rule of
    tests/test_gpu_sd.py::test_rollout_step (1e-5 in f32, 4e-3 in the 16-bit modes, of max(1, |x|)). A in {1, 8, 9, 16} (both
    capacities of the loss kernels' row code and their edges), TanhNormal on and off, GaussianContPolicy (log sigma from the row)
    at A in {1, 8}; n = 257 permuted rows; distinct O(1) means and log sigmas per column, the last log sigma beyond the clamp."""
    monkeypatch.setenv("V4L_COMPUTE", mode)
    n = 257
    kind = "mlp_tanh" if tanh else "mlp"
    case = dict(kind=kind, S=93, A=A, seed=80 + A, B=n, enc=[256, 256], head=[256, 256])
    pf, vf = _nets(case, mode, device, _sd_build if head == "sd" else None)
    if head == "sd":
        import test_gpu_sd as tsd
        w, b = tsd._last(pf)
        with torch.no_grad():
            b[:A].copy_(torch.linspace(-1.5, 1.5, A))
            b[A:].copy_(torch.tensor(util.loss_rows_logstd(A, False)))
    else:
        util.spread_policy_head(pf, logstd=util.loss_rows_logstd(A, tanh))
    agent = _ppo(pf, vf, device, n, 1e-4, 1e-4, target_kl=1e9)
    obs, acts, _, ro = _edge_rollout(agent, case, 7, tanh)
    rows = np.random.RandomState(8).permutation(SLOTS)[:n].astype(np.int32)
    rec, kl = _one_armed_update(agent, ro(False), torch.tensor(rows, device=device).view(1, n), n)
    idx = torch.tensor(rows.astype(np.int64), device=device)
    with torch.no_grad():
        want = agent.target_pf.update(obs[idx], acts[idx])["log_prob"].double().mean().item()
    got = float(kl[0]) + float(rec[ST_LP_MEAN])
    tol = (1e-5 if mode == "f32" else 4e-3) * max(1.0, abs(want))
    print("   %s A=%d tanh=%s %s: mean log pi_old %.6f, target_pf.update %.6f, |d| %.2e (bound %.2e)"
          % (head, A, tanh, mode, got, want, abs(got - want), tol))
    assert np.isfinite(got) and kl[1] == 0.0
    assert abs(got - want) <= tol, (got, want, tol)


# ---- 5. guard and stop together
@pytest.mark.parametrize("mode", MODES)
def test_guard_and_stop_together(mode, device, monkeypatch):
    """A NaN advantage in the first minibatch: the guard skips that policy step and flags it ([1, 0]); approx_kl of that update is
    finite and does not latch. The stop comes later, at the u* of the oracle with both semantics; after it skip_all stays 0 (it
    means "non-finite" only) and the KL column reports the stop."""
    monkeypatch.setenv("V4L_COMPUTE", mode)
    name = "mlp_s93"
    c = kc.CASES[name]
    dat = kc.data(name, nan_update=0)
    a = _agent(name, mode, device, c["target_kl"], guard=True)
    st, kl, skip = _run(a, "epoch-graph", dat, dat[5], monkeypatch)
    ref = _oracle(name, mode, c["target_kl"], nan_update=0, guard=True)
    us = _u_star(kl)
    assert us == ref["u_star"] and us >= 1
    assert skip[0].tolist() == [1, 0] and kl[0, 1] == 0 and np.isfinite(kl[0, 0])
    assert (skip[1:] == 0).all(), skip
    assert (kl[us:, 1] == 1).all() and (kl[:us, 1] == 0).all()
    # the policy stepped in updates 1 .. u* - 1, the critic in 0 .. u*
    assert a.trainer.adam_steps() == (us - 1, us + 1) == (ref["steps"]["pf"], ref["steps"]["vf"])
    assert all(torch.isfinite(v).all() for v in _state(a).values())


# ---- 6. the resident epoch
def test_resident_epoch(device, monkeypatch):
    """DeviceOnPolicyReplayBuffer with log pi_old stored at action time (f16): the logger gets the infos of updates 0 .. u* and none
    after, the last one with kl_stop == 1; last_kl_stop and kl_stops are set; the next epoch opens with a cleared latch."""
    import test_gpu_resume as rsm
    from vision4leg_amd.torchrl.algo import PPO
    from vision4leg_amd.torchrl.collector import VecOnPolicyCollector
    from vision4leg_amd.torchrl.replay_buffers import DeviceOnPolicyReplayBuffer
    monkeypatch.setenv("V4L_COMPUTE", "f16")
    case = util.CASES["mlp_s93"]
    E, T, B = 4, 16, 32
    U = 3 * (E * T // B)
    np.random.seed(3); torch.manual_seed(3); torch.cuda.manual_seed(3)
    pf, vf = rsm._nets(case, case["seed"], device)
    env = util.FakeVecEnv(E, case["S"], case["A"], img=0, seed=9, p_done=0.12, time_limit_key=True)
    eval_env = util.FakeVecEnv(E, case["S"], case["A"], img=0, seed=1, p_done=0.3)
    buf = DeviceOnPolicyReplayBuffer(max_replay_buffer_size=E * T, env_nums=E, time_limit_filter=True)
    coll = VecOnPolicyCollector(vf, env=env, eval_env=eval_env, pf=pf, replay_buffer=buf, device=device, epoch_frames=E * T)
    assert coll.fast_path
    agent = PPO(pf=pf, vf=vf, plr=2e-3, vlr=1e-4, clip_para=0.2, opt_epochs=3, tau=0.95, shuffle=True, entropy_coeff=0.005,
                env=None, replay_buffer=buf, collector=coll, logger=rsm._Log(), device=device, discount=0.99, num_epochs=10,
                batch_size=B, target_kl=0.02)
    seen = 0
    for epoch in range(2):
        agent.current_epoch = epoch
        coll.train_one_epoch()
        agent.update_per_epoch()
        torch.cuda.synchronize()
        assert buf.device_rollout()[-1] is not None  # log pi_old was stored
        infos = agent.logger.updates[seen:]
        seen = len(agent.logger.updates)
        us = len(infos) - 1
        print("   epoch %d: approx_kl %s" % (epoch, [round(i["approx_kl"], 5) for i in infos]))
        assert 1 <= us < U - 1, (us, U)
        assert [i["kl_stop"] for i in infos] == [0] * us + [1]
        assert sorted(infos[0]) == sorted(util.STAT_KEYS + ["approx_kl", "kl_stop"])
        # theta == target but for the critic's first step on the shared base: the epoch opens at the noise floor, latch cleared
        assert abs(infos[0]["approx_kl"]) < 0.01 and infos[-1]["approx_kl"] > 1.5 * 0.02
        assert agent.last_kl_stop == (epoch, us) and agent.kl_stops == epoch + 1
        kl = agent._kl_buf.cpu().numpy()
        assert (kl[us:, 1] == 1).all() and (kl[:us, 1] == 0).all()
        assert agent.trainer.step == (epoch + 1) * U  # every update's launches ran: the stop saves no GPU time on this path
