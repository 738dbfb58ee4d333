"""-m gpu: a V-MPO run of updates as hipGraph replays (v4l_trainer_vmpo_update_next / _update_run, library version 111) against
the eager launch sequence. The captured updates launch the kernels the eager ones launch with the same arguments, so every
comparison here is torch.equal / ==; v4l_trainer_vmpo_graph_counts tells a replay from an eager run that gave the same bits.

Row blocks: U = 3 blocks of B rows drawn over a rollout of 2 B rows; the draw is re-seeded until no block's selection sits on a
tie (vmpo_cases.tie_gap > TIE_GAP_MIN, the rule tests/test_vmpo_cpu.py::test_seed_rule states)."""
import numpy as np
import pytest
import torch

import test_gpu_parity as par
import test_gpu_vmpo as tv
import util
import vmpo_cases as vc
from vmpo_cases import LR, VMPO_CASES

pytestmark = pytest.mark.gpu

U = 3
CASE_MODES = [(name, mode) for name, case in VMPO_CASES.items()
              for mode in (("f16", "bf16", "f32") if case["kind"].startswith("mlp") else ("f16", "f32"))]


def _rollout_data(case, n_rows=None, blocks=U):
    """2 B seeded rollout rows and `blocks` row blocks of n_rows (default B) slots each, none on a selection tie."""
    B = case["B"]
    n = B if n_rows is None else n_rows
    rs = np.random.RandomState(7000 + case["seed"])
    obs = util.obs_rows(rs, 2 * B, case)
    acts, advs, rets, vals = 0.1 * rs.randn(2 * B, case["A"]), rs.randn(2 * B), rs.randn(2 * B), rs.randn(2 * B)
    for attempt in range(20):
        rr = np.random.RandomState(100 * case["seed"] + n + 1000 * attempt)
        rows = np.stack([rr.permutation(2 * B)[:n] for _ in range(blocks)]).astype(np.int32)
        if all(vc.tie_gap(advs[r].astype(np.float32)) > vc.TIE_GAP_MIN for r in rows):
            return dict(obs=obs, acts=acts, advs=advs, rets=rets, vals=vals), rows
    raise AssertionError("no tie-free draw of row blocks")


class _Twin:
    """A VMPO agent's trainer over a device-resident rollout, driven through the engine: call() opens a run with begin() and
    makes `count` updates, eagerly (graph=False) or through vmpo_update_run(graph=True)."""

    def __init__(self, case, mode, device, data, rows, graph):
        from vision4leg_amd.engine import HipTrainer
        self.agent, self.pf, self.vf = tv._agent(case, mode, device)
        self.tr, self.graph, self.device = self.agent.trainer, graph, device
        net = self.pf.hip
        net.ensure_bound()
        t = lambda a: torch.tensor(a, dtype=torch.float32, device=device)
        state, image = net.alloc_rollout(len(data["obs"]), device)
        net.ingest(t(data["obs"]), state, image)
        self.ro = HipTrainer.rollout(state, image, t(data["acts"]), t(data["advs"]), t(data["rets"]), t(data["vals"]))
        self.tr.sync_target()
        self.set_rows(rows)
        torch.cuda.synchronize()

    def set_rows(self, rows):
        from vision4leg_amd import _lib
        self.rows = torch.tensor(rows, device=self.device)
        self.stats = torch.zeros(len(rows), _lib.V4L_STATS, dtype=torch.float32, device=self.device)
        self.move_vstats()

    def move_vstats(self):
        from vision4leg_amd import _lib
        self.vstats = torch.zeros(len(self.rows), _lib.V4L_VMPO_STATS, dtype=torch.float32, device=self.device)

    def call(self, count=U):
        tr, n = self.tr, self.rows.shape[1]
        tr.stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(tr.stream):
            tr._pre(n)
            tr.begin(self.rows, self.stats, LR, LR)
            if self.graph:
                tr.vmpo_update_run(self.ro, n, count, self.vstats, graph=True)
            else:
                for _ in range(count):
                    tr.vmpo_update_next(self.ro, n, self.vstats, graph=False)
        torch.cuda.synchronize()

    def snapshot(self):
        tr = self.tr
        out = {"pf/" + k: v.detach().cpu().clone() for k, v in self.pf.state_dict().items()}
        out.update({"vf/" + k: v.detach().cpu().clone() for k, v in self.vf.state_dict().items()})
        for k in ("m_pf", "v_pf", "m_vf", "v_vf"):
            out[k] = getattr(tr, k).detach().cpu().clone()
        out["vmpo_state"] = torch.tensor(tr.vmpo_state(), dtype=torch.float64)
        out["stats"], out["vstats"] = self.stats.cpu().clone(), self.vstats.cpu().clone()
        return out


def _assert_same(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        # (a NaN slot — log_std/std of a 1-dimensional policy — would compare unequal to itself: none of these cases has one)
        assert torch.equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("name,mode", CASE_MODES)
def test_run_equals_eager(name, mode, device):
    """Nine updates eagerly against three vmpo_update_run(..., 3, graph=True) calls — eager + single replays, the capture of the
    run, its replay — compared after each call: parameters, Adam moments, the V-MPO state, both record arrays."""
    case = VMPO_CASES[name]
    data, rows = _rollout_data(case)
    eager = _Twin(case, mode, device, data, rows, graph=False)
    graph = _Twin(case, mode, device, data, rows, graph=True)
    assert graph.tr.vmpo_graph_counts() == (0, 0)
    counts = []
    for call in range(3):
        eager.call()
        graph.call()
        a, b = eager.snapshot(), graph.snapshot()
        _assert_same(a, b, "call %d" % call)
        assert torch.isfinite(b["stats"][:, :18]).all() and torch.isfinite(b["vstats"]).all()
        counts.append(graph.tr.vmpo_graph_counts())
    print("\n[%s %s] (captures, replays) after each call: %s" % (name, mode, counts))
    # call 1: one eager update, the single-update graph captured, two replays; call 2: the run captured and replayed
    assert counts[0] == (1, U - 1) and counts[1] == (2, U)
    assert counts[2] == (counts[1][0], counts[1][1] + 1)  # call 3: exactly one replay, no capture
    assert eager.tr.vmpo_graph_counts() == (0, 0)
    assert graph.tr.vmpo_state()[6] == 3 * U and graph.tr.adam_steps() == (3 * U,) * 2 and graph.tr.step == 3 * U
    assert (b["vstats"][:, 2] != 1.0).all()  # eta moved: the scalars' optimiser ran inside the replays
    assert graph.agent.f16_saturated == 0


def test_key_changes_recapture(device):
    """After a captured run: another count, a larger minibatch (re-bind + HipTrainer._vmpo_regrow: a new V-MPO block) and a
    moved V-MPO record tensor each capture again instead of replaying what was captured before — the capture count rises and
    the bits stay the eager twin's."""
    case, mode = VMPO_CASES["vmpo_mlp"], "f16"
    data, rows = _rollout_data(case)
    eager = _Twin(case, mode, device, data, rows, graph=False)
    graph = _Twin(case, mode, device, data, rows, graph=True)

    def both(what, count=U):
        eager.call(count)
        graph.call(count)
        _assert_same(eager.snapshot(), graph.snapshot(), what)
        return graph.tr.vmpo_graph_counts()
    for call in range(3):
        cap, rep = both("warm-up %d" % call)
    assert (cap, rep) == (2, U + 1)
    # another count: the run's graph holds three updates
    cap2, rep2 = both("count 2", count=2)
    assert cap2 == cap + 1 and rep2 == rep + 1
    cap2, rep2 = both("count 2 again", count=2)
    assert (cap2, rep2) == (cap + 1, rep + 2)
    # a larger minibatch: the workspace and the V-MPO block move
    _, rows_big = _rollout_data(case, n_rows=case["B"] + 32)
    block = graph.tr._vmpo[1].data_ptr()
    for tw in (eager, graph):
        tw.set_rows(rows_big)
    cap3, rep3 = both("larger minibatch")
    assert graph.tr._vmpo[1].data_ptr() != block and graph.tr.batch == case["B"] + 32
    assert (cap3, rep3) == (cap2 + 1, rep2 + U - 1)  # first update eagerly, then the single-update graph of the new shape
    cap3, rep3 = both("larger minibatch, run")
    assert (cap3, rep3) == (cap2 + 2, rep2 + U)
    # the V-MPO record tensor moves (the row and PPO record tensors stay): only the V-MPO key sees it
    old = graph.vstats
    old_bits = old.cpu().clone()
    for tw in (eager, graph):
        tw.move_vstats()
    assert graph.vstats.data_ptr() != old.data_ptr()
    cap4, rep4 = both("moved records")
    assert (cap4, rep4) == (cap3 + 1, rep3 + U - 1)
    assert (graph.vstats != 0).any() and torch.equal(old.cpu(), old_bits)  # nothing wrote where the dropped graphs did
    cap4, rep4 = both("moved records, run")
    assert (cap4, rep4) == (cap3 + 2, rep3 + U)


# ------------------------------------------------------------------------------------------ the shell's epoch
def _epoch_stack(device, mode="f16"):
    from vision4leg_amd import recipes
    from vision4leg_amd.torchrl.algo import VMPO
    from vision4leg_amd.torchrl.collector import VecOnPolicyCollector
    from vision4leg_amd.torchrl.replay_buffers import DeviceOnPolicyReplayBuffer
    case = dict(VMPO_CASES["vmpo_mlp"], B=32)
    E, T, B = 4, 16, 32
    pf, vf = par._build(case, mode, device)
    buf = DeviceOnPolicyReplayBuffer(max_replay_buffer_size=E * T, env_nums=E, time_limit_filter=True)
    coll = VecOnPolicyCollector(vf, env=recipes.ZeroCostVecEnv(E, case, seed=2, p_done=0.1), eval_env=recipes.ZeroCostVecEnv(E, case, seed=3),
                                pf=pf, replay_buffer=buf, device=device, epoch_frames=E * T)
    log = tv._Log()
    agent = VMPO(pf=pf, vf=vf, plr=LR, vlr=LR, opt_epochs=2, tau=0.95, shuffle=True, entropy_coeff=0.005, env=None,
                 replay_buffer=buf, collector=coll, logger=log, device=device, discount=0.99, num_epochs=10, batch_size=B)
    return agent, coll, log, pf, vf


def _three_epochs(device):
    agent, coll, log, pf, vf = _epoch_stack(device)
    np.random.seed(3); torch.manual_seed(3); torch.cuda.manual_seed(3)
    counts = []
    for _ in range(3):
        coll.train_one_epoch()
        agent.update_per_epoch()
        torch.cuda.synchronize()
        counts.append(agent.trainer.vmpo_graph_counts())
    params = {tag + k: v.detach().cpu().clone() for tag, net in (("pf/", pf), ("vf/", vf)) for k, v in net.state_dict().items()}
    return agent, counts, log.updates, params, (agent.eta.item(), agent.alpha.item())


def test_epoch_default_is_one_replay(device, monkeypatch):
    """update_per_epoch on a DeviceOnPolicyReplayBuffer (tests/test_gpu_vmpo.py::test_resident_epoch's setup: four updates an
    epoch), three epochs: the first runs update by update, the second captures the run, from then on an epoch is ONE replay;
    V4L_EPOCH_GRAPH=0 replays once per update; a twin built under V4L_GRAPH=0 never replays and logs the same infos."""
    monkeypatch.delenv("V4L_GRAPH", raising=False)
    monkeypatch.delenv("V4L_EPOCH_GRAPH", raising=False)
    agent, counts, infos, params, scalars = _three_epochs(device)
    assert agent.use_graph and len(infos) == 12 and agent.training_update_num == 12
    print("\n(captures, replays) after each epoch: %s" % counts)
    assert counts[0] == (1, 3)                      # eager, the single-update graph, three replays
    assert counts[1] == (2, 4)                      # the run captured, one replay
    assert counts[2] == (2, 5)                      # one replay, nothing captured
    monkeypatch.setenv("V4L_EPOCH_GRAPH", "0")
    _, counts_u, infos_u, params_u, scalars_u = _three_epochs(device)
    assert counts_u == [(1, 3), (1, 7), (1, 11)]     # U replays per epoch once the configuration is warm
    monkeypatch.delenv("V4L_EPOCH_GRAPH")
    monkeypatch.setenv("V4L_GRAPH", "0")
    twin, counts_e, infos_e, params_e, scalars_e = _three_epochs(device)
    assert not twin.use_graph and counts_e == [(0, 0)] * 3
    for other_infos, other_params, other_scalars in ((infos_e, params_e, scalars_e), (infos_u, params_u, scalars_u)):
        assert infos == other_infos
        assert scalars == other_scalars
        for k in params:
            assert torch.equal(params[k], other_params[k]), k
    assert np.isfinite([v for i in infos for v in i.values()]).all()


def test_update_batch_goes_through_the_single_replay(device, monkeypatch):
    """update(batch), the host-batch path with U = 1: the staged rollout arrays keep their addresses, so the second call
    captures the single-update graph and later calls replay it."""
    monkeypatch.delenv("V4L_GRAPH", raising=False)
    case = VMPO_CASES["vmpo_mlp"]
    agent, pf, vf = tv._agent(case, "f16", device)
    agent.trainer.sync_target()
    seen = []
    for u in range(3):
        b = util.make_batch(case, update=u)
        agent.update({k: b[k] for k in tv.BATCH_KEYS})
        seen.append(agent.trainer.vmpo_graph_counts())
    assert seen == [(0, 0), (1, 1), (1, 2)]


# ------------------------------------------------------------------------------------------ PPO beside it
def test_ppo_and_vmpo_graphs_do_not_mix(device, monkeypatch):
    """One process, nets of the same shapes: a PPO agent's captured epoch replayed before and after a V-MPO agent captured and
    replayed its own gives the bits of a PPO agent that ran its four epochs undisturbed."""
    from vision4leg_amd import _lib
    from vision4leg_amd.engine import HipTrainer
    from vision4leg_amd.torchrl.algo import PPO
    monkeypatch.delenv("V4L_GRAPH", raising=False)
    monkeypatch.delenv("V4L_EPOCH_GRAPH", raising=False)
    mode = "f16"
    case = dict(VMPO_CASES["vmpo_mlp"], B=32)
    data, rows = _rollout_data(case)
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=device)

    def stack(cls, **kw):
        agent, pf, vf = tv._agent(case, mode, device, cls=cls, **kw)
        net = pf.hip
        net.ensure_bound()
        state, image = net.alloc_rollout(len(data["obs"]), device)
        net.ingest(t(data["obs"]), state, image)
        ro = HipTrainer.rollout(state, image, t(data["acts"]), t(data["advs"]), t(data["rets"]), t(data["vals"]))
        agent.trainer.sync_target()
        return agent, pf, vf, ro

    def ppo_epoch(st):
        agent, _, _, ro = st
        stats = torch.zeros(U, _lib.V4L_STATS, dtype=torch.float32, device=device)
        agent.run_updates(ro, torch.tensor(rows, device=device), stats)
        torch.cuda.synchronize()
        return stats.cpu()

    alone = stack(PPO, clip_para=0.2)
    want = [ppo_epoch(alone) for _ in range(4)]
    mixed = stack(PPO, clip_para=0.2)
    got = [ppo_epoch(mixed) for _ in range(3)]  # update by update, the capture of the run, its replay
    vm = stack(None)
    vagent, _, _, vro = vm
    vinfos = [vagent._run(vro, torch.tensor(rows, device=device), case["B"], U, lambda u: "update %d" % u) for _ in range(3)]
    torch.cuda.synchronize()
    assert vagent.trainer.vmpo_graph_counts() == (2, U + 1)
    assert np.isfinite([v for ep in vinfos for i in ep for v in i.values()]).all()
    got.append(ppo_epoch(mixed))  # PPO's run graph again, after V-MPO's
    for ep in range(4):
        assert torch.equal(want[ep], got[ep]), ep
    for a, b in ((alone[1], mixed[1]), (alone[2], mixed[2])):
        for k, v in a.state_dict().items():
            assert torch.equal(v, b.state_dict()[k]), k
    assert mixed[0].trainer.vmpo_graph_counts() == (0, 0)
