"""Measurements behind DESIGN.md 4.13 / profiles/ppo_cat_timing.txt (algo.PPODiscrete on policies.CategoricalDisPolicy next to algo.PPO
on policies.GaussianContPolicy, the state-dependent-sigma policy, on the same net), on one GPU.
usage: python tools/ppo_cat_timing.py ROOT {cat|sd} {host|resident}
  launches and kernel time per update (the library's HIP-event profiler: eager launches, sum of kernel times, 10 updates after 2),
  then the wall time per update of a run of 48 updates as ONE hipGraph replay (resident only: torch events around
  PPO.run_updates, 5 replays after the capture), B = 1024, f16.
  host: update(batch) — the frozen target's forward runs; resident: a device rollout with stored log pi_old — it does not.
ROOT: the tree whose package runs (a built checkout of this commit, or of the one it is compared with: the parent commit has no
PPODiscrete, so only `sd` runs there). The net: S 93, six actions (K = 6 logits / A = 6: a 12-column head), 256-256 base and
head, vf.base = pf.base."""
import ctypes as C
import os
import sys

root, pol, kind = sys.argv[1:4]
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
sys.dont_write_bytecode = True
import numpy as np
import torch

CASE = dict(kind="mlp", S=93, A=6, K=6, seed=88, B=1024, enc=[256, 256], head=[256, 256], scale=600.0, shared=True)
dev = torch.device("cuda:0")
os.environ["V4L_COMPUTE"] = "f16"
B = CASE["B"]


class Coll:
    epoch_frames = 1


def profiled(fn):
    from vision4leg_amd import _lib
    L = _lib.lib()
    torch.cuda.synchronize()
    L.v4l_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
        buf = C.create_string_buffer(1 << 20)
        L.v4l_prof_collect(buf, len(buf))
    finally:
        L.v4l_prof_enable(0)
    rows = []
    for line in buf.value.decode().splitlines():
        label, calls, us, _ = line.split("\t")
        rows.append((label, int(calls), float(us)))
    return rows


def table(title, rows, per):
    print("== %s" % title)
    print("kernel time per update: %.1f us in %d launches" % (sum(r[2] for r in rows) / per, sum(r[1] for r in rows) // per))
    print("%-46s %6s %12s" % ("phase|op|kernel", "calls", "us/update"))
    for label, calls, us in rows:
        print("%-46s %6.1f %12.2f" % (label, calls / per, us / per))
    sys.stdout.flush()


def batch(u):
    from vision4leg_amd import recipes
    b = recipes.make_batch(CASE, update=u)
    out = {k: b[k] for k in ("obs", "acts", "advs", "estimate_returns", "values")}
    if pol == "cat":
        out["acts"] = np.random.RandomState(500 + u).randint(0, CASE["K"], size=B).astype(np.int64)
    return out


import vision4leg_amd.torchrl.networks as networks  # noqa: E402
import vision4leg_amd.torchrl.policies as policies  # noqa: E402
from vision4leg_amd import _lib  # noqa: E402
from vision4leg_amd.engine import HipTrainer  # noqa: E402
version = _lib.lib().v4l_version()
torch.manual_seed(CASE["seed"])
if pol == "cat":
    import ppo_cat_cases
    from vision4leg_amd.torchrl.algo import PPODiscrete as Learner
    pf, vf = ppo_cat_cases.build_nets(networks, policies, CASE)
else:
    import sd_cases
    from vision4leg_amd.torchrl.algo import PPO as Learner
    pf, vf = sd_cases.build_nets(networks, policies, CASE)
pf, vf = pf.to(dev), vf.to(dev)
agent = Learner(pf=pf, vf=vf, plr=1e-4, vlr=1e-4, clip_para=0.2, opt_epochs=3, tau=0.95, shuffle=True, entropy_coeff=0.005, env=None,
                replay_buffer=None, collector=Coll(), logger=None, device=dev, discount=0.99, num_epochs=1500, batch_size=B,
                save_dir=None)
agent.trainer.sync_target()
title = "%s update, %s policy, %s (library version %d), B = 1024, f16" % (Learner.__name__, pol, kind, version)
N = 10
if kind == "host":
    for u in range(2):
        agent.update(batch(u))
    table(title, profiled(lambda: [agent.update(batch(2 + u)) for u in range(N)]), N)
else:
    U = 48
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    bs = [batch(u) for u in range(4)]
    hip = pf.hip
    hip.ensure_bound()
    slots = len(bs) * B
    st, im = hip.alloc_rollout(slots, dev)
    hip.ingest(up(np.concatenate([b["obs"] for b in bs])), st, im)
    cat = lambda k: up(np.concatenate([b[k] for b in bs]))
    acts = cat("acts").reshape(slots, -1)
    thip = agent.target_pf.hip  # log pi_old of the synchronised target at the stored actions: every ratio starts at 1
    tout = thip.forward(st, im, slots)
    if pol == "cat":
        logp = thip.cat_head(tout, slots, acts)[2].clone()
    else:
        logp = thip.gauss_head(tout, None, slots, acts)[4].reshape(slots).clone()
    ro = HipTrainer.rollout(st, im, acts, cat("advs").reshape(-1), cat("estimate_returns").reshape(-1), cat("values").reshape(-1), logp)
    rs = np.random.RandomState(1)
    rowidx = torch.from_numpy(np.stack([rs.permutation(slots)[:B] for _ in range(U)]).astype(np.int32)).to(dev)
    stats = torch.zeros(U, _lib.V4L_STATS, dtype=torch.float32, device=dev)
    agent.run_updates(ro, rowidx[:2].contiguous(), stats[:2])
    table(title, profiled(lambda: agent.run_updates(ro, rowidx[:N].contiguous(), stats[:N])), N)
    agent._rowidx_buf = None
    for _ in range(3):  # update by update, then the capture of the whole run, then a replay
        agent.run_updates(ro, rowidx, stats)
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        agent.run_updates(ro, rowidx, stats)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1000.0 / U)
    print("wall time per update, %d updates as one hipGraph replay: %s us (5 replays; median %.1f)"
          % (U, " ".join("%.1f" % t for t in times), float(np.median(times))))
    print("records finite: %s" % bool(torch.isfinite(stats[:, :18]).all().item()))
