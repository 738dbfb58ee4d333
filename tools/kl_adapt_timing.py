"""Measurements behind DESIGN.md 2.4 / profiles/kl_adapt_timing.txt (PPO(desired_kl=...), the KL-adaptive learning rates), on
one GPU.
usage: python tools/kl_adapt_timing.py ROOT update {loco|mlp} {off|on[:DESIRED_KL]}
           bench.py's workload of that name (B = 1024, f16, log pi_old stored by the rollout step): wall-clock us per update of
           the epoch's hipGraph replay (48 updates; median and range over EPOCHS epochs, the rollout not timed), then launches
           and summed kernel time per update from one more epoch under the library's HIP-event profiler (eager launches).
           off: desired_kl None; on: desired_kl 0.01 (or the given one), the other three numbers at their defaults; the decisions
           and the rates after each epoch are printed.
       python tools/kl_adapt_timing.py ROOT sha
           sha256 of parameters and Adam moments after two f16 updates of PPO (option off).
ROOT: the tree whose package and bench.py run (a built checkout of this commit, or of the one it is compared with: the parent
commit has no desired_kl, so only `off` and `sha` run there)."""
import ctypes as C
import hashlib
import os
import sys
import time

root, what = sys.argv[1], sys.argv[2]
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
sys.dont_write_bytecode = True
import numpy as np
import torch

dev = torch.device("cuda:0")
EPOCHS = 7


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


from vision4leg_amd import _lib  # noqa: E402
version = _lib.lib().v4l_version()
if what == "update":
    import bench
    name, cfg = sys.argv[3], sys.argv[4]
    desired = None if cfg == "off" else float(cfg.partition(":")[2] or 0.01)
    ep = bench.Epoch(dict(bench.WORKLOADS[name]), "f16", dev, 1)
    U = ep.stats.shape[0]
    if desired is not None:
        ep.agent.desired_kl = desired
    for _ in range(2):  # the second epoch captures the whole-run graph
        ep.step()
    torch.cuda.synchronize()
    us, seen = [], []
    for _ in range(EPOCHS):
        ep.rollout()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ep.update()
        torch.cuda.synchronize()
        us.append(1e6 * (time.perf_counter() - t0) / U)
        if desired is not None:
            d = ep.agent._kl_buf[:, 1].cpu().numpy()
            seen.append("%d down %d up -> (%.3e, %.3e)" % ((d < 0).sum(), (d > 0).sum(), *ep.agent.trainer.lrs()))
    ep.rollout()
    rows = profiled(ep.update)
    print("== %s workload, desired_kl %s (library version %d), B = 1024, f16, %d updates per epoch" % (name, cfg, version, U))
    print("epoch graph: %.1f us per update (median of %d epochs; %.1f .. %.1f)" % (np.median(us), EPOCHS, min(us), max(us)))
    per_update = [r for r in rows if r[1] % U == 0]  # (GAE, target sync and the like run once per epoch)
    print("profiler (eager): %.1f us of kernels in %d launches per update; kl_adapt %.2f us"
          % (sum(r[2] for r in per_update) / U, sum(r[1] for r in per_update) // U,
             sum(r[2] for r in rows if "kl_adapt" in r[0]) / U))
    if desired is not None:
        print("decisions and rates after each epoch: %s" % "; ".join(seen))
    sys.stdout.flush()
else:
    os.environ["V4L_COMPUTE"] = "f16"
    from vision4leg_amd import recipes
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    import util
    from vision4leg_amd.torchrl.algo import PPO

    class Coll:
        epoch_frames = 1
    case = util.CASES["loco_s84"]
    torch.manual_seed(case["seed"])
    pf, vf = recipes.build_nets(networks, policies, case)
    pf, vf = pf.to(dev), vf.to(dev)
    agent = PPO(pf=pf, vf=vf, plr=1e-4, vlr=1e-4, clip_para=0.2, opt_epochs=3, collector=Coll(), batch_size=case["B"], tau=0.95,
                shuffle=True, entropy_coeff=0.005, env=None, replay_buffer=None, logger=None, device=dev, discount=0.99,
                num_epochs=1500, save_dir=None)
    agent.trainer.sync_target()
    for u in range(2):
        b = recipes.make_batch(case, update=u)
        agent.update({k: b[k] for k in ("obs", "acts", "advs", "estimate_returns", "values")})
    torch.cuda.synchronize()
    h = hashlib.sha256()
    tr = agent.trainer
    for t in list(agent.pf.state_dict().values()) + list(agent.vf.state_dict().values()) + [tr.m_pf, tr.v_pf, tr.m_vf, tr.v_vf]:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    print("ppo sha256 %s (library version %d)" % (h.hexdigest(), version), flush=True)
