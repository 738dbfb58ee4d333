"""Measurements behind DESIGN.md 2.3 / profiles/kl_stop_timing.txt (PPO(target_kl=...), the KL early stop), on one GPU.
usage: python tools/kl_stop_timing.py ROOT update {loco|mlp} {off|on|trip[:TARGET_KL]}
           bench.py's workload of that name (B = 1024, f16, log pi_old stored by the rollout step): wall-clock us per update of
           the epoch's hipGraph replay (48 updates; median and range over EPOCHS epochs, the rollout not timed), then launches
           and summed kernel time per update from one more epoch under the library's HIP-event profiler (eager launches).
           off: target_kl None; on: target_kl 1e9 (armed, never trips); trip: a target_kl small enough to trip inside the epoch
           (default 0.002; the update that set the latch is printed per epoch).
       python tools/kl_stop_timing.py ROOT noise {f32|bf16|f16}
           the noise floor: approx_kl of each epoch's first update (theta == target) with stored log pi_old, five epochs of the
           loco workload in that compute mode: how far the rollout step's log pi and the update's differ in the mean.
       python tools/kl_stop_timing.py ROOT sha
           sha256 of parameters and Adam moments after two f16 updates of PPO, V-MPO, A2C and REINFORCE (option off).
ROOT: the tree whose package and bench.py run (a built checkout of this commit, or of the one it is compared with: the parent
commit has no target_kl, so only `off` and `sha` run there)."""
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


def epoch_of(name, compute, target_kl):
    import bench
    wl = dict(bench.WORKLOADS[name])
    ep = bench.Epoch(wl, compute, dev, 1)
    if target_kl is not None:
        ep.agent.target_kl = float(target_kl)
    return ep, ep.stats.shape[0]


from vision4leg_amd import _lib  # noqa: E402
version = _lib.lib().v4l_version()
if what == "update":
    name, cfg = sys.argv[3], sys.argv[4]
    target = None if cfg == "off" else 1e9 if cfg == "on" else float(cfg.partition(":")[2] or 0.002)
    ep, U = epoch_of(name, "f16", target)
    for _ in range(2):  # the second epoch captures the whole-run graph
        ep.step()
    torch.cuda.synchronize()
    us, stops = [], []
    for _ in range(EPOCHS):
        ep.rollout()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ep.update()
        torch.cuda.synchronize()
        us.append(1e6 * (time.perf_counter() - t0) / U)
        if target is not None:
            flags = ep.agent._kl_buf[:, 1].cpu().numpy()
            stops.append(int(np.argmax(flags)) if flags.any() else None)
    ep.rollout()
    rows = profiled(ep.update)
    print("== %s workload, target_kl %s (library version %d), B = 1024, f16, %d updates per epoch" % (name, cfg, version, U))
    print("epoch graph: %.1f us per update (median of %d epochs; %.1f .. %.1f)" % (np.median(us), EPOCHS, min(us), max(us)))
    per_update = [r for r in rows if r[1] % U == 0]  # (GAE, target sync and the like run once per epoch)
    print("profiler (eager): %.1f us of kernels in %d launches per update; kl_stop %.2f us"
          % (sum(r[2] for r in per_update) / U, sum(r[1] for r in per_update) // U,
             sum(r[2] for r in rows if "kl_stop" in r[0]) / U))
    if target is not None:
        print("update that set the latch, per epoch: %s" % stops)
    sys.stdout.flush()
elif what == "noise":
    mode = sys.argv[3]
    ep, U = epoch_of("loco", mode, 1e9)
    first = []
    for _ in range(5):
        ep.step()
        torch.cuda.synchronize()
        first.append(float(ep.agent._kl_buf[0, 0].item()))
    print("noise floor, loco workload, %s (library version %d): approx_kl of each epoch's first update %s"
          % (mode, version, ["%.3e" % v for v in first]))
    a = np.abs(first)
    print("   |approx_kl|: min %.3e median %.3e max %.3e" % (a.min(), np.median(a), a.max()), flush=True)
else:
    os.environ["V4L_COMPUTE"] = "f16"
    from vision4leg_amd import recipes
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    import a2c_cases
    import util
    import vmpo_cases
    from vision4leg_amd.torchrl.algo import A2C, PPO, VMPO, Reinforce
    COMMON = dict(tau=0.95, shuffle=True, entropy_coeff=0.005, env=None, replay_buffer=None, logger=None, device=dev,
                  discount=0.99, num_epochs=1500, save_dir=None)

    class Coll:
        epoch_frames = 1
    keys = ("obs", "acts", "advs", "estimate_returns", "values")
    runs = (("ppo", util.CASES["loco_s84"], False,
             lambda pf, vf, B: PPO(pf=pf, vf=vf, plr=1e-4, vlr=1e-4, clip_para=0.2, opt_epochs=3, collector=Coll(), batch_size=B, **COMMON),
             keys),
            ("vmpo", vmpo_cases.VMPO_CASES["vmpo_mlp"], False,
             lambda pf, vf, B: VMPO(pf=pf, vf=vf, plr=1e-4, vlr=1e-4, opt_epochs=3, collector=Coll(), batch_size=B, **COMMON), keys),
            ("a2c", a2c_cases.A2C_CASES["a2c_mlp"], True,
             lambda pf, vf, B: A2C(pf=pf, vf=vf, plr=1e-4, vlr=1e-4, collector=Coll(), batch_size=B, **COMMON), keys[:4]),
            ("reinforce", util.CASES["mlp_s93"], False,
             lambda pf, vf, B: Reinforce(pf=pf, plr=1e-4, collector=Coll(), batch_size=B, **COMMON), keys[:4]))
    for tag, case, disjoint, make, ks in runs:
        torch.manual_seed(case["seed"])
        build = a2c_cases.build_nets if disjoint else recipes.build_nets
        pf, vf = build(networks, policies, case)
        pf, vf = pf.to(dev), vf.to(dev)
        agent = make(pf, vf, case["B"])
        if tag in ("ppo", "vmpo"):
            agent.trainer.sync_target()
        for u in range(2):
            b = recipes.make_batch(case, update=u)
            agent.update({k: b[k] for k in ks})
        torch.cuda.synchronize()
        h = hashlib.sha256()
        tr = agent.trainer
        for t in list(agent.pf.state_dict().values()) + list(agent.vf.state_dict().values()) + [tr.m_pf, tr.v_pf, tr.m_vf, tr.v_vf]:
            h.update(t.detach().cpu().contiguous().numpy().tobytes())
        print("%s sha256 %s" % (tag, h.hexdigest()), flush=True)
