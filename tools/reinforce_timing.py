"""Measurements behind DESIGN.md 4.11 / profiles/reinforce_timing.txt (algo.Reinforce next to algo.A2C and algo.PPO), on one GPU
with the library's HIP-event profiler.
usage: python tools/reinforce_timing.py ROOT update {reinforce|a2c|ppo} {mlp|loco}   launches and kernel time per update, B = 1024, f16
       python tools/reinforce_timing.py ROOT rollout {zero|real} {mlp|loco}          the fused rollout step, E = 32, f16: pf with
                                                                                      networks.zero_critic(pf) | the starters' pair
       python tools/reinforce_timing.py ROOT sha                                      sha256 of parameters and Adam moments after two
                                                                                      updates of PPO, V-MPO and A2C (f16)
ROOT: the tree whose package runs (a built checkout of this commit, or of the one it is compared with; the parent commit has no
algo.Reinforce and no zero critic)."""
import ctypes as C
import hashlib
import os
import sys

root, what = sys.argv[1], sys.argv[2]
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
sys.dont_write_bytecode = True
import numpy as np
import torch

CASES = {
    "mlp": dict(kind="mlp", S=93, A=6, seed=87, B=1024, enc=[256, 256], head=[256, 256]),
    "loco": dict(kind="loco", S=84, A=6, seed=81, B=1024, enc=[256, 256], head=[256, 256], layers=2, ff=256),
}
dev = torch.device("cuda:0")
os.environ["V4L_COMPUTE"] = "f16"
COMMON = dict(tau=0.95, shuffle=True, entropy_coeff=0.005, env=None, replay_buffer=None, logger=None, device=dev, discount=0.99,
              num_epochs=1500, save_dir=None)


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


def table(title, rows, per, unit):
    print("== %s" % title)
    print("kernel time per %s: %.1f us in %d launches" % (unit, sum(r[2] for r in rows) / per, sum(r[1] for r in rows) // per))
    print("%-46s %6s %12s" % ("phase|op|kernel", "calls", "us/" + unit))
    for label, calls, us in rows:
        print("%-46s %6.1f %12.2f" % (label, calls / per, us / per))
    sys.stdout.flush()


def nets(case, disjoint=False):
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    from vision4leg_amd import recipes
    torch.manual_seed(case["seed"])
    if disjoint:  # what algo.A2C takes: a state-MLP pair without a common parameter
        import a2c_cases
        pf, vf = a2c_cases.build_nets(networks, policies, case)
    else:
        pf, vf = recipes.build_nets(networks, policies, case)
    return pf.to(dev), vf.to(dev)


if what == "update":
    from vision4leg_amd import _lib, recipes
    algo, kind = sys.argv[3], sys.argv[4]
    case = CASES[kind]
    B = case["B"]
    if algo == "reinforce":
        from vision4leg_amd.torchrl.algo import Reinforce
        pf, _ = nets(case)
        agent = Reinforce(pf=pf, plr=1e-4, collector=Coll(), batch_size=B, **COMMON)
        keys = ("obs", "acts", "advs", "estimate_returns")
    elif algo == "a2c":
        from vision4leg_amd.torchrl.algo import A2C
        pf, vf = nets(case, disjoint=True)
        agent = A2C(pf=pf, vf=vf, plr=1e-4, vlr=1e-4, collector=Coll(), batch_size=B, **COMMON)
        keys = ("obs", "acts", "advs", "estimate_returns")
    else:
        from vision4leg_amd.torchrl.algo import PPO
        pf, vf = nets(case)
        agent = PPO(pf=pf, vf=vf, plr=1e-4, vlr=1e-4, clip_para=0.2, opt_epochs=3, collector=Coll(), batch_size=B, **COMMON)
        agent.trainer.sync_target()
        keys = ("obs", "acts", "advs", "estimate_returns", "values")
    N = 10
    batches = [recipes.make_batch(case, update=u) for u in range(N + 2)]
    pick = lambda b: {k: b[k] for k in keys}
    for u in range(2):
        agent.update(pick(batches[u]))
    rows = profiled(lambda: [agent.update(pick(batches[2 + u])) for u in range(N)])
    table("%s update, %s nets (library version %d), B = 1024, f16" % (algo, kind, _lib.lib().v4l_version()), rows, N, "update")
elif what == "rollout":
    from vision4leg_amd import _lib, engine, recipes
    critic, kind = sys.argv[3], sys.argv[4]
    case = CASES[kind]
    pf, vf = nets(case)
    if critic == "zero":
        import vision4leg_amd.torchrl.networks as networks
        vf = networks.zero_critic(pf).to(dev)
    E, T = 32, 24
    actor = engine.HipActor(pf.hip, vf.hip, E, shared_encoder=True, graph=False)
    net = pf.hip
    net.ensure_bound()
    state, image = net.alloc_rollout(T * E, dev)
    A = case["A"]
    acts, vals, logp = torch.zeros(T * E, A, device=dev), torch.ones(T * E, device=dev), torch.zeros(T * E, device=dev)
    actor.attach((state, image, acts, vals, logp))
    actor.seek(0)
    obs = torch.tensor(recipes.obs_rows(np.random.RandomState(3), T * E, case), dtype=torch.float32, device=dev)
    for s in range(4):
        actor.step(obs[s * E:(s + 1) * E])
    rows = profiled(lambda: [actor.step(obs[s * E:(s + 1) * E]) for s in range(4, T)])
    torch.cuda.synchronize()
    route = actor.route() if hasattr(actor, "route") else "?"
    table("rollout step, %s nets, %s critic, E = 32, f16, route %s (library version %d)"
          % (kind, critic, route, _lib.lib().v4l_version()), rows, T - 4, "step")
    print("filed values: min %.3g max %.3g" % (vals.min().item(), vals.max().item()))
else:
    from vision4leg_amd import recipes
    import a2c_cases
    import vmpo_cases
    from vision4leg_amd.torchrl.algo import A2C, PPO, VMPO
    ppo_keys = ("obs", "acts", "advs", "estimate_returns", "values")
    import util
    runs = (("ppo", util.CASES["mlp_s93"], False,
             lambda pf, vf, B: PPO(pf=pf, vf=vf, plr=1e-4, vlr=1e-4, clip_para=0.2, opt_epochs=3, collector=Coll(), batch_size=B, **COMMON),
             ppo_keys),
            ("vmpo", vmpo_cases.VMPO_CASES["vmpo_mlp"], False,
             lambda pf, vf, B: VMPO(pf=pf, vf=vf, plr=1e-4, vlr=1e-4, opt_epochs=3, collector=Coll(), batch_size=B, **COMMON), ppo_keys),
            ("a2c", a2c_cases.A2C_CASES["a2c_mlp"], True,
             lambda pf, vf, B: A2C(pf=pf, vf=vf, plr=1e-4, vlr=1e-4, collector=Coll(), batch_size=B, **COMMON), ppo_keys[:4]))
    for tag, case, disjoint, make, keys in runs:
        pf, vf = nets(case, disjoint)
        agent = make(pf, vf, case["B"])
        if tag != "a2c":
            agent.trainer.sync_target()
        for u in range(2):
            b = recipes.make_batch(case, update=u)
            agent.update({k: b[k] for k in keys})
        torch.cuda.synchronize()
        h = hashlib.sha256()
        tr = agent.trainer
        for t in list(pf.state_dict().values()) + list(vf.state_dict().values()) + [tr.m_pf, tr.v_pf, tr.m_vf, tr.v_vf]:
            h.update(t.detach().cpu().contiguous().numpy().tobytes())
        print("%s sha256 %s" % (tag, h.hexdigest()), flush=True)
