"""Measurements behind DESIGN.md 4.10 / profiles/sd_policy_timing.txt (policies.GaussianContPolicy against its twin with a logstd
parameter), on one GPU with the library's HIP-event profiler.
usage: python tools/sd_policy_timing.py ROOT sha             sha256 of parameters and Adam moments after two PPO.update calls
       python tools/sd_policy_timing.py ROOT time {sd|bb}    update and rollout-step timings, GaussianContPolicy | the twin
ROOT: the tree whose package runs (a built checkout of this commit, or of the one it is compared with)."""
import ctypes as C
import hashlib
import os
import sys

root, what = sys.argv[1], sys.argv[2]
sys.path.insert(0, root)
sys.dont_write_bytecode = True
import numpy as np
import torch

CASES = {
    "loco_s84": dict(kind="loco", S=84, A=6, seed=1, B=32, enc=[256, 256], head=[256, 256], layers=2, ff=256),
    "cnn_s93": dict(kind="cnn", S=93, A=6, seed=2, B=64, enc=[256, 256], head=[256, 256], visual_dim=256),
    "mlp_s93": dict(kind="mlp", S=93, A=6, seed=3, B=128, enc=[256, 256], head=[256, 256]),
}
dev = torch.device("cuda:0")


def agent_of(pf, vf, B):
    from vision4leg_amd.torchrl.algo import PPO

    class Coll: epoch_frames = 1
    return PPO(pf=pf, vf=vf, plr=1e-4, vlr=1e-4, clip_para=0.2, opt_epochs=3, tau=0.95, shuffle=True, entropy_coeff=0.005,
               env=None, replay_buffer=None, collector=Coll(), logger=None, device=dev, discount=0.99, num_epochs=1500,
               batch_size=B, save_dir=None)


def build(case, sd=False):
    import vision4leg_amd.torchrl.networks as networks
    import vision4leg_amd.torchrl.policies as policies
    from vision4leg_amd import recipes
    torch.manual_seed(case["seed"])
    if not sd:
        pf, vf = recipes.build_nets(networks, policies, case)
    else:
        net = {"append_hidden_shapes": list(case["head"]), "base_type": networks.MLPBase, "hidden_shapes": list(case["enc"])}
        pf = policies.GaussianContPolicy(input_shape=case["S"], output_shape=2 * case["A"], **net)
        vf = networks.Net(input_shape=(case["S"],), output_shape=1, **net)
        vf.base = pf.base
    return pf.to(dev), vf.to(dev)


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


if what == "sha":
    from vision4leg_amd import recipes
    for name, case in CASES.items():
        for mode in ("f16", "f32"):
            os.environ["V4L_COMPUTE"] = mode
            pf, vf = build(case)
            agent = agent_of(pf, vf, case["B"])
            agent.trainer.sync_target()
            for u in range(2):
                b = recipes.make_batch(case, update=u)
                agent.update({k: b[k] for k in ("obs", "acts", "advs", "estimate_returns", "values")})
            torch.cuda.synchronize()
            h = hashlib.sha256()
            for net in (pf, vf):
                for k, v in net.state_dict().items():
                    h.update(k.encode()); h.update(v.detach().cpu().numpy().tobytes())
            tr = agent.trainer
            for k in ("m_pf", "v_pf", "m_vf", "v_vf"):
                h.update(getattr(tr, k).detach().cpu().numpy().tobytes())
            print("ppo sha256 %s %s %s" % (name, mode, h.hexdigest()), flush=True)
else:
    from vision4leg_amd import _lib, recipes
    sd = sys.argv[3] == "sd"
    os.environ["V4L_COMPUTE"] = "f16"
    case = dict(CASES["mlp_s93"], B=1024, seed=76)
    pf, vf = build(case, sd)
    agent = agent_of(pf, vf, case["B"])
    agent.trainer.sync_target()
    batches = [recipes.make_batch(case, update=u) for u in range(12)]
    pick = lambda b: {k: b[k] for k in ("obs", "acts", "advs", "estimate_returns", "values")}
    for u in range(2):
        agent.update(pick(batches[u]))
    N = 10
    rows = profiled(lambda: [agent.update(pick(batches[2 + u])) for u in range(N)])
    tag = "GaussianContPolicy" if sd else "GaussianContPolicyBasicBias"
    print("== PPO update, %s (library version %d), B = 1024, f16" % (tag, _lib.lib().v4l_version()))
    print("kernel time per update: %.1f us in %d launches" % (sum(r[2] for r in rows) / N, sum(r[1] for r in rows) // N))
    print("%-46s %6s %12s" % ("phase|op|kernel", "calls", "us/update"))
    for label, calls, us in rows:
        print("%-46s %6.1f %12.2f" % (label, calls / N, us / N))
    # the same update fed log pi_old stored at action time (no target forward; the loss launch evaluates one policy per row)
    from vision4leg_amd.engine import HipTrainer
    n = case["B"]
    net = pf.hip
    net.ensure_bound()
    st_, im_ = net.alloc_rollout(n, dev)
    b0 = batches[0]
    net.ingest(torch.tensor(b0["obs"], dtype=torch.float32, device=dev), st_, im_)
    t32 = lambda a: torch.tensor(np.asarray(a).reshape(-1), dtype=torch.float32, device=dev)
    ro = HipTrainer.rollout(st_, im_, torch.tensor(b0["acts"], dtype=torch.float32, device=dev), t32(b0["advs"]),
                            t32(b0["estimate_returns"]), t32(b0["values"]), torch.full((n,), -float(case["A"]), device=dev))
    rows_ix = torch.arange(n, dtype=torch.int32, device=dev).view(1, n).repeat(N, 1).contiguous()
    agent.use_graph = False
    agent.run_updates(ro, rows_ix[:2].contiguous(), torch.zeros(2, 24, device=dev))
    rows = profiled(lambda: agent.run_updates(ro, rows_ix, torch.zeros(N, 24, device=dev)))
    print("== PPO update with stored log pi_old, %s, B = 1024, f16" % tag)
    print("kernel time per update: %.1f us in %d launches" % (sum(r[2] for r in rows) / N, sum(r[1] for r in rows) // N))
    for label, calls, us in rows:
        if "loss" in label:
            print("%-46s %6.1f %12.2f" % (label, calls / N, us / N))
    # rollout step, E = 32, shared base, eager
    from vision4leg_amd import engine
    E, T = 32, 24
    actor = engine.HipActor(pf.hip, vf.hip, E, shared_encoder=True, graph=False)
    net = pf.hip
    net.ensure_bound()
    state, image = net.alloc_rollout(T * E, dev)
    A = case["A"]
    acts, vals, logp = torch.zeros(T * E, A, device=dev), torch.zeros(T * E, device=dev), torch.zeros(T * E, device=dev)
    actor.attach((state, image, acts, vals, logp))
    actor.seek(0)
    obs = torch.tensor(recipes.obs_rows(np.random.RandomState(3), T * E, case), dtype=torch.float32, device=dev)
    for s in range(4):
        actor.step(obs[s * E:(s + 1) * E])
    rows = profiled(lambda: [actor.step(obs[s * E:(s + 1) * E]) for s in range(4, T)])
    route = actor.route() if hasattr(actor, "route") else "MLP_ONE_BLOCK (parent: no introspection; 16-bit, E <= 64, no tanh)"
    print("== rollout step, %s, E = 32, f16, route %s" % (tag, route))
    print("kernel time per env step: %.2f us in %d launches" % (sum(r[2] for r in rows) / (T - 4), sum(r[1] for r in rows) // (T - 4)))
    for label, calls, us in rows:
        print("%-46s %6.1f %12.2f" % (label, calls / (T - 4), us / (T - 4)))
