"""Fixtures that let tests/test_overlay_cpu.py run without the reference tree. Run: `python tests/golden/make_golden_overlay.py`
(needs /root/reference; imports it with the stub modules of tests/ref_stubs.py, like the tests used to).

  tests/golden/collector_ref.npz            two epochs of the reference's VecOnPolicyCollector over util.FakeVecEnv with
                                            util.StandInPolicy / StandInValue (util.run_collector): replay-buffer arrays,
                                            train rewards, the next draw of torch's generator
  tests/golden/ckpt_hip/<case>/ref_fwd.npz  the forward the reference's classes compute from the HIP-written checkpoint files
                                            of that directory (loaded strictly) on the seeded observation batch
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_stubs  # noqa: E402
import util  # noqa: E402

CKPT_CASES = ("loco_s84", "mlp_s93")


def main():
    ref_stubs.install()
    import gym
    numpy_bool = getattr(np, "bool", None)
    np.bool = bool  # collector/base.py:250-251 uses the alias numpy >= 1.24 removed
    import torchrl.networks as networks, torchrl.policies as policies
    from torchrl.collector.on_policy import VecOnPolicyCollector
    from torchrl.replay_buffers.on_policy import OnPolicyReplayBuffer

    def make_collector(vf, pf, env, buf, frames):
        sp = gym.spaces.Box()
        sp.shape = env.action_space.shape
        env.action_space = sp
        return VecOnPolicyCollector(vf, env=env, eval_env=util.FakeVecEnv(env.env_nums, env.S, env.A, img=0), pf=pf,
                                    replay_buffer=buf, device="cpu", train_render=False, epoch_frames=frames,
                                    max_episode_frames=5, eval_episodes=1)

    out = util.run_collector(make_collector, lambda E, n: OnPolicyReplayBuffer(env_nums=E, max_replay_buffer_size=n,
                                                                             time_limit_filter=True))
    assert out["buf/terminals"].sum() > 2
    np.savez_compressed(os.path.join(HERE, "collector_ref.npz"), **out)
    print("== collector_ref.npz:", {k: v.shape for k, v in out.items()})
    if numpy_bool is None:
        del np.bool
    for name in CKPT_CASES:
        case = util.CASES[name]
        d = os.path.join(HERE, "ckpt_hip", name)
        torch.manual_seed(case["seed"] + 300)
        rpf, rvf = util.build_nets(networks, policies, case)
        rvf.load_state_dict(torch.load(os.path.join(d, "model_vf_2.pth"), map_location="cpu"))
        rpf.load_state_dict(torch.load(os.path.join(d, "model_pf_2.pth"), map_location="cpu"))
        obs = torch.tensor(util.make_batch(case, update=5)["obs"], dtype=torch.float32)
        with torch.no_grad():
            mean, _, _ = rpf(obs)
            value = rvf(obs)
        np.savez_compressed(os.path.join(d, "ref_fwd.npz"), fwd_mean=mean.numpy(), fwd_value=value.numpy())
        print("== ckpt_hip/%s/ref_fwd.npz" % name)


if __name__ == "__main__":
    main()
