"""Generates tests/golden/ppo_sd_mlp.npz and ppo_sd_mlp_tanh.npz by running the UNMODIFIED reference's PPO
(torchrl/algo/on_policy/ppo.py) with its GaussianContPolicy (torchrl/policies/continuous_policy.py:222-236) on CPU: the policy's
forward and two PPO.update calls on recipes.make_batch for the two fixture cases of tests/sd_cases.py, the way
make_golden_a2c.py does for A2C; and pins tests/sd_cases.SDOracle against it. Run: `python tests/golden/make_golden_sd.py`.

The fixtures hold the reference's forward on the first minibatch (`fwd_mean`, `fwd_std`, `fwd_log_std`: [B, A]), and per update
the 18 infos (`u<k>/info`, order util.STAT_KEYS), every small parameter in full (`u<k>/<pf|vf>/<name>`,
util.small_param_names) and a checksum of every parameter (`u<k>/sum/<pf|vf>/<name>`: sum and sum of magnitudes, in double);
`seed` is the case's construction seed and `batch_seeds` the two minibatches' (recipes.make_batch). Reference outputs only."""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (puts the repository root and tests/ on sys.path)
import util  # noqa: E402
import sd_cases as sc  # noqa: E402


def run_reference(RefPPO, Box, networks, policies, case):
    pf, vf = sc.seeded_nets(networks, policies, case)
    assert type(pf).__name__ == "GaussianContPolicy" and "logstd" not in pf.state_dict()

    class Env: action_space = Box()
    class Coll: epoch_frames = 1
    class Log:
        def add_update_info(self, info): pass
    init = ({k: v.clone() for k, v in pf.state_dict().items()}, {k: v.clone() for k, v in vf.state_dict().items()})
    obs = torch.tensor(util.make_batch(case)["obs"], dtype=torch.float32)
    with torch.no_grad():
        fwd = tuple(t.clone() for t in pf(obs))
    agent = RefPPO(pf=pf, vf=vf, plr=sc.LR, vlr=sc.LR, clip_para=sc.CLIP_PARA, opt_epochs=3, tau=0.95, shuffle=True,
                   entropy_coeff=sc.ENTROPY_COEFF, env=Env(), replay_buffer=None, collector=Coll(), logger=Log(),
                   device=torch.device("cpu"), discount=0.99, num_epochs=1500, batch_size=case["B"], save_interval=100,
                   eval_interval=10, save_dir=tempfile.mkdtemp())
    out = []
    for u in range(2):
        info = agent.update(sc.host_batch(case, u))
        params = {"pf": {k: v.clone() for k, v in pf.state_dict().items()}, "vf": {k: v.clone() for k, v in vf.state_dict().items()}}
        out.append((info, params))
    return init, fwd, out


def main():
    networks, policies, RefPPO, _, Box = mg.import_reference()
    torch.set_num_threads(8)
    for name in sc.FIXTURE_CASES:
        case = sc.SD_CASES[name]
        print("==", name, case)
        init, fwd, runs = run_reference(RefPPO, Box, networks, policies, case)
        oracle = sc.fresh_oracle(case, init=init)
        small = util.small_param_names(*init)
        out = {"seed": np.int64(case["seed"]), "batch_seeds": np.array([1000 * case["seed"] + 17 + u for u in range(2)]),
               "fwd_mean": fwd[0].numpy(), "fwd_std": fwd[1].numpy(), "fwd_log_std": fwd[2].numpy()}
        assert fwd[2].shape == (case["B"], case["A"])
        with torch.no_grad():
            om, ostd, ols, _ = oracle.policy(oracle.pf, torch.tensor(util.make_batch(case)["obs"], dtype=torch.float32))
        assert util.rel_err(om, fwd[0]) < 2e-5 and util.rel_err(ostd, fwd[1]) < 2e-5 and (ols - fwd[2]).abs().max() < 2e-6
        for u, (info, params) in enumerate(runs):
            assert list(info) == util.STAT_KEYS, list(info)
            oinfo = oracle.update(*sc.batch_tensors(case, u), sc.LR, sc.LR)
            out["u%d/info" % u] = np.array([info[k] for k in util.STAT_KEYS])
            for k in util.STAT_KEYS:
                assert abs(info[k] - oinfo[k]) <= 1e-5 * max(1.0, abs(info[k])), (u, k, info[k], oinfo[k])
            worst = 0.0
            for tag, onet in (("pf", oracle.pf), ("vf", oracle.vf)):
                for k, v in params[tag].items():
                    d = v.double()
                    out["u%d/sum/%s/%s" % (u, tag, k)] = np.array([d.sum().item(), d.abs().sum().item()])
                    if (tag, k) in small:
                        out["u%d/%s/%s" % (u, tag, k)] = v.numpy().copy()
                    worst = max(worst, (onet[k] - v).abs().max().item())
            assert worst <= 1e-6, worst
            print("   update %d: policy_loss %.6f vf_loss %.6f log_std/mean %.6f log_std/std %.6f ratio/max %.6f; restatement: "
                  "worst parameter %.1e" % (u, info["Training/policy_loss"], info["Training/vf_loss"], info["log_std/mean"],
                                            info["log_std/std"], info["ratio/max"], worst))
        path = os.path.join(HERE, "ppo_%s.npz" % name)
        np.savez_compressed(path, **out)
        print("   wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
