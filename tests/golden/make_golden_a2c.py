"""Generates tests/golden/a2c_mlp.npz and a2c_mlp_tanh.npz by running the UNMODIFIED reference's A2C
(torchrl/algo/on_policy/a2c.py) on CPU: two A2C.update calls on recipes.make_batch for the two fixture cases of
tests/a2c_cases.py, the way make_golden_vmpo.py does for V-MPO; and pins tests/a2c_cases.A2COracle against it.
Run: `python tests/golden/make_golden_a2c.py`.

Per update the fixtures hold the 12 infos (`u<k>/info`, order a2c_cases.INFO_KEYS), every small parameter in full
(`u<k>/<pf|vf>/<name>`, util.small_param_names) and a checksum of every parameter (`u<k>/sum/<pf|vf>/<name>`: sum and sum of
magnitudes, in double); `seed` is the case's construction seed and `batch_seeds` the two minibatches' (recipes.make_batch).
Reference outputs only."""
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
import a2c_cases as ac  # noqa: E402


def run_reference(RefA2C, Box, networks, policies, case):
    pf, vf = ac.seeded_nets(networks, policies, case)

    class Env: action_space = Box()
    class Coll: epoch_frames = 1
    class Log:
        def add_update_info(self, info): pass
    agent = RefA2C(pf=pf, vf=vf, plr=ac.LR, vlr=ac.LR, tau=0.95, shuffle=True, entropy_coeff=ac.ENTROPY_COEFF, env=Env(),
                   replay_buffer=None, collector=Coll(), logger=Log(), device=torch.device("cpu"), discount=0.99,
                   num_epochs=1500, batch_size=case["B"], save_interval=100, eval_interval=10, save_dir=tempfile.mkdtemp())
    init = ({k: v.clone() for k, v in pf.state_dict().items()}, {k: v.clone() for k, v in vf.state_dict().items()})
    out = []
    for u in range(2):
        info = agent.update(ac.host_batch(case, u))
        params = {"pf": {k: v.clone() for k, v in pf.state_dict().items()}, "vf": {k: v.clone() for k, v in vf.state_dict().items()}}
        out.append((info, params))
    return init, out


def main():
    networks, policies, _, _, Box = mg.import_reference()
    sys.path.insert(0, mg.REF)
    from torchrl.algo.on_policy.a2c import A2C as RefA2C
    sys.path.remove(mg.REF)
    torch.set_num_threads(8)
    for name in ac.FIXTURE_CASES:
        case = ac.A2C_CASES[name]
        print("==", name, case)
        init, runs = run_reference(RefA2C, Box, networks, policies, case)
        oracle = ac.fresh_oracle(case, init=init)
        small = util.small_param_names(*init)
        out = {"seed": np.int64(case["seed"]), "batch_seeds": np.array([1000 * case["seed"] + 17 + u for u in range(2)])}
        for u, (info, params) in enumerate(runs):
            assert list(info) == ac.INFO_KEYS, list(info)
            oinfo = oracle.update(*ac.batch_tensors(case, u), ac.LR, ac.LR)
            out["u%d/info" % u] = np.array([info[k] for k in ac.INFO_KEYS])
            for k in ac.INFO_KEYS:
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
            print("   update %d: policy_loss %.6f vf_loss %.6f ent %.6f log_prob %.6f; restatement: worst parameter %.1e"
                  % (u, info["Training/policy_loss"], info["Training/vf_loss"], info["ent"], info["log_prob"], worst))
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **out)
        print("   wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
