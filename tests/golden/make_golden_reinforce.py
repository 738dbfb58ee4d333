"""Generates tests/golden/rf_mlp.npz and rf_loco.npz by running the UNMODIFIED reference's Reinforce
(torchrl/algo/on_policy/reinforce.py) on CPU: two Reinforce.update calls on util.make_batch for the two fixture cases of
tests/reinforce_cases.py, the way make_golden_vmpo.py does for V-MPO; and pins tests/reinforce_cases.ReinforceOracle against it.
Run: `python tests/golden/make_golden_reinforce.py`.

Per update the fixtures hold the 10 infos (`u<k>/info`, order reinforce_cases.INFO_KEYS), every small parameter in full
(`u<k>/pf/<name>`, util.small_param_names) and a checksum of every parameter (`u<k>/sum/pf/<name>`: sum and sum of magnitudes,
in double), and the case's seed. Reference outputs only."""
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
import reinforce_cases as rc  # noqa: E402


def run_reference(RefReinforce, Box, networks, policies, case):
    pf = rc.seeded_policy(networks, policies, case)

    class Env: action_space = Box()
    class Coll: epoch_frames = 1
    class Log:
        def add_update_info(self, info): pass
    agent = RefReinforce(pf=pf, plr=rc.LR, tau=0.95, shuffle=True, entropy_coeff=rc.ENTROPY_COEFF, env=Env(),
                         replay_buffer=None, collector=Coll(), logger=Log(), device=torch.device("cpu"), discount=0.99,
                         num_epochs=1500, batch_size=case["B"], save_interval=100, eval_interval=10, save_dir=tempfile.mkdtemp())
    assert agent.gae is False and agent.pf_optimizer.param_groups[0]["eps"] == rc.ADAM_EPS
    init = {k: v.clone() for k, v in pf.state_dict().items()}
    out = []
    for u in range(2):
        b = util.make_batch(case, update=u)
        info = agent.update({k: b[k] for k in rc.BATCH_KEYS})
        out.append((info, {k: v.clone() for k, v in pf.state_dict().items()}))
    return init, out


def main():
    networks, policies, _, _, Box = mg.import_reference()
    sys.path.insert(0, mg.REF)
    from torchrl.algo.on_policy.reinforce import Reinforce as RefReinforce
    sys.path.remove(mg.REF)
    torch.set_num_threads(8)
    for name in rc.FIXTURE_CASES:
        case = rc.REINFORCE_CASES[name]
        print("==", name, case)
        init, runs = run_reference(RefReinforce, Box, networks, policies, case)
        oracle = rc.fresh_oracle(case, init=init)
        small = util.small_param_names(init, {})
        out = {"seed": np.int64(case["seed"])}
        for u, (info, params) in enumerate(runs):
            assert list(info) == rc.INFO_KEYS, list(info)
            oinfo = oracle.update(*rc.batch_tensors(case, u), rc.LR)
            out["u%d/info" % u] = np.array([info[k] for k in rc.INFO_KEYS])
            for k in rc.INFO_KEYS:
                assert abs(info[k] - oinfo[k]) <= 1e-5 * max(1.0, abs(info[k])), (u, k, info[k], oinfo[k])
            worst = 0.0
            for k, v in params.items():
                d = v.double()
                out["u%d/sum/pf/%s" % (u, k)] = np.array([d.sum().item(), d.abs().sum().item()])
                if ("pf", k) in small:
                    out["u%d/pf/%s" % (u, k)] = v.numpy().copy()
                worst = max(worst, (oracle.pf[k] - v).abs().max().item())
            assert worst <= 1e-6, worst
            print("   update %d: policy_loss %.6f ent %.6f logprob/mean %.4f std %.4f; restatement: worst parameter %.1e"
                  % (u, info["Training/policy_loss"], info["ent"], info["logprob/mean"], info["logprob/std"], worst))
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **out)
        print("   wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
