"""Generates tests/golden/vmpo_mlp.npz and vmpo_loco.npz by running the UNMODIFIED reference's VMPO
(torchrl/algo/on_policy/v_mpo.py) on CPU: two VMPO.update calls on recipes.make_batch for the two fixture cases of
tests/vmpo_cases.py, the way make_golden_optim.py does for PPO; and pins tests/vmpo_cases.VMPOOracle against it.
Run: `python tests/golden/make_golden_vmpo.py`.

Per update the fixtures hold the 19 infos (`u<k>/info`, order vmpo_cases.INFO_KEYS), eta and alpha (`u<k>/eta`, `u<k>/alpha`),
every small parameter in full (`u<k>/<pf|vf>/<name>`, util.small_param_names) and a checksum of every parameter
(`u<k>/sum/<pf|vf>/<name>`: sum and sum of magnitudes, in double). Reference outputs only."""
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
import vmpo_cases as vc  # noqa: E402


def run_reference(RefVMPO, Box, networks, policies, case):
    pf, vf = mg.build_ref_nets(networks, policies, case)

    class Env: action_space = Box()
    class Coll: epoch_frames = 1
    class Log:
        def add_update_info(self, info): pass
    agent = RefVMPO(pf=pf, vf=vf, plr=vc.LR, vlr=vc.LR, opt_epochs=3, tau=0.95, shuffle=True, entropy_coeff=0.005, env=Env(),
                    replay_buffer=None, collector=Coll(), logger=Log(), device=torch.device("cpu"), discount=0.99,
                    num_epochs=1500, batch_size=case["B"], save_interval=100, eval_interval=10, save_dir=tempfile.mkdtemp())
    init = ({k: v.clone() for k, v in pf.state_dict().items()}, {k: v.clone() for k, v in vf.state_dict().items()})
    import torchrl.algo.utils as atu
    atu.copy_model_params_from_to(agent.pf, agent.target_pf)  # update_per_epoch's sync (v_mpo.py:50)
    out = []
    for u in range(2):
        b = util.make_batch(case, update=u)
        info = agent.update({k: b[k] for k in ("obs", "acts", "advs", "estimate_returns", "values")})
        params = {"pf": {k: v.clone() for k, v in pf.state_dict().items()}, "vf": {k: v.clone() for k, v in vf.state_dict().items()}}
        out.append((info, params, agent.eta.item(), agent.alpha.item()))
    return init, out


def main():
    networks, policies, _, _, Box = mg.import_reference()
    from torchrl.algo.on_policy.v_mpo import VMPO as RefVMPO
    torch.set_num_threads(8)
    for name in vc.FIXTURE_CASES:
        case = vc.VMPO_CASES[name]
        print("==", name, case)
        init, runs = run_reference(RefVMPO, Box, networks, policies, case)
        oracle = vc.fresh_oracle(case, init=init)
        small = util.small_param_names(*init)
        out = {}
        for u, (info, params, eta, alpha) in enumerate(runs):
            assert list(info) == vc.INFO_KEYS, list(info)
            oinfo = oracle.update(*vc.batch_tensors(case, u), vc.LR, vc.LR)
            out["u%d/info" % u] = np.array([info[k] for k in vc.INFO_KEYS])
            out["u%d/eta" % u], out["u%d/alpha" % u] = np.float64(eta), np.float64(alpha)
            for k in vc.INFO_KEYS:
                assert abs(info[k] - oinfo[k]) <= 1e-5 * max(1.0, abs(info[k])), (u, k, info[k], oinfo[k])
            assert abs(eta - oracle.eta.item()) <= 1e-6 and abs(alpha - oracle.alpha.item()) <= 1e-6
            worst = 0.0
            for tag, onet in (("pf", oracle.pf), ("vf", oracle.vf)):
                for k, v in params[tag].items():
                    d = v.double()
                    out["u%d/sum/%s/%s" % (u, tag, k)] = np.array([d.sum().item(), d.abs().sum().item()])
                    if (tag, k) in small:
                        out["u%d/%s/%s" % (u, tag, k)] = v.numpy().copy()
                    worst = max(worst, (onet[k] - v).abs().max().item())
            assert worst <= 1e-6, worst
            print("   update %d: policy_loss %.6f eta %.6f alpha %.6f KL/mean %.3e gn_pf %.4f; restatement: worst parameter %.1e"
                  % (u, info["Training/policy_loss"], eta, alpha, info["KL/mean"], info["grad_norm/pf"], worst))
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **out)
        print("   wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
