"""Generates tests/golden/ppo_cat_mlp.npz by running the UNMODIFIED reference's PPO (torchrl/algo/on_policy/ppo.py) on CPU with a
discrete policy: two PPO.update calls (no target sync in between) on ppo_cat_cases.host_batch for the fixture case of
tests/ppo_cat_cases.py, the way make_golden_sd.py does for GaussianContPolicy; and pins tests/ppo_cat_cases.CatPPOOracle and this
package's seeded parameter construction against it. Run: `python tests/golden/make_golden_ppo_cat.py`.

The reference's PPO cannot run its own CategoricalDisPolicy as it stands: update_actor reads out['log_std'] (ppo.py:53), which
discrete_policies.py:160-172 does not return. The policy here is a subclass of the reference's class, defined below, whose
`update` adds that one key — a constant, zeros of shape [n, 1] — to the dict the reference's method returns; nothing else of the
reference is touched, and the four log_std/* infos it then logs (all 0, std NaN-free: 0) are dropped from the fixture.

The fixture has a2c_cat_mlp.npz's format: per update the infos (`u<k>/info`: the 14 keys of ppo_cat_cases.INFO_KEYS), every small
parameter in full (`u<k>/<pf|vf>/<name>`) and a checksum of every parameter (`u<k>/sum/<pf|vf>/<name>`: sum and sum of
magnitudes, in double); `seed` and `batch_seeds`. Reference outputs only."""
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
import ppo_cat_cases as pc  # noqa: E402


def with_log_std(policies):
    """The reference's policies module with CategoricalDisPolicy replaced by a subclass whose update() also returns
    'log_std': zeros [n, 1] (the one key ppo.py:53 misses). build_nets reads the class from the module it is handed."""
    class CategoricalDisPolicyLogStd(policies.CategoricalDisPolicy):
        def update(self, obs, actions):
            out = super().update(obs, actions)
            out["log_std"] = torch.zeros(obs.shape[0], 1)
            return out

    class Module:
        CategoricalDisPolicy = CategoricalDisPolicyLogStd
    return Module


def run_reference(RefPPO, Box, networks, policies, case):
    pf, vf = pc.seeded_nets(networks, with_log_std(policies), case)
    assert isinstance(pf, policies.CategoricalDisPolicy) and type(pf).__mro__[1].__module__.startswith("torchrl.policies")
    assert (vf.base is pf.base) == case["shared"]

    class Env: action_space = Box()
    class Coll: epoch_frames = 1
    class Log:
        def add_update_info(self, info): pass
    init = ({k: v.clone() for k, v in pf.state_dict().items()}, {k: v.clone() for k, v in vf.state_dict().items()})
    agent = RefPPO(pf=pf, vf=vf, plr=pc.lr_of(case), vlr=pc.lr_of(case), clip_para=pc.CLIP_PARA, opt_epochs=3, tau=0.95,
                   shuffle=True, entropy_coeff=pc.ENTROPY_COEFF, env=Env(), replay_buffer=None, collector=Coll(), logger=Log(),
                   device=torch.device("cpu"), discount=0.99, num_epochs=1500, batch_size=case["B"], save_interval=100,
                   eval_interval=10, save_dir=tempfile.mkdtemp(), clipped_value_loss=bool(case.get("clipped_value_loss", False)))
    out = []
    for u in range(2):
        info = agent.update(pc.host_batch(case, u))
        params = {"pf": {k: v.clone() for k, v in pf.state_dict().items()}, "vf": {k: v.clone() for k, v in vf.state_dict().items()}}
        out.append((info, params))
    return init, out


def main():
    networks, policies, RefPPO, _, Box = mg.import_reference()
    import vision4leg_amd.torchrl.networks as my_networks
    import vision4leg_amd.torchrl.policies as my_policies
    torch.set_num_threads(8)
    name, case = pc.FIXTURE_CASE, pc.PPO_CAT_CASES[pc.FIXTURE_CASE]
    assert pc.updates_of(case) == 2
    print("==", name, case)
    init, runs = run_reference(RefPPO, Box, networks, policies, case)
    mine = pc.seeded_nets(my_networks, my_policies, case)  # this package's seeded construction: the reference's bits
    for ref_sd, net in zip(init, mine):
        sd = net.state_dict()
        assert list(sd) == list(ref_sd) and all(torch.equal(sd[k], ref_sd[k]) for k in sd)
    oracle = pc.fresh_oracle(case, init=init)
    small = util.small_param_names(*init)
    out = {"seed": np.int64(case["seed"]), "batch_seeds": np.array([1000 * case["seed"] + 17 + u for u in range(2)])}
    for u, (info, params) in enumerate(runs):
        assert list(info) == util.STAT_KEYS, list(info)
        assert all(info[k] == 0.0 for k in util.STAT_KEYS if k.startswith("log_std/"))  # the constant the subclass added
        oinfo = oracle.update(*pc.batch_tensors(case, u), pc.lr_of(case), pc.lr_of(case))
        assert list(oinfo) == pc.INFO_KEYS
        out["u%d/info" % u] = np.array([info[k] for k in pc.INFO_KEYS])
        for k in pc.INFO_KEYS:
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
        print("   update %d: policy_loss %.6f vf_loss %.6f ratio/max %.6f ratio/min %.6f; restatement: worst parameter %.1e"
              % (u, info["Training/policy_loss"], info["Training/vf_loss"], info["ratio/max"], info["ratio/min"], worst))
    path = os.path.join(HERE, pc.FIXTURE + ".npz")
    np.savez_compressed(path, **out)
    print("   wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
