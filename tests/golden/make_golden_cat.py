"""Generates tests/golden/a2c_cat_mlp.npz and rf_cat_mlp.npz by running the UNMODIFIED reference on CPU: its A2C
(torchrl/algo/on_policy/a2c.py) and its Reinforce (torchrl/algo/on_policy/reinforce.py) with its own
policies.CategoricalDisPolicy (torchrl/policies/discrete_policies.py:127-172), two update calls each on cat_cases.host_batch for
the fixture case of tests/cat_cases.py, the way make_golden_a2c.py / make_golden_reinforce.py do for the Gaussian policy; and
pins tests/cat_cases.CatOracle / CatReinforceOracle and this package's seeded parameter construction against it.
Run: `python tests/golden/make_golden_cat.py`.

The fixtures hold the keys of those two scripts: per update the infos (`u<k>/info`: 8 of A2C's in the order of
cat_cases.A2C_INFO_KEYS — the reference logs std/* only `if 'std' in out` —, Reinforce's 10), every small parameter in full
(`u<k>/<pf|vf>/<name>`) and a checksum of every parameter (`u<k>/sum/<pf|vf>/<name>`: sum and sum of magnitudes, in double);
`seed` and, for A2C, `batch_seeds`. Reference outputs only."""
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
import cat_cases as cc  # noqa: E402
import reinforce_cases as rc  # noqa: E402


def _agent(cls, Box, case, **nets):
    class Env: action_space = Box()
    class Coll: epoch_frames = 1
    class Log:
        def add_update_info(self, info): pass
    return cls(plr=cc.LR, tau=0.95, shuffle=True, entropy_coeff=cc.ENTROPY_COEFF, env=Env(), replay_buffer=None, collector=Coll(),
               logger=Log(), device=torch.device("cpu"), discount=0.99, num_epochs=1500, batch_size=case["B"], save_interval=100,
               eval_interval=10, save_dir=tempfile.mkdtemp(), **nets)


def _clone(net):
    return {k: v.clone() for k, v in net.state_dict().items()}


def run_a2c(RefA2C, Box, networks, policies, case):
    pf, vf = cc.seeded_nets(networks, policies, case)
    agent = _agent(RefA2C, Box, case, pf=pf, vf=vf, vlr=cc.LR)
    init = (_clone(pf), _clone(vf))
    out = []
    for u in range(2):
        info = agent.update(cc.host_batch(case, u))
        out.append((info, {"pf": _clone(pf), "vf": _clone(vf)}))
    return init, out


def run_reinforce(RefReinforce, Box, networks, policies, case):
    pf = cc.seeded_policy(networks, policies, case)
    agent = _agent(RefReinforce, Box, case, pf=pf)
    assert agent.gae is False and agent.pf_optimizer.param_groups[0]["eps"] == rc.ADAM_EPS
    init = _clone(pf)
    out = []
    for u in range(2):
        info = agent.update(cc.host_batch(case, u))
        out.append((info, {"pf": _clone(pf)}))
    return init, out


def write(name, case, keys, runs, oracle, step, small, extra):
    out = dict(extra, seed=np.int64(case["seed"]))
    nets = [("pf", oracle.pf)] + ([("vf", oracle.vf)] if oracle.vf else [])
    for u, (info, params) in enumerate(runs):
        assert list(info) == keys, list(info)
        oinfo = step(u)
        out["u%d/info" % u] = np.array([info[k] for k in keys])
        for k in keys:
            assert abs(info[k] - oinfo[k]) <= 1e-5 * max(1.0, abs(info[k])), (u, k, info[k], oinfo[k])
        worst = 0.0
        for tag, onet in nets:
            for k, v in params[tag].items():
                d = v.double()
                out["u%d/sum/%s/%s" % (u, tag, k)] = np.array([d.sum().item(), d.abs().sum().item()])
                if (tag, k) in small:
                    out["u%d/%s/%s" % (u, tag, k)] = v.numpy().copy()
                worst = max(worst, (onet[k] - v).abs().max().item())
        assert worst <= 1e-6, worst
        print("   update %d: policy_loss %.6f ent %.6f; restatement: worst parameter %.1e"
              % (u, info["Training/policy_loss"], info["ent"], worst))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print("   wrote %s (%d bytes)" % (path, os.path.getsize(path)))


def main():
    networks, policies, _, _, Box = mg.import_reference()
    sys.path.insert(0, mg.REF)
    from torchrl.algo.on_policy.a2c import A2C as RefA2C
    from torchrl.algo.on_policy.reinforce import Reinforce as RefReinforce
    sys.path.remove(mg.REF)
    import vision4leg_amd.torchrl.networks as my_networks
    import vision4leg_amd.torchrl.policies as my_policies
    torch.set_num_threads(8)
    case = cc.CAT_CASES[cc.FIXTURE_CASE]
    assert policies.CategoricalDisPolicy.__module__.startswith("torchrl.policies")

    print("== A2C", cc.FIXTURES["a2c"], case)
    init, runs = run_a2c(RefA2C, Box, networks, policies, case)
    mine = cc.seeded_nets(my_networks, my_policies, case)  # this package's seeded construction: the reference's bits
    for ref_sd, net in zip(init, mine):
        sd = net.state_dict()
        assert list(sd) == list(ref_sd) and all(torch.equal(sd[k], ref_sd[k]) for k in sd)
    oracle = cc.fresh_a2c_oracle(case, init=init)
    write(cc.FIXTURES["a2c"], case, cc.A2C_INFO_KEYS, runs, oracle,
          lambda u: oracle.update(*cc.batch_tensors(case, u), cc.LR, cc.LR), util.small_param_names(*init),
          {"batch_seeds": np.array([1000 * case["seed"] + 17 + u for u in range(2)])})

    print("== Reinforce", cc.FIXTURES["rf"], case)
    init, runs = run_reinforce(RefReinforce, Box, networks, policies, case)
    sd = cc.seeded_policy(my_networks, my_policies, case).state_dict()
    assert list(sd) == list(init) and all(torch.equal(sd[k], init[k]) for k in sd)
    roracle = cc.fresh_rf_oracle(case, init=init)
    write(cc.FIXTURES["rf"], case, cc.RF_INFO_KEYS, runs, roracle,
          lambda u: roracle.update(*cc.batch_tensors(case, u), cc.LR), util.small_param_names(init, {}), {})


if __name__ == "__main__":
    main()
