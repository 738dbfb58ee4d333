"""Generates tests/golden/ppo_optim_{mlp_s93,loco_s84}_{decoupled,coupled}.npz by running the UNMODIFIED reference's PPO on CPU
with optimizer_class=functools.partial(torch.optim.AdamW, weight_decay=W) and functools.partial(torch.optim.Adam, weight_decay=W)
(tests/optim_cases.GOLDEN_WD), two PPO.update calls each, the way make_golden_tact.py does for its case; and pins the restatement
of tests/optim_cases.py (adam_step, put in oracle.ppo_oracle.adam_step's place) against it. Run:
`python tests/golden/make_golden_optim.py`.

The fixtures hold what make_golden.py's hold for an update (18 infos, fingerprints and leading elements of every parameter's
change, every small tensor in full, the clipped gradients' fingerprints), plus the setting (weight_decay, decoupled, lr) and how
far the decay moved the parameters. Reference outputs only.

Which W, and why the learning rate stays 1e-4. tests/test_gpu_parity.py::test_ppo_update's parameter rules are sized for
lr = 1e-4: every element within 2.2e-4 (u + 1) of the oracle in the 16-bit modes (an element whose gradient changes sign inside
the 16-bit envelope moves by 2 lr per update), the mean within 2e-5 (u + 1); 2e-5 and 1e-7 in f32. The GPU test uses those rules
unchanged, so it runs at lr = 1e-4, and the decay has to show at that rate:
  decoupled  an element moves by lr W |p| per step. W = 100 (the factor 1 - lr W = 0.99): after two updates the largest move
             is asserted >= 10 x the 16-bit element gate of the second update (4.4e-4) and the mean move >= 10 x the 16-bit mean
             gate (4e-5). torch's default W = 0.01 would move an element by 1e-6 |p|: below every gate.
  coupled    Adam normalises the step, so L2 decay cannot move an element by more than 2 lr per step whatever W is (a step of
             +lr turned into -lr): it turns the step's direction towards -sign(p) where W |p| outweighs the clipped gradient.
             W = 1 does that for most elements. After two updates the MEAN move is asserted >= 5 x the 16-bit mean gate (4e-5)
             and the largest move >= 1.5 x the 16-bit element gate (its ceiling is 4 lr = 8e-4 = 1.8 x) and so >= 30 x the f32
             element gate (2e-5): in the 16-bit modes it is above all the mean rule that a decay-free kernel fails.
Both are asserted below against a run of the same seed without decay, and the measured moves are written into the fixture
(`decay_moved`: largest and mean |p_decay - p_plain| after each update) and printed. Measured, after two updates:
  mlp_s93   decoupled  largest 4.14e-2 (94 x 4.4e-4) / mean 8.75e-4 (22 x 4e-5)    coupled  largest 7.61e-4 (1.7 x) / mean 2.80e-4 (7 x)
  loco_s84  decoupled  largest 4.14e-2 (94 x)        / mean 1.25e-3 (31 x)         coupled  largest 7.91e-4 (1.8 x) / mean 2.94e-4 (7 x)
"""
import functools
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
import optim_cases as oc  # noqa: E402

GATE16_ELEM, GATE16_MEAN, GATE32_ELEM = 4.4e-4, 4e-5, 2e-5   # test_ppo_update's rules at the second update


def run_reference(RefPPO, Box, networks, policies, case, optimizer_class):
    """Two reference PPO.update calls -> per update (info, {tag: state_dict copy}, {tag: {name: clipped grad}})."""
    pf, vf = mg.build_ref_nets(networks, policies, case)

    class Env: action_space = Box()
    class Coll: epoch_frames = 1
    class Log:
        def add_update_info(self, info): pass
    kw = {} if optimizer_class is None else {"optimizer_class": optimizer_class}
    agent = RefPPO(pf=pf, vf=vf, plr=oc.GOLDEN_LR, vlr=oc.GOLDEN_LR, clip_para=0.2, opt_epochs=3, tau=0.95, shuffle=True,
                   entropy_coeff=0.005, env=Env(), replay_buffer=None, collector=Coll(), logger=Log(),
                   device=torch.device("cpu"), discount=0.99, num_epochs=1500, batch_size=case["B"],
                   save_interval=100, eval_interval=10, save_dir=tempfile.mkdtemp(), **kw)
    init = {"pf": {k: v.clone() for k, v in pf.state_dict().items()}, "vf": {k: v.clone() for k, v in vf.state_dict().items()}}
    out = []
    for u in range(2):
        b = util.make_batch(case, update=u)
        info = agent.update({k: b[k] for k in ("obs", "acts", "advs", "estimate_returns", "values")})
        params = {"pf": {k: v.clone() for k, v in pf.state_dict().items()}, "vf": {k: v.clone() for k, v in vf.state_dict().items()}}
        grads = {tag: {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
                 for tag, net in (("pf", pf), ("vf", vf))}
        out.append((info, params, grads))
    return agent, init, out


def main():
    networks, policies, RefPPO, _, Box = mg.import_reference()
    from oracle import ppo_oracle as orc

    torch.set_num_threads(8)
    plain_step = orc.adam_step
    for name in oc.GOLDEN_CASES:
        case = util.CASES[name]
        _, _, plain = run_reference(RefPPO, Box, networks, policies, case, None)
        for mode_wd in oc.MODES_WD:
            wd, decoupled = oc.GOLDEN_WD[mode_wd], mode_wd == "decoupled"
            print("==", name, mode_wd, "weight_decay", wd)
            cls = functools.partial(torch.optim.AdamW if decoupled else torch.optim.Adam, weight_decay=wd)
            agent, init, runs = run_reference(RefPPO, Box, networks, policies, case, cls)
            g = agent.pf_optimizer.param_groups[0]
            assert type(agent.pf_optimizer) is (torch.optim.AdamW if decoupled else torch.optim.Adam)
            assert g["weight_decay"] == wd and g["decoupled_weight_decay"] == decoupled and g["eps"] == 1e-5
            # the oracle with the restatement in adam_step's place must track the reference as it does without decay
            opf = {k: v.clone() for k, v in init["pf"].items()}
            ovf = util.share_encoder(opf, {k: v.clone() for k, v in init["vf"].items()}, case["kind"])
            orc.adam_step = oc.oracle_adam_step(wd, decoupled)
            try:
                oracle = orc.PPOOracle(case["kind"], opf, ovf, {k: v.clone() for k, v in opf.items()}, case["S"])
                oracle.sync_target()
                out = {"weight_decay": np.float64(wd), "decoupled": np.bool_(decoupled), "lr": np.float64(oc.GOLDEN_LR)}
                small = util.small_param_names(init["pf"], init["vf"])
                t = lambda a: torch.tensor(a, dtype=torch.float32)
                moved = []
                before = init
                for u, (info, params, grads) in enumerate(runs):
                    b = util.make_batch(case, update=u)
                    oinfo = oracle.update(t(b["obs"]), t(b["acts"]), t(b["advs"]), t(b["estimate_returns"]), t(b["values"]),
                                          oc.GOLDEN_LR, oc.GOLDEN_LR)
                    out["u%d/info" % u] = np.array([info[k] for k in util.STAT_KEYS])
                    for k in util.STAT_KEYS:
                        assert abs(info[k] - oinfo[k]) <= 2e-4 * max(1.0, abs(info[k])), (k, info[k], oinfo[k])
                    # the logged norms hold no decay term: the first update's critic norm equals the decay-free run's exactly
                    # (the critic steps first on untouched parameters; the actor's forward already sees the decayed encoder)
                    if u == 0:
                        assert info["grad_norm/vf"] == plain[0][0]["grad_norm/vf"], (info["grad_norm/vf"], plain[0][0]["grad_norm/vf"])
                    big, tot, cnt = 0.0, 0.0, 0
                    for tag, onet in (("pf", opf), ("vf", ovf)):
                        for k, v in params[tag].items():
                            d = (v - before[tag][k]).double()
                            out["u%d/d%s/%s" % (u, tag, k)] = np.concatenate([[d.sum().item(), d.abs().sum().item()], d.flatten()[:32].numpy()])
                            if (tag, k) in small:
                                out["u%d/%s/%s" % (u, tag, k)] = v.numpy().copy()
                            assert torch.allclose(onet[k], v, rtol=0, atol=2e-5), (tag, k, (onet[k] - v).abs().max())
                            dd = (v - plain[u][1][tag][k]).abs()
                            big = max(big, dd.max().item())
                            tot += dd.sum().item(); cnt += dd.numel()
                        for k, gr in grads[tag].items():
                            gr = gr.double()
                            out["u%d/g%s/%s" % (u, tag, k)] = np.concatenate(
                                [[gr.sum().item(), gr.abs().sum().item(), gr.norm().item()], gr.flatten()[:32].numpy()])
                    moved.append((big, tot / cnt))
                    before = params
                    print("   update %d: ratio max %.4f vf_loss %.4f gn_pf %.4f; the decay moved the parameters by %.2e (largest) "
                          "/ %.2e (mean)" % (u, info["ratio/max"], info["Training/vf_loss"], info["grad_norm/pf"], big, tot / cnt))
            finally:
                orc.adam_step = plain_step
            out["decay_moved"] = np.array(moved)
            big, mean = moved[1]
            if decoupled:
                assert big >= 10 * GATE16_ELEM and mean >= 10 * GATE16_MEAN, (big, mean)
            else:
                assert mean >= 5 * GATE16_MEAN and big >= 1.5 * GATE16_ELEM >= 30 * GATE32_ELEM, (big, mean)
            path = os.path.join(HERE, oc.golden_name(name, mode_wd) + ".npz")
            np.savez_compressed(path, **out)
            print("   wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
