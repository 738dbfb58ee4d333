"""A2C with the reference's constructor, attributes and epoch protocol (torchrl/algo/on_policy/a2c.py:8-114 on top of
on_rl_algo.py:11-48, rl_algo.py:19-168), on the PPO shell of this package.

What differs is the update (a2c.py:46-107): no ratio, no target policy, an MSE critic and ONE pass over the epoch's samples
(on_rl_algo.py:36-41), with no learning-rate schedule. Two single-block launches of its own (a2c_critic_loss_kernel,
a2c_loss_kernel) sit between PPO's opening launch, forwards, backwards and clip + Adam launches (max_grad_norm 0.5, a2c.py:81,86).
How a run of updates is launched and read back: second_record.py.

State-MLP nets (networks.Net pairs, the `ppo_state.py` workload) only. The reference's A2C evaluates vf(obs) before
pf_optimizer.step() and backpropagates vf_loss after it (a2c.py:76-85): with a parameter common to pf and vf torch raises
"one of the variables needed for gradient computation has been modified by an inplace operation", and every vision starter hands
one encoder object to both nets — so the reference's A2C runs networks.Net pairs and nothing else the starters build. With
disjoint parameter sets the two optimiser steps are independent and the update keeps the PPO update's critic-first launch order.

Not supported, refused at construction: any other net kind, pf and vf with a common parameter, and what second_record.py refuses.
"""
import torch.optim as optim

from .second_record import _SecondRecordPPO
from .... import _lib


def _is_state_mlp(net):
    cfg = getattr(net, "_net_cfg", None)
    return cfg is not None and cfg().kind == _lib.V4L_NET_MLP  # (host only: no engine handle is made)


class A2C(_SecondRecordPPO):
    _second_stats = _lib.V4L_A2C_STATS
    _rollout_keys = ("acts", "advs", "estimate_returns")  # (no stored values, no stored log pi_old: A2C reads neither)
    _passes = 1  # on_rl_algo.py:36-41
    _syncs_target = False
    _run_entry, _next_entry = "a2c_update_run", "a2c_update_next"
    _takes_categorical = True  # policies.CategoricalDisPolicy: a2c_cat_loss_kernel in a2c_loss_kernel's place

    def __init__(self, pf, vf, plr=3e-4, vlr=3e-4, optimizer_class=optim.Adam, entropy_coeff=0.001, shuffle=True, tau=None, gae=True,
                 **kwargs):
        self._refuse(pf, kwargs)
        if not (_is_state_mlp(pf) and _is_state_mlp(vf)):
            raise NotImplementedError("vision4leg_amd: A2C runs state-MLP nets (networks.Net pairs) only: the reference's A2C "
                                      "raises on a shared encoder (vf(obs) is evaluated before pf_optimizer.step() and "
                                      "backpropagated after it, a2c.py:76-85), and every vision starter shares one")
        if {id(p) for p in pf.parameters()} & {id(p) for p in vf.parameters()}:
            raise NotImplementedError("vision4leg_amd: A2C needs pf and vf without a common parameter: the reference's A2C raises "
                                      "on shared parameters (an in-place optimiser step between vf(obs) and vf_loss.backward())")
        for k in ("clip_para", "opt_epochs", "clipped_value_loss"):  # PPO's, not A2C's (a2c.py:13-20)
            if k in kwargs:
                raise TypeError("A2C.__init__() got an unexpected keyword argument %r" % k)
        # clip_para is never read by an A2C launch; one pass over the samples (on_rl_algo.py:36-41)
        super().__init__(pf, vf, plr=plr, vlr=vlr, optimizer_class=optimizer_class, entropy_coeff=entropy_coeff, clip_para=0.0,
                         opt_epochs=1, clipped_value_loss=False, shuffle=shuffle, tau=tau, gae=gae, **kwargs)
        # the trainer's third net handle is never run by an A2C update: kept private, no `target_pf` on the surface
        self._target_pf = self.__dict__.pop("target_pf")
        for k in ("clip_para", "opt_epochs", "clipped_value_loss"):
            self.__dict__.pop(k)
        self.sample_key = ["obs", "acts", "advs", "estimate_returns"]  # on_rl_algo.py:18

    @property
    def networks(self):
        return [self.pf, self.vf]  # on_rl_algo.py:43-48

    def to(self, device):
        hidden = self.__dict__.get("target_pf", self.__dict__.get("_target_pf"))
        for net in self.networks + ([hidden] if hidden is not None else []):
            net.to(device)

    def _info(self, row, arow):
        """The logger's info dict of one update: the reference's 12 keys in its order (a2c.py:89-105), the A2C record's first —
        8 for a categorical policy: the reference logs std/* only `if 'std' in out` (a2c.py:63-65,97-102)."""
        info = {k: float(arow[j]) for j, k in enumerate(_lib.A2C_INFO_KEYS)}
        if getattr(getattr(self, "pf", None), "categorical_head", False):
            info = {k: info[k] for k in _lib.A2C_CAT_INFO_KEYS}
        return info
