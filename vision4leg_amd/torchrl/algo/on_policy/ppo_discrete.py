"""PPODiscrete: the clipped-surrogate PPO update (torchrl/algo/on_policy/ppo.py:28-153) for policies.CategoricalDisPolicy.

The reference's own PPO cannot run that class — update_actor reads out['log_std'] (ppo.py:53), which
discrete_policies.py:160-172 does not return — so algo.PPO keeps refusing it and the capability is this named extension. What
runs is PPO's update with one launch exchanged: actor_loss_cat_kernel (csrc/elem.h) in actor_loss_kernel's place, on
Categorical(softmax(logits)) — ratio, clip, entropy bonus with ent.mean() — and the record's four log_std/* slots left empty.
log pi_old is the value the rollout step stored (DeviceOnPolicyReplayBuffer) or, from a host batch, the log-softmax of the frozen
target policy's logits at the stored action index. Everything else — critic, clip + Adam, the learning-rate schedule, opt_epochs
passes over the samples, an epoch's updates as ONE hipGraph replay — is PPO's, launch for launch.

Refused at construction: any policy that is not a CategoricalDisPolicy, a critic that is not a state-MLP net, target_kl,
desired_kl, skip_nonfinite_steps, save_train_state / resume, and data parallel.
"""
import os

import torch

from . import ppo as _ppo
from .ppo import PPO
from .... import _lib

# what update() returns and the logger gets: the reference PPO's 18 keys in its order without log_std/* 
INFO_KEYS = [k for k in _lib.STAT_KEYS if not k.startswith("log_std/")]


class PPODiscrete(PPO):
    _takes_categorical = True  # actor_loss_cat_kernel in actor_loss_kernel's place

    def __init__(self, pf, vf, **kwargs):
        # before PPO.__init__, so before anything touches a device
        if not getattr(pf, "categorical_head", False):
            raise NotImplementedError("vision4leg_amd: PPODiscrete takes policies.CategoricalDisPolicy (discrete actions) only: "
                                      "its loss kernel is categorical; a Gaussian policy (%s) runs under algo.PPO"
                                      % type(pf).__name__)
        cfg = getattr(vf, "_net_cfg", None)
        if cfg is None or cfg().kind != _lib.V4L_NET_MLP:  # (host only: no engine handle is made)
            raise NotImplementedError("vision4leg_amd: PPODiscrete runs state-MLP nets (a CategoricalDisPolicy and a networks.Net "
                                      "critic, with or without a common base) only")
        if kwargs.get("target_kl") is not None:
            raise NotImplementedError("vision4leg_amd: PPODiscrete does not take target_kl (the KL early stop reads a Gaussian "
                                      "log pi_old; its categorical sibling is not built)")
        if kwargs.get("desired_kl") is not None:
            raise NotImplementedError("vision4leg_amd: PPODiscrete does not take desired_kl (the KL-adaptive learning rates read a "
                                      "Gaussian log pi_old; their categorical sibling is not built)")
        if kwargs.get("skip_nonfinite_steps"):
            raise NotImplementedError("vision4leg_amd: PPODiscrete does not take skip_nonfinite_steps=True (the guard is verified "
                                      "for PPO's Gaussian update only)")
        if kwargs.get("save_train_state") or kwargs.get("resume") is not None:
            raise NotImplementedError("vision4leg_amd: PPODiscrete does not save or resume a train state (not verified for this "
                                      "learner); snapshot() writes the reference's model files")
        forced = (os.environ.get("V4L_FORCE_DP_PHASES", "0") != "0" and torch.distributed.is_available()
                  and torch.distributed.is_initialized())
        if _ppo._dist_world() > 1 or forced:
            raise NotImplementedError("vision4leg_amd: PPODiscrete runs in a single process (no data-parallel PPODiscrete update: "
                                      "world_size > 1 / V4L_FORCE_DP_PHASES)")
        super().__init__(pf, vf, **kwargs)

    def train_state(self):
        raise NotImplementedError("vision4leg_amd: PPODiscrete has no resumable train state")

    def save_checkpoint(self, prefix, epoch):
        raise NotImplementedError("vision4leg_amd: PPODiscrete has no resumable train state; use snapshot()")

    def load_checkpoint(self, prefix, epoch, restore_rng=True, restore_collector=False):
        raise NotImplementedError("vision4leg_amd: PPODiscrete has no resumable train state")

    def _info(self, row, flags=None, kl=None, adapt=None):
        """The logger's info dict of one update: the reference PPO's keys in its order without the four log_std/* (14 keys)."""
        info = super()._info(row, flags, kl, adapt)
        return {k: info[k] for k in INFO_KEYS}
