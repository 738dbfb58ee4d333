"""REINFORCE with the reference's constructor, attributes and epoch protocol (torchrl/algo/on_policy/reinforce.py:7-82 on top of
on_rl_algo.py:11-48, rl_algo.py:19-168), on the PPO shell of this package.

The update (reinforce.py:34-76) is the policy's half of an A2C update and nothing else: the opening launch (rows, advantage
statistics and the policy's operand-type weight copies in one launch), the policy's forward, one single-block loss launch of its
own (reinforce_loss_kernel), the policy's backward, clip (max_grad_norm 0.5, reinforce.py:65) + Adam. ONE pass over the epoch's
samples (on_rl_algo.py:36-41), no learning-rate schedule, discounted rewards (`gae = False`, reinforce.py:32), and Adam's eps is
torch's default 1e-8: the reference hands optimizer_class no eps here (reinforce.py:26-29). How a run of updates is launched and
read back: second_record.py. Every net kind PPO takes.

The critic. The reference's `self.vf = ZeroNet()` is "a vacant value network to simplify the code structure"; for the same reason
`vf` here is `networks.zero_critic(pf)`: a critic on pf's trunk whose last layer is zero, so the trainer, the fused rollout step,
the collector's fast path, the return estimate and the truncation bootstrap run unchanged code and see exact zeros. No launch of
an update reads or writes its parameters or its optimiser state, and the critic's Adam step count stays 0. The cost is a value
head the rollout step does not need.

Not supported, refused at construction: what second_record.py refuses, and a collector whose critic is a real one.
"""
import torch.nn as nn
import torch.optim as optim

from .second_record import _SecondRecordPPO
from ... import networks
from .... import _lib


class Reinforce(_SecondRecordPPO):
    _second_stats = _lib.V4L_REINFORCE_STATS
    # (v4l_trainer's argument check asks for the returns array of every rollout; no REINFORCE launch reads it)
    _rollout_keys = ("acts", "advs", "estimate_returns")
    _passes = 1  # on_rl_algo.py:36-41
    _syncs_target = False
    _run_entry, _next_entry = "reinforce_update_run", "reinforce_update_next"
    _call_eps = None  # optimizer_class(params, lr=plr): torch's own eps, 1e-8 (reinforce.py:26-29)
    _takes_categorical = True  # policies.CategoricalDisPolicy: reinforce_cat_loss_kernel in reinforce_loss_kernel's place

    def __init__(self, pf, plr, optimizer_class=optim.Adam, entropy_coeff=0.001, **kwargs):
        self._refuse(pf, kwargs)
        for k in ("vf", "vlr", "clip_para", "opt_epochs", "clipped_value_loss"):  # A2C's / PPO's, not Reinforce's (reinforce.py:12-18)
            if k in kwargs:
                raise TypeError("Reinforce.__init__() got an unexpected keyword argument %r" % k)
        given = getattr(kwargs.get("collector"), "vf", None)
        if given is not None and networks.is_zero_critic(given, pf):
            vf = given  # the net the rollout step already runs (VecOnPolicyCollector made it from a networks.ZeroNet)
        elif isinstance(given, nn.Module) and next(given.parameters(), None) is not None:
            raise ValueError("vision4leg_amd: Reinforce has no critic: hand the collector networks.ZeroNet() (it becomes "
                             "networks.zero_critic(pf)) or networks.zero_critic(pf) itself, not a %s" % type(given).__name__)
        else:
            vf = networks.zero_critic(pf)
        kwargs.pop("gae", None)  # self.gae = False whatever the caller passes (reinforce.py:32)
        # clip_para is never read by a REINFORCE launch; one pass over the samples (on_rl_algo.py:36-41); vlr: the critic's
        # optimiser never steps
        super().__init__(pf, vf, plr=plr, vlr=plr, optimizer_class=optimizer_class, entropy_coeff=entropy_coeff, clip_para=0.0,
                         opt_epochs=1, clipped_value_loss=False, gae=False, **kwargs)
        # what the trainer holds beyond the policy and its optimiser is never run by a REINFORCE update: kept private
        self._target_pf = self.__dict__.pop("target_pf")
        self._vf_optimizer = self.__dict__.pop("vf_optimizer")
        for k in ("vlr", "clip_para", "opt_epochs", "clipped_value_loss"):
            self.__dict__.pop(k)
        self.sample_key = ["obs", "acts", "advs", "estimate_returns"]  # on_rl_algo.py:18

    @property
    def networks(self):
        return [self.pf, self.vf]  # on_rl_algo.py:43-48

    @property
    def snapshot_networks(self):
        return [("pf", self.pf)]  # reinforce.py:78-82

    def to(self, device):
        hidden = self.__dict__.get("target_pf", self.__dict__.get("_target_pf"))
        for net in self.networks + ([hidden] if hidden is not None else []):
            net.to(device)

    def _lr_vf(self):
        return self._vf_optimizer.lr  # (handed to the opening launch; no launch of an update steps with it)

    def _info(self, row, rrow):
        """The logger's info dict of one update: the reference's 10 keys in its order (reinforce.py:43-74), the REINFORCE record's first."""
        return {k: float(rrow[j]) for j, k in enumerate(_lib.REINFORCE_INFO_KEYS)}
