"""V-MPO with the reference's constructor, attributes and epoch protocol (torchrl/algo/on_policy/v_mpo.py:11-192 on top of
a2c.py:13-44, on_rl_algo.py:11-34, rl_algo.py:19-168), on the PPO shell of this package.

What differs is the actor stage of a minibatch update (v_mpo.py:58-134): the better half of the minibatch by normalised
advantage is chosen on the device (vmpo_select_kernel), the live and the frozen target policy run on those rows, and one
single-block launch (vmpo_loss_kernel) forms the softmax-weighted log-prob + alpha KL loss, its gradients, the statistics and
the Adam step of the two learnable scalars eta and alpha. The critic step, the clip + Adam launches and the advantage statistics
are PPO's with clipped_value_loss=False. How a run of updates is launched and read back, and what is refused at construction
(the reference's snapshot holds neither eta nor alpha; snapshot() keeps writing the reference's files): second_record.py.
"""
import torch

from .second_record import _SecondRecordPPO
from .... import _lib


class _ScalarAdam:
    """`param_optimizer` of the reference (v_mpo.py:35-39): `optimizer_class([eta, alpha], lr=plr, eps=1e-5)`. Its state lives in
    the trainer's V-MPO device block and its step is taken inside the loss launch, at the policy optimiser's learning rate (the
    reference runs both at plr: V-MPO has no schedule). This object reports the group's values."""

    def __init__(self, plr, eps, betas, weight_decay, decoupled):
        self.param_groups = [{"params": ["eta", "alpha"], "lr": plr, "eps": eps, "betas": betas, "weight_decay": weight_decay,
                              "decoupled_weight_decay": bool(decoupled)}]

    def zero_grad(self):
        pass


class VMPO(_SecondRecordPPO):
    _second_stats = _lib.V4L_VMPO_STATS
    _rollout_keys = ("acts", "advs", "estimate_returns", "values")  # (no stored log pi_old: the KL needs the target's mean)
    _passes = property(lambda self: self.opt_epochs)
    _syncs_target = True
    _run_entry, _next_entry = "vmpo_update_run", "vmpo_update_next"

    def __init__(self, pf, vf, opt_epochs=10, eta_eps=0.02, alpha_eps=0.1, clipped_value_loss=False, **kwargs):
        self._refuse(pf, kwargs)
        # the critic step is plain MSE whatever clipped_value_loss says (v_mpo.py:136-155): stored, ignored, as in the reference
        super().__init__(pf, vf, opt_epochs=opt_epochs, clipped_value_loss=False, **kwargs)
        self.clipped_value_loss = clipped_value_loss
        self.eta_eps, self.alpha_eps = eta_eps, alpha_eps
        g = self.pf_optimizer.param_groups[0]
        self.param_optimizer = _ScalarAdam(self.plr, g["eps"], g["betas"], g["weight_decay"], g["decoupled_weight_decay"])
        with torch.cuda.device(self.device):
            self.trainer.vmpo_init(eta_eps, alpha_eps, eta0=1.0, alpha0=0.1)  # v_mpo.py:28,32

    # ---- the two learnable scalars, read from the device (one synchronise each)
    def _scalar(self, i):
        with torch.cuda.device(self.device):
            return torch.tensor([self.trainer.vmpo_state()[i]], dtype=torch.float32, device=self.device)

    @property
    def eta(self):
        return self._scalar(0)

    @property
    def alpha(self):
        return self._scalar(1)

    def _info(self, row, vrow):
        """The logger's info dict of one update: the reference's 19 keys (v_mpo.py:119-134, 154-155, 173-176)."""
        both = {k: float(row[j]) for j, k in enumerate(_lib.STAT_KEYS)}
        both.update({k: float(vrow[j]) for j, k in enumerate(_lib.VMPO_STAT_KEYS)})
        return {k: both[k] for k in _lib.VMPO_INFO_KEYS}
