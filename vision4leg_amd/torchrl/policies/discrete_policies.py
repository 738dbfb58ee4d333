"""The discrete-action policy of the on-policy learners with the reference's name and method protocol
(torchrl/policies/discrete_policies.py:127-172: CategoricalDisPolicy).

A `networks.Net` whose K = output_shape head outputs are logits; `torch.softmax(logits, -1)` feeds
`torch.distributions.Categorical`. No parameter of its own: the state_dict keys are exactly networks.Net's, so checkpoints
cross-load with the reference's class. `forward / explore / eval_act / update` evaluate the trunk and the categorical head
(log-softmax by max-subtraction, entropy, log-prob) with libv4l_hip.so kernels (v4l_cat_head, v4l_cat_sample); only the uniform
draw of `explore` uses torch's generator. Runs under algo.A2C and algo.Reinforce; algo.PPO and algo.VMPO refuse it.
K = 2 .. 16: the logits fill the engine's 16-column head row.
"""
import torch
from torch.distributions import Categorical

from .. import networks
from ...engine import cat_sample

__all__ = ["CategoricalDisPolicy"]


class CategoricalDisPolicy(networks.Net):
    """Discrete policy (reference discrete_policies.py:127-172): `CategoricalDisPolicy(**net_kwargs)`, networks.Net's keywords."""

    categorical_head = True  # read by the net's engine handle -> v4l_net_set_categorical

    def __init__(self, **kwargs):
        width = int(kwargs["output_shape"])
        if width < 2 or width > 16:
            raise NotImplementedError("vision4leg_amd: CategoricalDisPolicy takes 2 <= output_shape <= 16 (the logits of the "
                                      "actions fill the engine's 16-column head row), got %d" % width)
        super().__init__(**kwargs)
        self.continuous = False

    def _dist(self, x, actions=None):
        lead = x.shape[:-1]
        probs, ent, logp = self.hip.categorical_dist(x.reshape(-1, x.shape[-1]), actions)
        return probs.view(*lead, probs.shape[-1]), ent.view(*lead), (logp.view(*lead) if logp is not None else None)

    def forward(self, x):
        """softmax(logits): [..., K] probabilities (discrete_policies.py:136-138)."""
        return self._dist(x)[0]

    def explore(self, x, return_log_probs=False):
        """{"dis": probabilities, "action": int64 [n][, "log_prob": [n]]} (discrete_policies.py:140-154). The action is drawn by
        inverse CDF — the first k whose running sum of probabilities exceeds u — from ONE `torch.rand` per row on the current
        generator of x's device. That is the same distribution as the reference's `Categorical(probs).sample()`, but NOT
        `torch.multinomial`'s random stream: a seeded rollout does not reproduce the reference's action sequence."""
        lead = x.shape[:-1]
        net = self.hip
        st, im, n = net.stage(x.reshape(-1, x.shape[-1]))
        logits = net.forward(st, im, n)  # padded rows in the net's workspace: valid until its next forward
        flat, _, _ = net.cat_head(logits, n)
        u = torch.rand(n, dtype=torch.float32, device=flat.device)
        action = cat_sample(flat, u)
        out = {"dis": flat.view(*lead, flat.shape[-1]), "action": action.view(*lead)}
        if return_log_probs:  # dis.log_prob(action), from the same logits rows
            out["log_prob"] = net.cat_head(logits, n, action)[2].view(*lead)
        return out

    def eval_act(self, x):
        """The argmax action as a numpy array [n] (discrete_policies.py:156-158)."""
        probs, _, _ = self._dist(x)
        flat = probs.reshape(-1, probs.shape[-1])
        return cat_sample(flat, deterministic=True).view(*probs.shape[:-1]).cpu().numpy()

    def update(self, obs, actions):
        """{"dis": Categorical, "log_prob": [n, 1], "ent": [n]} of the action indices `actions` [n] (discrete_policies.py:160-172)."""
        probs, ent, logp = self._dist(obs, actions)
        return {"dis": Categorical(probs=probs), "log_prob": logp.unsqueeze(-1), "ent": ent}
