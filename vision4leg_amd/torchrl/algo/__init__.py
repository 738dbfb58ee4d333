from .on_policy import A2C, PPO, VMPO, PPODiscrete, Reinforce  # noqa: F401

__all__ = ["A2C", "PPO", "PPODiscrete", "VMPO", "Reinforce"]
