from .on_policy import PPO, VMPO  # noqa: F401

__all__ = ["PPO", "VMPO"]
