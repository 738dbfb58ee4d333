from .ppo import PPO  # noqa: F401
from .vmpo import VMPO  # noqa: F401
