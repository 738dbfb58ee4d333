from .ppo import PPO  # noqa: F401
from .ppo_discrete import PPODiscrete  # noqa: F401
from .vmpo import VMPO  # noqa: F401
from .a2c import A2C  # noqa: F401
from .reinforce import Reinforce  # noqa: F401
