from .continuous_policy import *  # noqa: F401,F403
from .discrete_policies import *  # noqa: F401,F403
