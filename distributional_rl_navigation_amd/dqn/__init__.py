from .policy import DQNPolicy  # noqa: F401
from .agent import DQNAgent, split_at_target_sync  # noqa: F401
