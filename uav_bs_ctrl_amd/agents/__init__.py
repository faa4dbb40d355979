"""Agent registry, mirroring /root/reference/algos/madrqn/agents/__init__.py:1-7 (``'gnn'`` entry) and
/root/reference/algos/drqn/agents/__init__.py (``'drqn_gnn'``); ``'rnn'``: exp2's no-communication arm (madrqn/agents/rnn_agents.py)."""
REGISTRY = {}

from .gnn_agents import DrqnGnnAgent, GnnAgent  # noqa: E402
from .rnn_agents import RnnAgent  # noqa: E402

REGISTRY["gnn"] = GnnAgent
REGISTRY["drqn_gnn"] = DrqnGnnAgent
REGISTRY["rnn"] = RnnAgent
