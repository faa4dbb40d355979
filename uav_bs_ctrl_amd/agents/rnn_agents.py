"""Recurrent agent of exp2's no-communication arm (o='mlp', c=None) on MI355X.

Interface-compatible with /root/reference/algos/madrqn/agents/rnn_agents.py:6-35 (``RnnAgent(obs_shape, n_actions, args)``,
``init_hidden()``, ``forward(obs, h) -> (q, h')``) and with its ``state_dict``: ``enc.0`` ... (Linear + ReLU stack), ``rnn``
(GRUCell), ``f_out`` (Linear or DuelingLayer), in the reference's ``parameters()`` order.  The reference's learner picks it when
``o == 'mlp' and c is None`` (learner.py:64-67).

``obs`` is either the reference's [N, F] tensor of flattened observations or a ``graph.FlatObsBatch`` built on the device from
the padded observations (``from_padded_obs_flat``), whose first encoder layer reads the padded pieces in place
(csrc/flat_obs.hip).  ``encode`` / ``step`` split the forward like ``GnnAgent``'s, so the learner time-batches the encoder; ``step``
is ``GnnAgent``'s c=None branch (GRU cell + Q head).
"""
from __future__ import annotations

import torch as th
import torch.nn as nn

from ..graph import FlatObsBatch, HeteroBatch
from .gnn_agents import _gru, _head, _unroll, mlp_encode
from .heads import build_head


class RnnAgent(nn.Module):
    """Recurrent policy for independent agents (rnn_agents.py:6-35)."""

    def __init__(self, obs_shape, n_actions, args):
        super().__init__()
        self._n_layers = args.n_layers
        self._hidden_size = args.hidden_size
        layers = [nn.Linear(obs_shape, self._hidden_size), nn.ReLU()]
        for _ in range(self._n_layers - 1):
            layers += [nn.Linear(self._hidden_size, self._hidden_size), nn.ReLU()]
        self.enc = nn.Sequential(*layers)
        self.rnn = nn.GRUCell(self._hidden_size, self._hidden_size)
        self.f_out = build_head(self._hidden_size, n_actions, args)

    def init_hidden(self):
        return th.zeros(1, self._hidden_size)   # on CPU, as the reference does (rnn_agents.py:27-29)

    def encode(self, obs):
        """Observation encoder only: x [N, H] (independent of h: the learner encodes all T+1 steps in one call)."""
        if isinstance(obs, HeteroBatch) and not isinstance(obs, FlatObsBatch):
            obs = obs.agent_feat()
        return mlp_encode(self.enc, obs)

    def step(self, g, x, h, dx_out=None):
        """GRU cell + Q head on pre-encoded observations x (GnnAgent.step's c=None branch)."""
        n = x.shape[0]
        if h.shape[0] != n:
            h = h.expand(n, -1)
        h = _gru(self.rnn, (x,), h.contiguous())
        return _head(self.f_out, h), h

    def unroll(self, x_all, h0, T1):
        """q_all [T1, N, n_actions] from the pre-encoded observations of T1 time-major steps (GnnAgent.unroll)."""
        return _unroll(self.rnn, self.f_out, x_all, h0, T1)

    def forward(self, obs, h):
        return self.step(obs, self.encode(obs), h)
