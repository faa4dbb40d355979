"""Q heads of the agent.

``DuelingLayer`` keeps the reference's parameter layout (``adv_head``, ``v_head``; algos/madrqn/agents/dueling.py:4-16)
so checkpoints interchange: q = V + (A - mean_a A).  On CUDA fp32 with H in {64, 128, 256} and at most 15 actions both heads
and the combine are ONE launch of csrc/head.hip on the live parameters (``ops.dueling_head``); everywhere else - CPU, float64,
other shapes, ``ops.DUEL_FUSED = False`` - ONE GEMM over the stacked [n_actions + 1, H] weight and the combine in torch.
"""
import torch as th
import torch.nn as nn

from .. import ops


class DuelingLayer(nn.Module):
    def __init__(self, in_feats, n_actions):
        super().__init__()
        self.n_actions = n_actions
        self.adv_head = nn.Linear(in_feats, n_actions)
        self.v_head = nn.Linear(in_feats, 1)

    def forward(self, x):
        if x.dim() == 2 and ops.dueling_supported(x, *ops.dueling_params(self)):
            return ops.dueling_head(x, self)
        return self.forward_torch(x)

    def forward_torch(self, x):
        w = th.cat((self.adv_head.weight, self.v_head.weight), 0)
        b = th.cat((self.adv_head.bias, self.v_head.bias), 0)
        out = ops.linear(x, w, b)                                  # [N, A + 1]: advantages | state value
        adv, val = out[:, :self.n_actions], out[:, self.n_actions:]
        return val + adv - adv.mean(-1, keepdim=True)
