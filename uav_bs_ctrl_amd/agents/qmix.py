"""QMIX monotonic mixing network (reference: algos/madrqn/agents/mixers.py:6-49).

Not graph work.  Parameter names/shapes follow the reference (``hyper_w_1``, ``hyper_w_final``, ``hyper_b_1``, ``V``)
so checkpoints interchange; the arithmetic is reorganised for the GPU: the four state-conditioned projections share
their input, so they run as ONE GEMM over the stacked weight, and the per-sample 1 x n and 1 x embed products become
broadcast multiply-reduces over [T*B, n, embed] (a ``bmm`` per sample would be pure launch overhead at n <= 16).

On CUDA float32 tensors (n <= 16, embed <= 128) everything behind that GEMM is one HIP launch per direction
(``ops.qmix_mix``, csrc/qmix.hip) and the GEMM itself is ``ops.linear``; CPU tensors, float64 and other shapes keep the torch
formulation below, which is also the kernels' oracle.
"""
import os

import torch as th
import torch.nn as nn
import torch.nn.functional as F

from .. import ops

QMIX_FUSED = os.environ.get("UAVGNN_QMIX_FUSED", "1") != "0"   # False: the torch formulation everywhere (A/B switch, tools/qmix_probe.py)


def mix_torch(proj, qs, n, e, v2_weight, v2_bias):
    """The mixing tail in torch ops (mixers.py:31-45): proj [rows, (n+3) e] with the column blocks w1 | w_final | b1 | v_hid, qs [rows, n]
    -> q_tot [rows, 1].  What CPU / float64 / unsupported shapes run, and the oracle of ``ops.qmix_mix``."""
    w1, w_final, b1, v_hid = proj.split((n * e, e, e, e), 1)
    hidden = F.elu((qs.reshape(-1, n, 1) * w1.abs().view(-1, n, e)).sum(1) + b1)      # monotone: |w| >= 0
    v = F.linear(F.relu(v_hid), v2_weight, v2_bias)
    return (hidden * w_final.abs()).sum(1, keepdim=True) + v


class QMixer(nn.Module):
    def __init__(self, state_shape, n_agents, args):
        super().__init__()
        self.n_agents, self.state_dim, self.embed_dim = n_agents, int(state_shape), args.embed_dim
        self.hyper_w_1 = nn.Linear(self.state_dim, self.embed_dim * self.n_agents)
        self.hyper_w_final = nn.Linear(self.state_dim, self.embed_dim)
        self.hyper_b_1 = nn.Linear(self.state_dim, self.embed_dim)
        self.V = nn.Sequential(nn.Linear(self.state_dim, self.embed_dim), nn.ReLU(), nn.Linear(self.embed_dim, 1))

    def forward(self, agent_qs, states):
        """agent_qs [T, B, n], states [T, B, state_dim] -> q_tot [T, B, 1]."""
        T, B = agent_qs.shape[:2]
        n, e = self.n_agents, self.embed_dim
        heads = (self.hyper_w_1, self.hyper_w_final, self.hyper_b_1, self.V[0])
        W, b = th.cat([m.weight for m in heads], 0), th.cat([m.bias for m in heads], 0)
        s2, q2 = states.reshape(-1, self.state_dim), agent_qs.reshape(-1, n)
        if QMIX_FUSED and s2.is_cuda and q2.is_cuda and s2.dtype == q2.dtype == W.dtype == th.float32 \
                and 1 <= n <= ops.QMIX_MAX_AGENTS and 1 <= e <= ops.QMIX_MAX_EMBED:
            proj = ops.linear(s2, W, b)        # the weight gradient takes the package's split-K paths, the bias gradient _colsum
            return ops.qmix_mix(proj, q2, self.V[2].weight, self.V[2].bias).view(T, B, 1)
        return mix_torch(F.linear(s2, W, b), q2, n, e, self.V[2].weight, self.V[2].bias).view(T, B, 1)
