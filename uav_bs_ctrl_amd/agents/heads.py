"""Q heads of the agent.

``DuelingLayer`` keeps the reference's parameter layout (``adv_head``, ``v_head``; algos/madrqn/agents/dueling.py:4-16)
so checkpoints interchange: q = V + (A - mean_a A).  On CUDA fp32 with H in {64, 128, 256} and at most 15 actions both heads
and the combine are ONE launch of csrc/head.hip on the live parameters (``ops.dueling_head``); everywhere else - CPU, float64,
other shapes, ``ops.DUEL_FUSED = False`` - ONE GEMM over the stacked [n_actions + 1, H] weight and the combine in torch.

``NoisyLinear`` is the factorised-Gaussian noisy head (Fortunato et al., 2018; include/uavgnn_ext.h has the noise stream): the means
keep ``nn.Linear``'s names and layout - it IS an ``nn.Linear``, so with its mode "off" (the default, and what every evaluation
uses) each call site of the plain head computes the plain head on the means, launch for launch.  ``noisy_mode`` sets the mode of a
network's heads for a scope: "rows" (training rollouts: one draw per row inside ONE launch of csrc/ext/noisy_head.hip, one step of the
module's device pair ``rng_state`` consumed per call) or "shared" (an update: ONE draw folded into effective parameters at the start
of the scope, ``ops.noisy_fold``, used by every step of that scope).

``QuantileLinear`` is the distributional head in quantile-regression form (QR-DQN; include/uavgnn_qr.h): K quantile values per action
under ``nn.Linear``'s parameter names, ``weight [A*K, H]`` / ``bias [A*K]``.  It is NOT an ``nn.Linear``: the fused TarMAC step keys on
that type and has no form for a head this wide, so an agent with this head takes the generic route (communication block, then the
head).  ``quantile_mode`` sets what a call returns for a scope: "mean" (the default: q [N, A], the mean over the quantiles - rollouts,
``act``, evaluations, films) or "quantiles" (theta [N, A*K]: the two forward passes of an update).
"""
import contextlib
import math

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


class _Fold:
    """One shared draw of a NoisyLinear: the effective parameters (with autograd history into the four parameters when grad was
    enabled), the noise, and the halves of the sunk gradient that have arrived (``ops.tarmac_step``)."""
    __slots__ = ("W", "b", "f_in", "f_out", "pending", "done")

    def __init__(self, W, b, f_in, f_out):
        self.W, self.b, self.f_in, self.f_out = W, b, f_in, f_out
        self.pending, self.done = {}, False


class NoisyLinear(nn.Linear):
    """q = h W^T + b, W = weight + weight_sigma (.) (f(xi_out) f(xi_in)^T), b = bias + bias_sigma (.) f(xi_out), f(z) = sign(z) sqrt|z|.
    ``weight`` / ``bias`` ~ U(-1/sqrt(H), 1/sqrt(H)), both sigmas = sigma0 / sqrt(H).  ``rng_state``: the device int64 {seed, step} pair of
    the noise stream - like DiscreteComm's: None until first use, then seeded from torch's default generator (the rank mixed in under
    torch.distributed), not part of the state_dict; every consuming launch advances the step by an in-place device add (replays under
    graph capture).  ``noise``: injected noise for tests, consumed by the next draw - (f_in [H], f_out [A]) for a shared draw,
    (f_in [N, H], f_out [N, A]) for a per-row one."""

    def __init__(self, in_feats, n_actions, sigma0):
        super().__init__(in_feats, n_actions)
        self.sigma0 = float(sigma0)
        bound = 1.0 / math.sqrt(in_feats)
        self.weight_sigma = nn.Parameter(th.empty(n_actions, in_feats))
        self.bias_sigma = nn.Parameter(th.empty(n_actions))
        with th.no_grad():
            self.weight.uniform_(-bound, bound)
            self.bias.uniform_(-bound, bound)
            self.weight_sigma.fill_(self.sigma0 * bound)
            self.bias_sigma.fill_(self.sigma0 * bound)
        self.noisy_mode = "off"
        self.noise = None
        self.rng_state = None
        self._fold = None

    def extra_repr(self):
        return super().extra_repr() + f", sigma0={self.sigma0}"

    def rng(self):
        """The module's pair, seeded on first use (DiscreteComm.forward's rule)."""
        dev = self.weight.device
        if self.rng_state is None or self.rng_state.device != dev:
            seed = int(th.randint(0, 2 ** 62, (1,)).item())      # from torch's (seedable) default generator
            if th.distributed.is_available() and th.distributed.is_initialized():
                seed = (seed ^ (th.distributed.get_rank() * 0x9E3779B97F4A7C15)) & (2 ** 62 - 1)
            self.rng_state = th.tensor([seed, 0], dtype=th.int64, device=dev)
        return self.rng_state

    def params(self):
        return self.weight, self.weight_sigma, self.bias, self.bias_sigma

    def fold(self):
        """The scope's shared draw (mode "shared"); drawn once, one step consumed."""
        if self._fold is None:
            noise, self.noise = self.noise, None
            rng = self.rng() if noise is None and self.weight.is_cuda else None
            self._fold = _Fold(*ops.noisy_fold(*self.params(), rng=rng, noise=noise))
            if rng is not None:
                rng[1:].add_(1)
        return self._fold

    def rows(self, h):
        """Mode "rows": q [N, A] with one draw per row of h, no autograd; one step consumed."""
        noise, self.noise = self.noise, None
        rng = noise if noise is not None else (self.rng() if h.is_cuda else None)
        with th.no_grad():
            q = ops.head_fwd(h, self.weight, self.bias, noisy=(self.weight_sigma, self.bias_sigma, rng))
        if isinstance(rng, th.Tensor):
            rng[1:].add_(1)
        return q

    def forward(self, x):
        if self.noisy_mode == "off":
            return ops.linear(x, self.weight, self.bias) if x.dim() == 2 else super().forward(x)
        if self.noisy_mode == "rows":
            if th.is_grad_enabled() and (x.requires_grad or self.weight.requires_grad):
                raise ops.L.UavGnnError("NoisyLinear: mode 'rows' is the no-grad rollout form; an update runs under noisy_mode(net, 'shared')")
            return self.rows(x)
        f = self.fold()
        return ops.linear(x, f.W, f.b) if x.dim() == 2 else nn.functional.linear(x, f.W, f.b)


def noisy_heads(net):
    """The NoisyLinear modules of a network (a list; empty for every other head form)."""
    return [m for m in net.modules() if isinstance(m, NoisyLinear)]


@contextlib.contextmanager
def noisy_mode(net, mode):
    """Sets the mode of the noisy heads of `net` (a module, or the list ``noisy_heads`` gave) for the scope: "off", "rows" or "shared".
    "shared" draws each head's fold on entry (under the grad mode of the caller); the previous mode and fold return on exit."""
    if mode not in ("off", "rows", "shared"):
        raise ValueError(f"noisy_mode: unknown mode {mode!r} (off, rows, shared)")
    heads = net if isinstance(net, (list, tuple)) else noisy_heads(net)
    prev = [(m.noisy_mode, m._fold) for m in heads]
    for m in heads:
        m.noisy_mode, m._fold = mode, None
        if mode == "shared":
            m.fold()
    try:
        yield heads
    finally:
        for m, (mode0, fold0) in zip(heads, prev):
            m.noisy_mode, m._fold = mode0, fold0


class QuantileLinear(nn.Module):
    """theta = h W^T + b with W [A*K, H], b [A*K]: theta[n, a*K + i] is the value of action a at the fraction tau_i = (2 i + 1) / (2 K);
    Q(a) = mean_i theta[a, i].  Initialised like ``nn.Linear(in_feats, A*K)``.  Mode "mean" without autograd on the GPU: ONE
    ``uavgnn_qr_mean_fold`` launch gives (W_bar, b_bar), then the plain head runs on them.  The fold is recomputed per call - the fused
    optimizer writes parameters through raw pointers, so no version counter tells when they changed, and a call inside a captured graph
    must replay with the parameters of the replay.  Under grad, on the CPU or in float64 "mean" is the torch expression."""

    def __init__(self, in_feats, n_actions, K):
        super().__init__()
        if isinstance(K, bool) or not isinstance(K, int) or K not in ops.QR_K:
            raise ValueError(f"quantiles: K must be one of {ops.QR_K}, got {K!r}")
        if not 1 <= n_actions <= 64:
            raise ValueError(f"quantiles: 1 <= n_actions <= 64 expected, got {n_actions}")
        self.in_features, self.n_actions, self.K = in_feats, n_actions, K
        lin = nn.Linear(in_feats, n_actions * K)
        self.weight, self.bias = lin.weight, lin.bias
        self.quantile_mode = "mean"

    def extra_repr(self):
        return f"in_features={self.in_features}, n_actions={self.n_actions}, K={self.K}"

    def forward(self, x):
        A, K = self.n_actions, self.K
        if self.quantile_mode == "quantiles":
            return ops.linear(x, self.weight, self.bias) if x.dim() == 2 else nn.functional.linear(x, self.weight, self.bias)
        needs_grad = th.is_grad_enabled() and (x.requires_grad or self.weight.requires_grad or self.bias.requires_grad)
        if needs_grad or x.dim() != 2 or not (x.is_cuda and x.dtype == th.float32 and self.weight.is_cuda):
            W_bar, b_bar = ops.quantile_mean_fold_torch(self.weight, self.bias, A, K)
            return nn.functional.linear(x, W_bar, b_bar)
        with th.no_grad():
            W_bar, b_bar = ops.quantile_mean_fold(self.weight, self.bias, A, K)
            return ops.head_fwd(x if x.is_contiguous() else x.contiguous(), W_bar, b_bar)


def quantile_heads(net):
    """The QuantileLinear modules of a network (a list; empty for every other head form)."""
    return [m for m in net.modules() if isinstance(m, QuantileLinear)]


@contextlib.contextmanager
def quantile_mode(net, mode):
    """Sets what the quantile heads of `net` (a module, or the list ``quantile_heads`` gave) return for the scope: "mean" or
    "quantiles"; the previous mode returns on exit."""
    if mode not in ("mean", "quantiles"):
        raise ValueError(f"quantile_mode: unknown mode {mode!r} (mean, quantiles)")
    heads = net if isinstance(net, (list, tuple)) else quantile_heads(net)
    prev = [m.quantile_mode for m in heads]
    for m in heads:
        m.quantile_mode = mode
    try:
        yield heads
    finally:
        for m, mode0 in zip(heads, prev):
            m.quantile_mode = mode0


def build_head(in_feats, n_actions, args):
    """The Q head an agent's `args` ask for: DuelingLayer (``dueling``), NoisyLinear (``noisy`` = sigma0, a number), QuantileLinear
    (``quantiles`` = K, an int) or nn.Linear."""
    K = getattr(args, "quantiles", None)
    if K is not None and not isinstance(K, bool) and isinstance(K, int):
        if getattr(args, "dueling", False):
            raise ValueError("quantiles together with dueling is not supported: the dueling quantile head does not exist; set one of the two")
        if getattr(args, "noisy", None) is not None:
            raise ValueError("quantiles together with noisy is not supported: the noisy quantile head does not exist; set one of the two")
        return QuantileLinear(in_feats, n_actions, K)
    sigma0 = getattr(args, "noisy", None)
    if sigma0 is not None and not isinstance(sigma0, bool) and isinstance(sigma0, (int, float)):
        if getattr(args, "dueling", False):
            raise ValueError("dueling together with noisy is not supported: the noisy dueling head does not exist yet; set one of the two")
        return NoisyLinear(in_feats, n_actions, sigma0)
    if getattr(args, "dueling", False):
        return DuelingLayer(in_feats, n_actions)
    return nn.Linear(in_feats, n_actions)
