"""Tensor-native sequence replay - counterpart of algos/madrqn/buffer.py:7-42.

The reference keeps a deque of Python dicts holding one DGLGraph per time step and re-batches 32 x (T+1) of them with
``dgl.batch`` on every update (learner.py:99-116).  Here a fixed-length sequence of env steps is a row of a ring of
HBM-resident PADDED observation tensors (the simulator's own format, mubs_cov.py:215-242: gt [n,M,5], ubs [n,n-1,3],
agent [n,2], plus d_u2u [n,n] for the talk relation); sampling is an index gather and the graphs of a sampled batch are
rebuilt on the device by ``from_padded_obs`` (two HIP passes per time step).  Same sequence semantics as the
reference: T transitions per sequence plus the next observation / hidden state of the last one (buffer.py:26-35);
``h`` is stored per step so that ``h[0]`` / ``h[1]`` seed the policy / target BPTT (learner.py:113).

Storage per sequence at 8 x 80, T = 50:  51*8*80*5*4 B = 653 KB of GT rows (+ 4 % for the rest)  ->  5 000 sequences
(the reference's replay_size) = 3.4 GB of the 288 GB.

``device_state=True`` (opt-in) moves what was left on the host - the ring position, the sampler, the batch's way into a captured update
- to the device (csrc/replay.hip), so that a hipGraph can hold commits, samples and gathers (``graphs.GraphedEpisode``); the default keeps
the host path as it was.

``CompactSequenceReplay`` (opt-in, device-state only) stores the simulator state the observations are a pure function of - 48.7 KB per
sequence at 8 x 50, T = 50, H = 256 against 881 KB - and rebuilds the update's buffers in its gather (csrc/replay_rebuild.hip), bit for bit.
"""
from __future__ import annotations

from typing import Dict, Optional

import ctypes

import torch as th

from . import _lib as L
from .graph import HeteroBatch, from_obs_dicts, from_padded_obs, from_padded_obs_flat, from_single_ubs_obs, batch as hb_batch

SCHEME = ("gt", "ubs", "agent", "d_u2u", "h", "state", "act", "rew", "done")
NARROW_SAMPLER_CAPACITY = 65536      # uavgnn_replay_sample: one workgroup, one launch; above it uavgnn_replay_sample_wide
MAX_DEVICE_CAPACITY = 2 ** 30        # the limit of uavgnn_replay_sample_wide
PRIO_ONE = 1 << 20                   # the fixed-point 1.0 of a priority (csrc/replay_prio.hip)


def _check_prioritized(prioritized, device_state: bool):
    """None, or (alpha, beta, eta, eps) as four floats: explicit numbers - the package keeps no defaults."""
    if prioritized is None:
        return None
    if not device_state:
        raise ValueError("prioritized: priorities live on the device (device_state=True); a host-state ring has none")
    try:
        alpha, beta, eta, eps = (float(v) for v in prioritized)
    except (TypeError, ValueError):
        raise ValueError(f"prioritized: None or four numbers (alpha, beta, eta, eps) expected, got {prioritized!r}") from None
    if not (alpha >= 0.0 and 0.0 <= beta <= 16.0 and 0.0 <= eta <= 1.0 and eps >= 0.0) or float("inf") in (alpha, eps):
        raise ValueError(f"prioritized = (alpha, beta, eta, eps) = {(alpha, beta, eta, eps)}: finite alpha, eps >= 0, beta in [0, 16] "
                         f"(the sampler's weights stay finite) and eta in [0, 1] expected")
    return alpha, beta, eta, eps


class _RingState:
    """Ring position and sampler of both replays.  Default: Python integers ``head`` / ``size`` and ``torch.randperm`` - the host path.
    ``device_state=True``: ``state`` int64 {head, size}, ``rng`` int64 {seed, draws} and ``status`` int32 [1] are DEVICE tensors; the
    commit, the sampler and the gather into a captured update's buffers are one launch each (csrc/replay.hip) that read the
    counters on the device - so a hipGraph holding them replays with the CURRENT ring position (``graphs.GraphedEpisode``).
    ``prioritized=(alpha, beta, eta, eps)`` (opt-in, device state only; None - the default - leaves every launch as it was): proportional
    prioritised replay over sequences (csrc/replay_prio.hip).  ``prio`` [capacity] / ``prio_max`` [1] hold unsigned 32-bit FIXED-POINT
    priorities (2^20 = 1.0) as the bits of int32 tensors; a commit gives the new sequences ``prio_max``, ``sample_indices`` draws
    stratified and proportional WITH replacement (ascending slots, repeats possible) and leaves the importance weights in
    ``is_weights`` [B], ``update_priorities(idx, td)`` rewrites the priorities of a batch from its TD errors.
    A class sets ``_scheme`` (its field names: ``_obs_fields``, the observation side of a transition, then act / rew / done) and
    ``mem`` / ``cur`` / ``capacity`` / ``T`` / ``n_envs`` / ``device`` before ``_init_ring_state``."""

    def push(self, tr: Dict[str, th.Tensor]) -> None:
        """One transition of every parallel env.  tr: the ``_obs_fields`` [E, ...] (observation BEFORE the action; may be absent when
        staged), act / rew / done and the ``next_*`` observation fields (madrqn/buffer.py:18-35, drqn/buffer.py:17-29)."""
        self.stage_obs(tr)
        for k in ("act", "rew", "done"):
            self.cur[k][:, self.ptr] = tr[k]
        self.ptr += 1
        if self.ptr == self.T:
            for k in self._obs_fields:
                if "next_" + k in tr:
                    self.cur[k][:, self.T] = tr["next_" + k]
            self._commit()
            self.ptr = 0

    def stage_obs(self, tr: Dict[str, th.Tensor]) -> None:
        """The observation half of the current transition (the ``_obs_fields`` BEFORE the action), written at the current step
        WITHOUT advancing: a simulator that overwrites its observation buffers in place can be stepped before ``push`` receives
        act / rew / done / next_* - no clone of the observation in between."""
        for k in self._obs_fields:
            if k in tr:
                self.cur[k][:, self.ptr] = tr[k]

    def _check_device_state(self, device_state: bool, prioritized=None) -> None:
        """What ``device_state=True`` asks of ``device`` / ``n_envs`` / ``capacity``, and ``prioritized`` of ``device_state`` - a constructor
        calls it BEFORE it allocates the ring."""
        self.prioritized = _check_prioritized(prioritized, bool(device_state))
        if not device_state:
            return
        if self.device.type != "cuda":
            raise ValueError("device_state=True: the ring counters and the sampler live on the GPU (no CPU fallback exists)")
        if self.n_envs > self.capacity:
            raise ValueError(f"device_state=True: one commit of n_envs = {self.n_envs} sequences exceeds capacity = {self.capacity}")
        if self.capacity > MAX_DEVICE_CAPACITY:
            raise ValueError(f"device_state=True: capacity = {self.capacity} exceeds the device sampler's limit of 2^30 = "
                             f"{MAX_DEVICE_CAPACITY} sequences")

    def _init_ring_state(self, device_state: bool, seed: Optional[int], is_weights: Optional[th.Tensor] = None) -> None:
        self.device_state = bool(device_state)
        self.ptr = 0            # time index inside the sequences under construction (buffer.py:16)
        self.head = 0           # next ring slot
        self.size = 0
        if not self.device_state:
            if seed is not None:
                raise ValueError("seed: the key of the device sampler (device_state=True); the host sampler takes generator=")
            return
        self._check_device_state(True, self.prioritized)
        if seed is None:       # from torch's default generator: torch.manual_seed reproduces a run
            seed = int(th.randint(0, 2 ** 62, (1,)).item())
        self.head = self.size = None                          # the counters are ``state`` on the device
        self.state = th.zeros(2, dtype=th.int64, device=self.device)
        self.rng = th.tensor([int(seed), 0], dtype=th.int64, device=self.device)
        self.status = th.zeros(1, dtype=th.int32, device=self.device)
        # capacity > 65 536: the many-workgroup sampler and its scratch (fixed address: a captured draw replays on it; nothing in it
        # outlives a draw, so neither state.pt nor a resumed run knows it).  Up to 65 536 the one-launch sampler, as before.
        self._sample_ws = None
        if self.capacity > NARROW_SAMPLER_CAPACITY:
            self._sample_ws = th.empty(L.lib().uavgnn_replay_sample_wide_workspace_bytes(self.capacity), dtype=th.uint8, device=self.device)
        rows = []
        for k in self._scheme:
            src, dst = self.cur[k], self.mem[k]
            if src.numel() > 0:
                rows += [src.data_ptr(), dst.data_ptr(), src[0].numel() * src.element_size()]
        self._commit_fields = (ctypes.c_longlong * len(rows))(*rows)
        if self.prioritized is not None:
            self._init_priorities(is_weights)

    def _init_priorities(self, is_weights: Optional[th.Tensor]) -> None:
        """``prioritized=(alpha, beta, eta, eps)``: one fixed-point priority per ring slot (uint32 bits in an int32 tensor; ``PRIO_ONE`` =
        2^20 = 1.0), the running maximum new sequences are committed with, and - per batch size, at fixed addresses, so a captured draw
        replays on them - the sampler's scratch and the importance weights ``is_weights`` [B] of the LAST draw."""
        self.prio = th.full((self.capacity,), PRIO_ONE, dtype=th.int32, device=self.device)
        self.prio_max = th.full((1,), PRIO_ONE, dtype=th.int32, device=self.device)
        self.is_weights, self._prio_ws, self._prio_batch = None, None, None
        if is_weights is not None:
            if is_weights.dim() != 1 or is_weights.dtype != th.float32 or not is_weights.is_contiguous() or is_weights.device != self.prio.device:
                raise ValueError("is_weights: a contiguous float32 [B] tensor on the ring's device expected")
            self._prio_buffers(is_weights.numel(), is_weights)

    def reserve_batch(self, batch_size: int) -> th.Tensor:
        """``is_weights`` for draws of ``batch_size`` sequences, allocated now if no draw has fixed it yet - what a captured update binds."""
        if self.prioritized is None:
            raise ValueError("reserve_batch needs prioritized=(alpha, beta, eta, eps)")
        if self._prio_batch is None:
            self._prio_buffers(int(batch_size))
        if int(batch_size) != self._prio_batch:
            raise ValueError(f"prioritized: is_weights holds {self._prio_batch} weights, a batch of {batch_size} was asked for")
        return self.is_weights

    def _prio_buffers(self, B: int, is_weights: Optional[th.Tensor] = None) -> None:
        n = L.lib().uavgnn_replay_prio_workspace_bytes(self.capacity, B)
        if n <= 0:
            raise ValueError(f"prioritized: a batch of {B} sequences is outside the sampler's range [1, 65535]")
        self._prio_ws = th.empty(n, dtype=th.uint8, device=self.device)
        self.is_weights = th.ones(B, dtype=th.float32, device=self.device) if is_weights is None else is_weights
        self._prio_batch = B

    def __len__(self) -> int:
        """Committed sequences.  device_state=True: reads ``state`` from the device - a host SYNCHRONISATION (never inside a capture)."""
        return int(self.state[1].item()) if self.device_state else self.size

    def _commit(self) -> None:
        """The E sequences under construction -> ring slots (head + e) % capacity; head and size advance (buffer.py:31)."""
        E = self.n_envs
        if self.device_state:
            if self.prioritized is not None:          # first: it reads `head`, which the commit's second launch advances
                L.check(L.lib().uavgnn_replay_prio_commit(self.state.data_ptr(), E, self.capacity, self.prio.data_ptr(),
                                                          self.prio_max.data_ptr(), L.stream()), "uavgnn_replay_prio_commit")
            L.check(L.lib().uavgnn_replay_commit(self._commit_fields, len(self._commit_fields) // 3, E, self.capacity,
                                                 self.state.data_ptr(), L.stream()), "uavgnn_replay_commit")
            return
        slots = (self.head + th.arange(E, device=self.device)) % self.capacity
        for k in self._scheme:
            self.mem[k][slots] = self.cur[k]
        self.head = (self.head + E) % self.capacity
        self.size = min(self.size + E, self.capacity)

    def sample_indices(self, batch_size: int, generator: Optional[th.Generator] = None) -> th.Tensor:
        """Without replacement, like ``random.sample`` (buffer.py:37-39).  device_state=True: one sampler launch keyed by the device
        ``rng`` pair - a uniform subset in ASCENDING slot order (``random.sample`` returns a random order; the loss is a mean over
        the batch) - no host synchronisation: asking for more than the ring holds sets ``status`` (``check()``).
        capacity > 65 536: the same draw, bit for bit, from the many-workgroup sampler (seven launches, csrc/replay_wide.hip)."""
        if self.device_state:
            if generator is not None:
                raise ValueError("device_state=True: the sampler is keyed by the device `rng` pair, not by a torch generator")
            idx = th.empty(batch_size, dtype=th.int64, device=self.device)
            if self.prioritized is not None:
                return self._sample_prioritized(idx)
            if self._sample_ws is not None:
                L.check(L.lib().uavgnn_replay_sample_wide(self.state.data_ptr(), self.rng.data_ptr(), self.capacity, batch_size,
                                                          idx.data_ptr(), self.status.data_ptr(), self._sample_ws.data_ptr(), L.stream()),
                        "uavgnn_replay_sample_wide")
                return idx
            L.check(L.lib().uavgnn_replay_sample(self.state.data_ptr(), self.rng.data_ptr(), self.capacity, batch_size,
                                                 idx.data_ptr(), self.status.data_ptr(), L.stream()), "uavgnn_replay_sample")
            return idx
        assert self.size >= batch_size, "Insufficient samples for update."
        return th.randperm(self.size, generator=generator, device=self.device)[:batch_size]

    def _sample_prioritized(self, idx: th.Tensor) -> th.Tensor:
        """Stratified proportional draw WITH replacement (uavgnn_replay_prio_sample, four launches): ascending slots, repeats possible;
        the importance weights of the draw, normalised by their maximum, are left in ``is_weights`` (one buffer per ring: the first
        draw fixes the batch size unless the constructor was given the buffer)."""
        B = idx.numel()
        self.reserve_batch(B)
        L.check(L.lib().uavgnn_replay_prio_sample(self.state.data_ptr(), self.rng.data_ptr(), self.capacity, B, self.prio.data_ptr(),
                                                  float(self.prioritized[1]), idx.data_ptr(), self.is_weights.data_ptr(),
                                                  self.status.data_ptr(), self._prio_ws.data_ptr(), L.stream()), "uavgnn_replay_prio_sample")
        return idx

    def update_priorities(self, idx: th.Tensor, td: th.Tensor) -> None:
        """New priorities of the sampled sequences ``idx`` [B] (ascending, as drawn) from the TD errors ``td`` [T, B, C] of the update formed
        on them: eta max|td| + (1 - eta) mean|td| per sequence, (. + eps)^alpha in fixed point; ``prio_max`` grows with them.  One launch
        (uavgnn_replay_prio_update); a non-finite row is skipped and sets status bit 1 (``check()``)."""
        if self.prioritized is None:
            raise ValueError("update_priorities needs prioritized=(alpha, beta, eta, eps)")
        if idx.dtype != th.int64 or not idx.is_contiguous():
            raise ValueError("idx: a contiguous int64 tensor expected")
        if td.dim() != 3 or td.shape[1] != idx.numel() or td.dtype != th.float32 or not td.is_contiguous():
            raise ValueError(f"td: a contiguous float32 [T, {idx.numel()}, C] tensor expected, got {tuple(td.shape)} {td.dtype}")
        L.require_gpu(idx, td)
        alpha, _, eta, eps = self.prioritized
        T, B, C = td.shape
        L.check(L.lib().uavgnn_replay_prio_update(td.data_ptr(), T, B, C, idx.data_ptr(), self.capacity, alpha, eta, eps,
                                                  self.prio.data_ptr(), self.prio_max.data_ptr(), self.status.data_ptr(), L.stream()),
                "uavgnn_replay_prio_update")

    def check(self) -> None:
        """Raises when a kernel of the device-resident path flagged an error (a host synchronisation)."""
        if self.device_state and int(self.status.item()) != 0:
            raise L.UavGnnError(f"replay status = {int(self.status.item()):#x}: bit 0 - a batch larger than the number of committed "
                                f"sequences was sampled (its indices were wrapped into the ring)"
                                + ("; bit 1 - a priority update was skipped (non-finite TD errors, or an index outside the ring)"
                                   if self.prioritized is not None else ""))

    def _gather_fields(self, target, B: int):
        """[(ring tensor, first step, destination, steps)] of ``gather_into``: a class lists what its update buffers hold."""
        raise NotImplementedError

    def gather_into(self, idx: th.Tensor, target) -> None:
        """Every field of the sampled sequences ``idx`` from the ring straight into the time-major fixed-address buffers of
        ``target`` - a ``graphs.GraphedUpdate`` / ``GraphedSingleUbsUpdate`` or any object with their buffer attributes - in ONE
        launch (uavgnn_replay_gather).  Same bits as ``index_select`` per field followed by ``target.load``."""
        if not self.device_state:
            raise ValueError("gather_into needs device_state=True")
        if idx.dtype != th.int64 or not idx.is_contiguous():
            raise ValueError("idx: a contiguous int64 tensor expected")
        L.require_gpu(idx)
        B = idx.numel()
        rows = []
        for name, src, t0, dst, steps in self._gather_fields(target, B):
            slab = src[0, 0].numel()
            if slab == 0:
                continue
            if dst.dtype != src.dtype or not dst.is_contiguous() or dst.numel() != steps * B * slab or not dst.is_cuda:
                raise ValueError(f"gather_into: {name}: a contiguous {src.dtype} buffer of {steps} x {B} x {slab} elements expected, "
                                 f"got {tuple(dst.shape)} {dst.dtype}")
            es = src.element_size()
            rows += [src.data_ptr() + t0 * slab * es, dst.data_ptr(), slab * es, steps, src.stride(0) * es, B * slab * es, self.capacity]
        fields = (ctypes.c_longlong * len(rows))(*rows)
        L.check(L.lib().uavgnn_replay_gather(fields, len(rows) // 7, idx.data_ptr(), B, L.stream()), "uavgnn_replay_gather")


class SequenceReplay(_RingState):
    _scheme, _obs_fields = SCHEME, ("gt", "ubs", "agent", "d_u2u", "h", "state")
    step_fields = ("gt", "ubs", "agent", "d_u2u")    # what ``learner.cache`` takes from ``obs`` / ``next_obs``

    def __init__(self, capacity: int, max_seq_len: int, n_agents: int, n_gts: int, hidden_size: int,
                 n_envs: int = 1, state_dim: int = 0, r_comm: float = float("inf"), rew_dim: Optional[int] = None,
                 device="cuda", device_state: bool = False, seed: Optional[int] = None, prioritized=None,
                 is_weights: Optional[th.Tensor] = None):
        T, n, M = max_seq_len, n_agents, n_gts
        self.capacity, self.T, self.n, self.M, self.n_envs = capacity, T, n, M, n_envs
        self.r_comm, self.device = r_comm, th.device(device)
        self._check_device_state(device_state, prioritized)
        f = dict(dtype=th.float32, device=self.device)
        rd = n if rew_dim is None else rew_dim

        def ring(lead):  # committed sequences / sequences under construction (one per parallel env)
            return dict(gt=th.zeros(lead, T + 1, n, M, 5, **f), ubs=th.zeros(lead, T + 1, n, max(n - 1, 0), 3, **f),
                        agent=th.zeros(lead, T + 1, n, 2, **f), d_u2u=th.zeros(lead, T + 1, n, n, **f),
                        h=th.zeros(lead, T + 1, n, hidden_size, **f), state=th.zeros(lead, T + 1, state_dim, **f),
                        act=th.zeros(lead, T, n, dtype=th.int64, device=self.device), rew=th.zeros(lead, T, rd, **f),
                        done=th.zeros(lead, T, 1, **f))
        self.mem = ring(capacity)
        self.cur = ring(n_envs)
        self._init_ring_state(device_state, seed, is_weights)

    def _gather_fields(self, target, B: int):
        m, o, T = self.mem, target.obs, self.T
        out = [("gt", m["gt"], 0, o.gt, T + 1), ("ubs", m["ubs"], 0, o.ubs, T + 1), ("agent", m["agent"], 0, o.agent, T + 1)]
        if o.d_u2u is not None:
            out.append(("d_u2u", m["d_u2u"], 0, o.d_u2u, T + 1))
        if getattr(target, "states", None) is not None:
            out.append(("state", m["state"], 0, target.states, T + 1))
        return out + [("h0", m["h"], 0, target.h0, 1), ("h1", m["h"], 1, target.h1, 1), ("act", m["act"], 0, target.acts, T),
                      ("rew", m["rew"], 0, target.rews, T), ("done", m["done"], 0, target.dones, T)]

    def gather(self, idx: th.Tensor, enc: str = "gnn") -> Dict:
        """Batch dict in the layout ``MultiAgentQLearner.loss`` consumes: obs = list of T+1 HeteroBatch of B envs.
        enc='mlp': flattened-observation batches (``from_padded_obs_flat``) over a time-major copy of the gathered observations, plus
        ``obs_all`` / ``obs_all_next`` (row views of the same copy) for the learner's time-batched encoder."""
        B, T, n = idx.numel(), self.T, self.n
        if enc not in ("gnn", "mlp"):
            raise ValueError(f"enc must be 'gnn' or 'mlp', got {enc!r}")
        if enc == "mlp" and self.device.type != "cuda":
            raise ValueError("enc='mlp': flattened-observation batches are built on the GPU only (graph.from_padded_obs_flat)")
        obs_keys = ("gt", "ubs", "agent", "d_u2u")
        # enc='mlp': the observation fields are gathered TIME-MAJOR in the one copy of the gather ([T+1, B, ...]: index_select along the
        # sequence dimension of the transposed ring), so every step and the time-batched rows are views the flat builder keeps as they are
        m = {k: v.index_select(0, idx) for k, v in self.mem.items() if not (enc == "mlp" and k in obs_keys)}
        out = dict(h0=m["h"][:, 0].reshape(B * n, -1), h1=m["h"][:, 1].reshape(B * n, -1),
                   acts=m["act"].permute(1, 0, 2).reshape(T, B * n, 1), rews=m["rew"].permute(1, 0, 2).contiguous(),
                   dones=m["done"].permute(1, 0, 2).contiguous(), states=m["state"].permute(1, 0, 2).contiguous())
        if enc == "mlp":
            tm = {k: self.mem[k].transpose(0, 1).index_select(1, idx) for k in obs_keys}              # [T+1, B, ...]
            rows = lambda x, lo: x[lo:].reshape(((x.shape[0] - lo) * x.shape[1],) + x.shape[2:])  # noqa: E731  (no -1: ubs is empty at n = 1)
            out["obs"] = [from_padded_obs_flat(tm["gt"][t], tm["ubs"][t], tm["agent"][t], tm["d_u2u"][t], self.r_comm)
                          for t in range(T + 1)]
            out["obs_all"] = from_padded_obs_flat(rows(tm["gt"], 0), rows(tm["ubs"], 0), rows(tm["agent"], 0))
            out["obs_all_next"] = from_padded_obs_flat(rows(tm["gt"], 1), rows(tm["ubs"], 1), rows(tm["agent"], 1))
            return out
        obs = []
        for t in range(T + 1):
            if self.device.type == "cuda":
                obs.append(from_padded_obs(m["gt"][:, t], m["ubs"][:, t], m["agent"][:, t], m["d_u2u"][:, t],
                                           self.r_comm))
            else:   # host path (tests): the vectorised host builder per env
                gs = []
                for b in range(B):
                    o = [dict(agent=m["agent"][b, t, i].numpy(), ubs=m["ubs"][b, t, i].numpy(),
                              gt=m["gt"][b, t, i].numpy()) for i in range(n)]
                    gs.append(from_obs_dicts(o, m["d_u2u"][b, t].numpy(), self.r_comm))
                obs.append(hb_batch(gs))
        out["obs"] = obs
        return out

    def sample(self, batch_size: int, generator: Optional[th.Generator] = None, enc: str = "gnn") -> Dict:
        return self.gather(self.sample_indices(batch_size, generator), enc)


COMPACT_SCHEME = ("pos_ubs", "rate", "avg", "pos_gts", "h", "act", "rew", "done")


def compact_bytes_per_sequence(n: int, M: int, T: int, H: int, rd: int) -> int:
    """Bytes of one sequence of a ``CompactSequenceReplay``: T+1 steps of pos_ubs [n,2] f64 and rate / avg [M] f32, pos_gts [M,2] f32
    once, h [2,n,H] f32, act [T,n] int64, rew [T,rd] and done [T,1] f32."""
    return (T + 1) * (16 * n + 8 * M) + 8 * M + 8 * n * H + 8 * T * n + 4 * T * rd + 4 * T


class CompactSequenceReplay(_RingState):
    """Opt-in ring of the multi-UBS experiments that stores what the simulator computes its observations FROM instead of the
    observations: per step pos_ubs [n,2] f64, rate [M] and avg [M] (``BatchedUbsCoverageEnv.replay_state()``), per sequence pos_gts
    [M,2] (staged at step 0) and the two hidden states an update reads, h [2,n,H] (steps 0 and 1), plus act / rew / done.  No ``state``
    field, also under QMIX.  ``gather_into`` REBUILDS gt / ubs / agent / d_u2u / state of the sampled sequences straight into the
    update's time-major buffers with one launch (uavgnn_replay_rebuild_obs: the arithmetic of the simulator step, so the same bits a
    ``SequenceReplay`` would have copied) and moves h0 / h1 / act / rew / done with the existing gather launch.  48.7 KB per sequence
    at 8 x 50, T = 50, H = 256 against 881 KB (``bytes_per_sequence``).

    CONTRACT: a sequence never spans a reset - pos_gts is stored once per sequence, and it changes only at a reset.
    ``graphs.Episode`` enforces ``episode_limit % T == 0`` and resets at the start of an episode, so its sequences never do.

    Device-state only (``device_state=True`` on the GPU: commit, samplers and gather of ``_RingState``); built from the environment so
    that the map's constants and shapes cannot disagree with the simulator's:

        rb = CompactSequenceReplay.for_env(env, capacity, max_seq_len, hidden_size, rew_dim=None, seed=None)     # n_envs = env.B
    """
    _scheme, _obs_fields = COMPACT_SCHEME, ("pos_ubs", "rate", "avg")
    step_fields = ("pos_ubs", "rate", "avg", "pos_gts")      # what ``learner.cache`` takes from ``obs`` / ``next_obs``

    def __init__(self, env, capacity: int, max_seq_len: int, hidden_size: int, rew_dim: Optional[int] = None,
                 device_state: bool = True, seed: Optional[int] = None, prioritized=None, is_weights: Optional[th.Tensor] = None):
        if not device_state:
            raise ValueError("CompactSequenceReplay: device_state=True only (the rebuild is a device launch; no host path exists)")
        T, n, M = max_seq_len, env.n_agents, env.n_gts
        self.capacity, self.T, self.n, self.M, self.n_envs = capacity, T, n, M, env.B
        self.r_comm, self.device = env.p.r_comm, th.device(env.device)
        if self.device.type != "cuda":
            raise ValueError("CompactSequenceReplay: the ring, its counters and the rebuild live on the GPU (no CPU fallback exists)")
        self._check_device_state(True, prioritized)
        self._ic, self._fc = env._ic, env._fc                # the constant arrays uavgnn_env_step takes
        self.Sg, self.state_dim, self.hidden_size = env.out["obs_gt"].shape[-1], env.state_dim, hidden_size
        self.rew_dim = n if rew_dim is None else rew_dim
        f = dict(dtype=th.float32, device=self.device)

        def ring(lead):  # committed sequences / sequences under construction (one per parallel env)
            return dict(pos_ubs=th.zeros(lead, T + 1, n, 2, dtype=th.float64, device=self.device), rate=th.zeros(lead, T + 1, M, **f),
                        avg=th.zeros(lead, T + 1, M, **f), pos_gts=th.zeros(lead, M, 2, **f), h=th.zeros(lead, 2, n, hidden_size, **f),
                        act=th.zeros(lead, T, n, dtype=th.int64, device=self.device), rew=th.zeros(lead, T, self.rew_dim, **f),
                        done=th.zeros(lead, T, 1, **f))
        self.mem = ring(capacity)
        self.cur = ring(self.n_envs)
        self._init_ring_state(True, seed, is_weights)

    @classmethod
    def for_env(cls, env, capacity: int, max_seq_len: int, hidden_size: int, rew_dim: Optional[int] = None, seed: Optional[int] = None,
                prioritized=None, is_weights: Optional[th.Tensor] = None):
        return cls(env, capacity, max_seq_len, hidden_size, rew_dim, True, seed, prioritized, is_weights)

    @property
    def bytes_per_sequence(self) -> int:
        return compact_bytes_per_sequence(self.n, self.M, self.T, self.hidden_size, self.rew_dim)

    def stage_obs(self, tr: Dict[str, th.Tensor]) -> None:
        """The step fields at the current step; pos_gts at step 0 only (constant until the next reset); h at steps 0 and 1 only."""
        super().stage_obs(tr)
        if self.ptr == 0 and "pos_gts" in tr:
            self.cur["pos_gts"].copy_(tr["pos_gts"])
        if self.ptr < 2 and "h" in tr:
            self.cur["h"][:, self.ptr] = tr["h"]

    def push(self, tr: Dict[str, th.Tensor]) -> None:
        if self.T == 1 and "next_h" in tr:       # the only sequence length whose h[1] is the hidden state AFTER the last transition
            self.cur["h"][:, 1] = tr["next_h"]
        super().push(tr)

    def _gather_fields(self, target, B: int):
        m, T = self.mem, self.T
        return [("h0", m["h"], 0, target.h0, 1), ("h1", m["h"], 1, target.h1, 1), ("act", m["act"], 0, target.acts, T),
                ("rew", m["rew"], 0, target.rews, T), ("done", m["done"], 0, target.dones, T)]

    def rebuild_into(self, idx: th.Tensor, gt: th.Tensor, ubs: th.Tensor, agent: th.Tensor, d_u2u: Optional[th.Tensor] = None,
                     state: Optional[th.Tensor] = None) -> None:
        """The observations of the sequences ``idx`` into time-major buffers gt [T+1,B,n,M,Sg], ubs [T+1,B,n,n-1,3], agent [T+1,B,n,2]
        and, where given, d_u2u [T+1,B,n,n] and state [T+1,B,state_dim]: ONE launch (uavgnn_replay_rebuild_obs), capturable."""
        if idx.dtype != th.int64 or not idx.is_contiguous():
            raise ValueError("idx: a contiguous int64 tensor expected")
        L.require_gpu(idx)
        B, T1, n, M = idx.numel(), self.T + 1, self.n, self.M
        shapes = dict(gt=(gt, (n, M, self.Sg)), ubs=(ubs, (n, max(n - 1, 0), 3)), agent=(agent, (n, 2)), d_u2u=(d_u2u, (n, n)),
                      state=(state, (self.state_dim,)))
        for name, (x, tail) in shapes.items():
            if x is not None and (tuple(x.shape) != (T1, B) + tail or x.dtype != th.float32 or not x.is_contiguous() or not x.is_cuda):
                raise ValueError(f"rebuild_into: {name}: a contiguous float32 buffer {(T1, B) + tail} on the GPU expected, got "
                                 f"{tuple(x.shape)} {x.dtype}")
        m = self.mem
        L.check(L.lib().uavgnn_replay_rebuild_obs(self._ic, self._fc, m["pos_ubs"].data_ptr(), m["rate"].data_ptr(), m["avg"].data_ptr(),
                                                  m["pos_gts"].data_ptr(), self.capacity, T1, idx.data_ptr(), B, gt.data_ptr(), self.Sg,
                                                  L.ptr(ubs) or None, agent.data_ptr(), L.ptr(d_u2u), L.ptr(state), L.stream()),
                "uavgnn_replay_rebuild_obs")

    def gather_into(self, idx: th.Tensor, target) -> None:
        """The update's buffers of ``target`` (a ``graphs.GraphedUpdate``) from the sequences ``idx``: the rebuild launch for ``obs.*`` and
        ``states``, the gather launch for h0 / h1 / acts / rews / dones.  Same bits as ``SequenceReplay.gather_into`` on a ring that
        stored the simulator's observations."""
        o = target.obs
        self.rebuild_into(idx, o.gt, o.ubs, o.agent, o.d_u2u, getattr(target, "states", None))
        super().gather_into(idx, target)

    def gather(self, idx: th.Tensor, enc: str = "gnn") -> Dict:
        """The batch dict ``SequenceReplay.gather`` returns, over rebuilt time-major tensors (``states``: always, [T+1, B, state_dim])."""
        B, T, n, M = idx.numel(), self.T, self.n, self.M
        if enc not in ("gnn", "mlp"):
            raise ValueError(f"enc must be 'gnn' or 'mlp', got {enc!r}")
        f = dict(dtype=th.float32, device=self.device)
        gt, ubs = th.empty(T + 1, B, n, M, self.Sg, **f), th.empty(T + 1, B, n, max(n - 1, 0), 3, **f)
        agent, d_u2u, states = th.empty(T + 1, B, n, 2, **f), th.empty(T + 1, B, n, n, **f), th.empty(T + 1, B, self.state_dim, **f)
        self.rebuild_into(idx, gt, ubs, agent, d_u2u, states)
        m = {k: self.mem[k].index_select(0, idx) for k in ("h", "act", "rew", "done")}
        out = dict(h0=m["h"][:, 0].reshape(B * n, -1), h1=m["h"][:, 1].reshape(B * n, -1),
                   acts=m["act"].permute(1, 0, 2).reshape(T, B * n, 1), rews=m["rew"].permute(1, 0, 2).contiguous(),
                   dones=m["done"].permute(1, 0, 2).contiguous(), states=states)
        if enc == "mlp":
            rows = lambda x, lo: x[lo:].reshape(((x.shape[0] - lo) * x.shape[1],) + x.shape[2:])  # noqa: E731  (no -1: ubs is empty at n = 1)
            out["obs"] = [from_padded_obs_flat(gt[t], ubs[t], agent[t], d_u2u[t], self.r_comm) for t in range(T + 1)]
            out["obs_all"] = from_padded_obs_flat(rows(gt, 0), rows(ubs, 0), rows(agent, 0))
            out["obs_all_next"] = from_padded_obs_flat(rows(gt, 1), rows(ubs, 1), rows(agent, 1))
            return out
        out["obs"] = [from_padded_obs(gt[t], ubs[t], agent[t], d_u2u[t], self.r_comm) for t in range(T + 1)]
        return out

    def sample(self, batch_size: int, generator: Optional[th.Generator] = None, enc: str = "gnn") -> Dict:
        return self.gather(self.sample_indices(batch_size, generator), enc)


SINGLE_UBS_SCHEME = ("gt", "agent", "h", "act", "rew", "done")


class SingleUbsSequenceReplay(_RingState):
    """The DRQN's replay of experiment 1 (algos/drqn/buffer.py:5-36, scheme ('obs', 'h', 'act', 'rew', 'done')) in HBM: a ring of
    fixed-length sequences of the single-UBS environment's observation FIELDS - gt [T+1, M, 4], agent [T+1, 2] - and the
    recurrent state h [T+1, H], plus act / rew / done [T, 1] per sequence row.  Same sequence semantics as the reference: T
    transitions, then the next observation / hidden state of the last one (buffer.py:23-25).  ``gather`` hands the learner either
    the T+1 `seen-by` batches (``from_single_ubs_obs`` on views of the gathered fields: no graph is ever stored or copied) or the
    T+1 flattened [B, 2+4M] tensors (agent || gt row-major)."""
    _scheme, _obs_fields = SINGLE_UBS_SCHEME, ("gt", "agent", "h")

    def __init__(self, capacity: int, max_seq_len: int, n_gts: int, hidden_size: int, n_envs: int = 1, device="cuda",
                 device_state: bool = False, seed: Optional[int] = None, prioritized=None, is_weights: Optional[th.Tensor] = None):
        T, M = max_seq_len, n_gts
        self.capacity, self.T, self.M, self.n_envs = capacity, T, M, n_envs
        self.device = th.device(device)
        self._check_device_state(device_state, prioritized)
        f = dict(dtype=th.float32, device=self.device)

        def ring(lead):  # committed sequences / sequences under construction (one per parallel env)
            return dict(gt=th.zeros(lead, T + 1, M, 4, **f), agent=th.zeros(lead, T + 1, 2, **f),
                        h=th.zeros(lead, T + 1, hidden_size, **f), act=th.zeros(lead, T, 1, dtype=th.int64, device=self.device),
                        rew=th.zeros(lead, T, 1, **f), done=th.zeros(lead, T, 1, **f))
        self.mem = ring(capacity)
        self.cur = ring(n_envs)
        self._init_ring_state(device_state, seed, is_weights)

    def _gather_fields(self, target, B: int):
        m, T = self.mem, self.T
        return [("gt", m["gt"], 0, target.gt, T + 1), ("agent", m["agent"], 0, target.agent, T + 1), ("h0", m["h"], 0, target.h0, 1),
                ("h1", m["h"], 1, target.h1, 1), ("act", m["act"], 0, target.acts, T), ("rew", m["rew"], 0, target.rews, T),
                ("done", m["done"], 0, target.dones, T)]

    def gather(self, idx: th.Tensor, enc: str = "gnn", time_batched: bool = True) -> Dict:
        """Batch dict in the layout ``MultiAgentQLearner.loss`` consumes (one agent per environment): obs = T+1 `seen-by`
        HeteroBatch of B environments (enc='gnn') or T+1 [B, 2+4M] tensors (enc='rnn'), h0 / h1 [B, H], acts / rews / dones
        [T, B, 1].  The observation fields are gathered TIME-MAJOR in the one copy of the gather, so every step is a view.
        time_batched: also obs_all / obs_all_next - all T+1 steps (the steps from 1 on) as ONE batch of (T+1) B ((T) B) environments,
        views of the same gather - which switch on the learner's time-batched encoder and sequence-level recurrence."""
        if enc not in ("gnn", "rnn"):
            raise ValueError(f"enc must be 'gnn' or 'rnn', got {enc!r}")
        B = idx.numel()
        gt = self.mem["gt"].transpose(0, 1).index_select(1, idx)              # [T+1, B, M, 4]
        agent = self.mem["agent"].transpose(0, 1).index_select(1, idx)        # [T+1, B, 2]
        h = self.mem["h"][:, :2].index_select(0, idx)
        out = dict(h0=h[:, 0].contiguous(), h1=h[:, 1].contiguous(),
                   acts=self.mem["act"].index_select(0, idx).transpose(0, 1).contiguous(),
                   rews=self.mem["rew"].index_select(0, idx).transpose(0, 1).contiguous(),
                   dones=self.mem["done"].index_select(0, idx).transpose(0, 1).contiguous())
        T1 = self.T + 1
        if enc == "gnn":
            out["obs"] = [from_single_ubs_obs(gt[t], agent[t]) for t in range(T1)]
            if time_batched:
                out["obs_all"] = from_single_ubs_obs(gt.view(T1 * B, self.M, -1), agent.view(T1 * B, -1))
                out["obs_all_next"] = from_single_ubs_obs(gt[1:].view(self.T * B, self.M, -1), agent[1:].view(self.T * B, -1))
        else:
            flat = th.cat((agent, gt.reshape(T1, B, -1)), 2)                  # [T+1, B, 2+4M]
            out["obs"] = [flat[t] for t in range(T1)]
            if time_batched:
                out["obs_all"] = flat.view(T1 * B, -1)
                out["obs_all_next"] = flat[1:].view(self.T * B, -1)
        return out

    def sample(self, batch_size: int, generator: Optional[th.Generator] = None, enc: str = "gnn", time_batched: bool = True) -> Dict:
        return self.gather(self.sample_indices(batch_size, generator), enc, time_batched)
