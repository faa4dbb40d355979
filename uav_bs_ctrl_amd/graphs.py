"""hipGraph capture of the rollout step and of the whole update.

At the reference's own operating point - ONE environment per ``act`` and 32 sequences of T = 50 steps per ``update``
(algos/madrqn/learner.py:69-80,:94-173; run.py:55-57) - the path is launch-bound: an ``act`` is ~20 kernels of a few
microseconds each and an ``update`` ~3000.  Every kernel of the path takes an explicit stream, allocates nothing and
keeps no state (include/uavgnn.h), the device-side graph builder has a ``static`` mode without a host round trip, the
exploration rate / learning rate / Adam step count live in device memory, and the update's tail is one launch
(uav_bs_ctrl_amd/optim.py) - so both calls capture into ``torch.cuda.CUDAGraph`` (hipGraph on ROCm) and replay from
fixed-address input buffers.  Same arithmetic as the eager calls, kernel for kernel.

With the replay's ring position, its sampler and the exploration schedule on the device (``replay`` with ``device_state=True``,
csrc/replay.hip) the loop that ties the calls together captures too: ``GraphedEpisode`` replays a whole training episode - reset, rollout,
caching, commits, sampling, gathers, updates - as one graph (``Episode``: the same launches, eager).  ``Evaluation`` /
``GraphedEvaluation`` are the reference's ``test_agent()`` on a separate evaluation simulator with their own device random state, and
``stats=`` (``stats.EpochStats``) keeps the epoch's log row on the device.

Every class here captures through ONE routine, ``_warm_up_and_capture``: snapshot, warm-up on a side stream, capture into a ``_Window``
(one graph, or several in one pool when the body cuts it at a collective), snapshot back.  What a class restores, whether it
synchronises or empties the weight-plane store before the window opens and whether the learner's generator is registered are
arguments at its call.  The epsilon-greedy launch of all of them is ``_select``.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch as th

from . import _lib as L
from . import ops
from .graph import from_padded_obs, from_padded_obs_flat, from_single_ubs_obs


def _builder(enc: str):
    """Device builder of the observation batches: graphs ('gnn', exp3) or flattened observations ('mlp', exp2)."""
    if enc not in ("gnn", "mlp"):
        raise ValueError(f"enc must be 'gnn' or 'mlp', got {enc!r}")
    return from_padded_obs_flat if enc == "mlp" else from_padded_obs


def _capture(graph, **kw):
    """``torch.cuda.graph`` for this module's captures.  With a process group alive the capture runs in THREAD-LOCAL error mode:
    ProcessGroupNCCL's watchdog thread polls the events of the collectives issued so far (``hipEventQuery``), and under the default
    global mode a query that lands inside another thread's capture window is an error - "operation not permitted when stream is
    capturing" - that terminates the process (seen once in ~8 runs of the world-size-1 RCCL test of ``GraphedUpdate``, whose warm-up
    updates leave all-reduces for the watchdog to retire).  Thread-local mode restricts the check to the capturing thread, which
    issues nothing but this library's launches."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        kw.setdefault("capture_error_mode", "thread_local")
    return th.cuda.graph(graph, **kw)


class _RngSnapshot:
    """The random state a warm-up advances besides the parameters: the learner's epsilon generator and the device {seed, step} pairs
    of DiscreteComm's in-kernel noise (``rng_state``).  Restored after the capture, so a graphed run starts from the state an eager
    run starts from.  (A generator registered with a capturing graph keeps its captured offset bookkeeping; only its state before
    the first replay is put back.)"""

    def __init__(self, learner):
        self.learner = learner
        self.gen = learner._gen.get_state()
        self.comm = [(m, m.rng_state.clone()) for net in (learner.policy_net, learner.target_net) for m in net.modules()
                     if isinstance(getattr(m, "rng_state", None), th.Tensor)]

    def restore(self):
        self.learner._gen.set_state(self.gen)
        for m, st in self.comm:
            m.rng_state.copy_(st)


class _Window:
    """The capture window of ``_warm_up_and_capture``: ``graphs``, the last of which is the one being captured while ``open``.  A body
    that holds a collective calls ``cut()`` where the collective belongs: the open graph ends there and the next one begins, in
    the first one's memory pool, so the collective can be issued eagerly between two replays.  gen: a generator every graph of the
    window registers (the epsilon draws of ``th.rand``); None: none is registered."""

    def __init__(self, gen=None):
        self.gen, self.graphs, self._ctx = gen, [], None
        self._add()              # the first graph exists (and knows the generator) before the warm-up runs

    def _add(self):
        graph = th.cuda.CUDAGraph()
        if self.gen is not None and hasattr(graph, "register_generator_state"):
            graph.register_generator_state(self.gen)
        self.graphs.append(graph)

    @property
    def open(self) -> bool:
        return self._ctx is not None

    def __enter__(self):
        self._ctx = _capture(self.graphs[-1], **({"pool": self.graphs[0].pool()} if len(self.graphs) > 1 else {}))
        self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        ctx, self._ctx = self._ctx, None
        return ctx.__exit__(*exc)

    def cut(self):
        self.__exit__(None, None, None)
        self._add()
        self.__enter__()


def _warm_up_and_capture(warmup: int, body, window: _Window, captured=None, *, learner=None, state=None, sync: bool = False,
                         flush: bool = False):
    """The capture protocol of this module, once.  ``body`` runs ``warmup`` times for real on a side stream (allocator pools, lazy
    kernels, plane caches), then ``captured`` (default: ``body``) runs once inside ``window`` - ``_capture`` on the current stream, no
    fork or second stream inside it - and its value is returned.  What the warm-up moved is put back afterwards, so a graphed run
    starts from the state an eager run starts from:

    learner: its ``state_tensors()`` (after ``sync_lr()``: a learning rate the scheduler moved since the last sync is part of the
        snapshot, not undone by it), its random state (``_RngSnapshot``) and, at the end, its weight-plane store (emptied: the
        planes in it were split from the warm-up's parameters).
    state: further tensors to clone before the warm-up and copy back after the capture.
    Neither (None, None): nothing is restored and the device is not synchronised after the capture.
    sync: synchronise before the window opens - collectives ran in the warm-up and must be complete.
    flush: empty the learner's weight-plane store before the window opens, so that the graph holds the launches that build the planes
        (whether it does changes the graph's node list)."""
    restore = learner is not None or state is not None
    state = list(state or ())
    if learner is not None:
        learner.optimizer.sync_lr()
        state = learner.state_tensors() + state
    snap = [t.clone() for t in state]
    rng = None if learner is None else _RngSnapshot(learner)
    side = th.cuda.Stream()
    side.wait_stream(th.cuda.current_stream())
    with th.cuda.stream(side):
        for _ in range(warmup):
            body()
    th.cuda.current_stream().wait_stream(side)
    if flush:
        learner.invalidate_weight_cache()
    if sync:
        th.cuda.synchronize()
    with window:
        out = (captured or body)()
    if restore:
        th.cuda.synchronize()
        for dst, src in zip(state, snap):
            dst.copy_(src)
        if learner is not None:
            rng.restore()
            learner.invalidate_weight_cache()
    return out


def _select(learner, logits: th.Tensor, eps: th.Tensor, pair: Optional[th.Tensor] = None) -> th.Tensor:
    """Epsilon-greedy actions [N] int64 from ``logits`` [N, A] with the exploration rate in device memory (``eps``: float32 [1]): one
    exploration draw per team of ``learner.n_agents`` rows, first maximum (learner.py:75-78).  pair: a device int64 {seed, step} -
    the uniforms are drawn inside the kernel and the step advances by one (uavgnn_eps_greedy_philox); None - they come from
    ``learner._gen``, one per team and one per row in ONE generator call (uavgnn_eps_greedy_dev)."""
    N = logits.shape[0]
    acts = th.empty(N, dtype=th.int64, device=learner.device)
    logits = logits if logits.stride(1) == 1 else logits.contiguous()
    if pair is not None:
        L.check(L.lib().uavgnn_eps_greedy_philox(logits.data_ptr(), logits.stride(0), N, learner.n_actions, learner.n_agents,
                                                 pair.data_ptr(), eps.data_ptr(), 0.0, acts.data_ptr(), L.stream()),
                "uavgnn_eps_greedy_philox")
    else:
        teams = N // learner.n_agents
        u = th.rand(teams + N, device=learner.device, generator=learner._gen)
        L.check(L.lib().uavgnn_eps_greedy_dev(logits.data_ptr(), logits.stride(0), N, learner.n_actions, learner.n_agents,
                                              u.data_ptr(), u.data_ptr() + 4 * teams, eps.data_ptr(), acts.data_ptr(), L.stream()),
                "uavgnn_eps_greedy_dev")
    return acts


class _PaddedObs:
    """Fixed-address padded observation buffers (the simulator's format, mubs_cov.py:215-242) of ``lead`` env steps."""

    def __init__(self, lead, n, M, device, with_comm=True):
        f = dict(dtype=th.float32, device=device)
        self.gt = th.zeros(*lead, n, M, 5, **f)
        self.ubs = th.zeros(*lead, n, max(n - 1, 0), 3, **f)
        self.agent = th.zeros(*lead, n, 2, **f)
        self.d_u2u = th.zeros(*lead, n, n, **f) if with_comm else None

    def load(self, gt, ubs, agent, d_u2u=None):
        self.gt.copy_(gt, non_blocking=True)
        self.ubs.copy_(ubs, non_blocking=True)
        self.agent.copy_(agent, non_blocking=True)
        if self.d_u2u is not None:
            self.d_u2u.copy_(d_u2u, non_blocking=True)


class _GraphedActBase:
    """What the captured rollout steps share: the capture of ``_body`` with the learner's generator registered, the epsilon-greedy
    selection from device-resident epsilon, and the replay.  A subclass sets ``learner``, ``B`` (teams), ``h_in`` and
    its observation buffers, defines ``_obs()`` (the observation batch built from those buffers) and calls ``_capture_act``."""

    def _capture_act(self, warmup: int):
        learner = self.learner
        self.eps = th.zeros(1, dtype=th.float32, device=learner.device)
        self._eps_host = None
        window = _Window(learner._gen)
        # nothing is restored: a rollout step moves no parameter, and the warm-up's epsilon draws and comm noise steps stay advanced
        self.acts, self.h_out = _warm_up_and_capture(warmup, self._body, window)
        self.graph = window.graphs[0]

    @th.no_grad()
    def _body(self):
        with self.learner.rollout_noise():
            logits, h = self.learner.policy_net(self._obs(), self.h_in)
        return _select(self.learner, logits, self.eps), h

    def _replay(self, h, eps_thres: float):
        if h is not None and h.data_ptr() != self.h_in.data_ptr():
            self.h_in.copy_(h if h.shape[0] == self.h_in.shape[0] else h.expand_as(self.h_in), non_blocking=True)
        if eps_thres != self._eps_host:
            self.eps.copy_(th.tensor([eps_thres], dtype=th.float32), non_blocking=True)
            self._eps_host = eps_thres
        self.graph.replay()
        return self.acts, self.h_out


class GraphedAct(_GraphedActBase):
    """``learner.act`` on B environments as one graph replay: device-side graph construction from padded observations,
    no-grad policy forward, epsilon-greedy selection (one draw per team, learner.py:75-78).

        ga = GraphedAct(learner, B, n, M, r_comm)
        acts, h = ga(gt, ubs, agent, d_u2u, h, eps)        # acts [B*n] int64, h' [B*n, H]; both are the graph's buffers

    enc='mlp': flattened-observation batches (exp2) instead of observation graphs.
    """

    def __init__(self, learner, B: int, n: int, M: int, r_comm: float = float("inf"), warmup: int = 2, enc: str = "gnn"):
        self.learner, self.B, self.n, self.M, self.r_comm = learner, B, n, M, r_comm
        self._build = _builder(enc)
        dev = learner.device
        with_comm = learner.args.c is not None
        self.obs = _PaddedObs((B,), n, M, dev, with_comm)
        self.h_in = th.zeros(B * n, learner.args.hidden_size, dtype=th.float32, device=dev)
        self._capture_act(warmup)

    def _obs(self):
        return self._build(self.obs.gt, self.obs.ubs, self.obs.agent, self.obs.d_u2u, self.r_comm, static=True)

    def __call__(self, gt, ubs, agent, d_u2u, h, eps_thres: float):
        """Copies the observation into the graph's buffers and replays.  A producer that writes ``self.obs.gt / .ubs /
        .agent / .d_u2u`` and ``self.h_in`` in place (e.g. a device-side simulator) passes gt=None and skips the copies."""
        if gt is not None:
            self.obs.load(gt, ubs, agent, d_u2u)
        return self._replay(h, eps_thres)


def _single_ubs_enc(enc: str) -> str:
    if enc not in ("gnn", "rnn"):
        raise ValueError(f"enc must be 'gnn' or 'rnn', got {enc!r}")
    return enc


class GraphedSingleUbsAct(_GraphedActBase):
    """``QLearner.act`` on B single-UBS environments (experiment 1) as one graph replay: the `seen-by` batch as views of the
    observation fields (enc='gnn') or the flattened [B, 2+4M] rows filled by one copy inside the graph (enc='rnn'), no-grad policy
    forward, epsilon-greedy selection with one draw per environment (algos/drqn/learner.py:60-63).

        ga = GraphedSingleUbsAct(learner, B, M, enc, obs=(env.out["obs_gt"], env.out["obs_agent"]))
        acts, h = ga(None, None, h, eps)                   # acts [B] int64, h' [B, H]; both are the graph's buffers

    obs: (gt [B,M,4], agent [B,2]) fixed-address buffers somebody else writes - the simulator's own, so a rollout copies nothing;
    default: buffers of the graph, filled by ``__call__(gt, agent, h, eps)``."""

    def __init__(self, learner, B: int, M: int, enc: str = "gnn", obs=None, warmup: int = 2):
        self.learner, self.B, self.M, self.enc = learner, B, M, _single_ubs_enc(enc)
        dev = learner.device
        f = dict(dtype=th.float32, device=dev)
        if obs is None:
            self.gt, self.agent = th.zeros(B, M, 4, **f), th.zeros(B, 2, **f)
        else:
            self.gt, self.agent = obs
            if tuple(self.gt.shape) != (B, M, 4) or tuple(self.agent.shape) != (B, 2) or not (self.gt.is_contiguous()
                                                                                            and self.agent.is_contiguous()):
                raise ValueError(f"obs: contiguous gt [{B},{M},4] and agent [{B},2] expected, got {tuple(self.gt.shape)} / "
                                 f"{tuple(self.agent.shape)}")
        self.flat = th.zeros(B, 2 + 4 * M, **f) if enc == "rnn" else None
        self.h_in = th.zeros(B, learner.args.hidden_size, **f)
        self._capture_act(warmup)

    def _obs(self):
        if self.enc == "rnn":
            return th.cat((self.agent, self.gt.view(self.B, -1)), 1, out=self.flat)
        return from_single_ubs_obs(self.gt, self.agent)

    def __call__(self, gt, agent, h, eps_thres: float):
        """gt=None: the observation buffers were written in place (the simulator's buffers handed over as ``obs``)."""
        if gt is not None:
            self.gt.copy_(gt, non_blocking=True)
            self.agent.copy_(agent, non_blocking=True)
        return self._replay(h, eps_thres)


class _GraphedUpdateBase:
    """What the captured updates share: the capture of ``learner.update(self._batch())`` - the learner's state restored after the
    warm-up updates, the window cut at the gradient all-reduce into two graphs when ``learner.needs_collective()`` - the replay and
    ``load_from``.  A subclass sets ``learner`` and its fixed-address input buffers, defines ``_batch()`` / ``load(m)`` and calls
    ``_capture_update``."""

    def _capture_update(self, warmup: int):
        learner = self.learner
        assert learner.fused_tail, "graph capture needs the device-resident update tail (CUDA learner)"
        self.split = learner.needs_collective()
        window = _Window()               # the generator is not registered: an update draws nothing from it

        def cut_body():                  # the update without its collective: `accumulate` | `apply`
            out = learner.accumulate(self._batch())
            window.cut()
            learner.apply()
            return out
        # the weight-plane store is not emptied before the window: the planes are built inside `accumulate`'s own store either way
        self.out = _warm_up_and_capture(warmup, self._body, window, cut_body if self.split else None, learner=learner, sync=self.split)
        self.graph = window.graphs[0]
        if self.split:
            self.graph_tail = window.graphs[1]

    def _body(self) -> Dict:
        return self.learner.update(self._batch())

    def _bind_weights(self, weights: Optional[th.Tensor], T: int, B: int, C: int) -> None:
        """``weights`` [B] (None: the update is not prioritised) and the TD buffer ``td`` [T, B, C] the loss writes into.  A learner with
        multi-step targets (``learner.returns``) needs nothing more of a captured update: its kernel writes ``td`` itself (no copy), the
        partial sums of its loss live in the learner's own per-shape workspace, allocated by the warm-up before the capture, and the
        gradient buffer in the capture's pool - fixed addresses all."""
        self.weights, self.td = weights, None
        if weights is None:
            return
        if tuple(weights.shape) != (B,) or weights.dtype != th.float32 or not weights.is_contiguous() or weights.device != self.h0.device:
            raise ValueError(f"weights: a contiguous float32 [{B}] tensor on the learner's device expected")
        self.td = th.zeros(T, B, C, dtype=th.float32, device=weights.device)

    def load_from(self, replay, idx: th.Tensor) -> None:
        """The sequences ``idx`` of a device-state replay straight from its ring into the graph's buffers: ONE gather launch
        (``replay.gather_into``) instead of one ``index_select`` and one copy per field.  Same bits as ``load``."""
        replay.gather_into(idx, self)

    def __call__(self, m: Optional[Dict[str, th.Tensor]] = None) -> Dict:
        if m is not None:
            self.load(m)
        self.learner.optimizer.sync_lr()
        self.graph.replay()
        if self.split:
            self.learner.grads.all_reduce_mean_(self.learner.group)
            self.graph_tail.replay()
        self.learner.invalidate_weight_cache()   # the replay moved the parameters without passing through learner.apply()
        return self.out


class GraphedUpdate(_GraphedUpdateBase):
    """``learner.update`` on B stored sequences of T transitions as one graph replay: graphs of all T+1 steps rebuilt on
    the device from the padded observations of the sampled batch (``SequenceReplay.mem`` layout), time-batched encoder,
    2T+1 forwards, BPTT backward, clip + AdamW + polyak.

        gu = GraphedUpdate(learner, B, T, n, M, r_comm)
        out = gu(batch)      # batch: gt [B,T+1,n,M,5], ubs, agent, d_u2u, h [B,T+1,n,H], act [B,T,n], rew [B,T,rd], done [B,T,1]
                             # with learner.mixer (QMIX): also state [B,T+1,state_dim] -> ``self.states`` [T+1,B,state_dim], rd = 1

    Data-parallel runs (``learner.needs_collective()``): the gradient all-reduce is NOT captured.  The update is cut at
    its only collective into TWO graphs - ``accumulate`` (graph construction, 2T+1 forwards, backward into the flat gradient
    buffer) and ``apply`` (clip + AdamW + polyak) - with the RCCL all-reduce of the flat buffer issued eagerly on the same
    stream between the two replays: the capture never depends on what the communicator does under stream capture, and a
    rank that replays while another is still capturing cannot dead-lock inside a captured collective.
    """

    def __init__(self, learner, B: int, T: int, n: int, M: int, r_comm: float = float("inf"), rew_dim: Optional[int] = None,
                 warmup: int = 2, enc: str = "gnn", capture: bool = True, weights: Optional[th.Tensor] = None):
        """capture=False: only the fixed-address buffers, ``_batch()`` and ``load`` / ``load_from`` - for a larger capture that holds the
        update itself (``GraphedEpisode``).  weights: the fixed-address importance weights [B] of a prioritised replay (its
        ``is_weights``, shared) - the batch then carries them and the loss leaves its TD errors in ``td`` [T, B, n] ([T, B, 1] with a
        mixer); None: neither exists."""
        assert learner.fused_tail, "graph capture needs the device-resident update tail (CUDA learner)"
        self.learner, self.B, self.T, self.n, self.M, self.r_comm = learner, B, T, n, M, r_comm
        self._build = _builder(enc)      # enc='mlp': flattened-observation batches (exp2)
        dev, H = learner.device, learner.args.hidden_size
        rd = n if rew_dim is None else rew_dim
        # time-major: step t of every sequence is contiguous.  enc='mlp' without communication (RnnAgent) reads no talk relation
        self.obs = _PaddedObs((T + 1, B), n, M, dev, enc == "gnn" or learner.args.c is not None)
        self.h0 = th.zeros(B * n, H, dtype=th.float32, device=dev)
        self.h1 = th.zeros(B * n, H, dtype=th.float32, device=dev)
        self.acts = th.zeros(T, B * n, 1, dtype=th.int64, device=dev)
        self.rews = th.zeros(T, B, rd, dtype=th.float32, device=dev)
        self.dones = th.zeros(T, B, 1, dtype=th.float32, device=dev)
        # QMIX (learner.py:145-148): the global state of all T+1 steps; None without a mixer (``SequenceReplay._gather_fields`` looks here)
        mixer = getattr(learner, "mixer", None)
        self.states = None if mixer is None else th.zeros(T + 1, B, mixer.state_dim, dtype=th.float32, device=dev)
        self._bind_weights(weights, T, B, n if mixer is None else 1)
        if capture:
            self._capture_update(warmup)

    def _batch(self) -> Dict:
        T, B, n, M = self.T, self.B, self.n, self.M
        o = self.obs
        build = self._build
        obs = [build(o.gt[t], o.ubs[t], o.agent[t], None if o.d_u2u is None else o.d_u2u[t], self.r_comm, static=True)
               for t in range(T + 1)]
        flat = lambda x, lo: x[lo:].reshape(((x.shape[0] - lo) * x.shape[1],) + x.shape[2:])  # noqa: E731  (no -1: ubs is empty at n = 1)
        obs_all = build(flat(o.gt, 0), flat(o.ubs, 0), flat(o.agent, 0), None, self.r_comm, static=True)
        obs_next = build(flat(o.gt, 1), flat(o.ubs, 1), flat(o.agent, 1), None, self.r_comm, static=True)
        out = dict(obs=obs, obs_all=obs_all, obs_all_next=obs_next, h0=self.h0, h1=self.h1, acts=self.acts,
                   rews=self.rews, dones=self.dones)
        if self.states is not None:
            out["states"] = self.states
        if self.weights is not None:
            out.update(weights=self.weights, td_out=self.td)
        return out

    def load(self, m: Dict[str, th.Tensor]) -> None:
        """m: a gathered batch in ``SequenceReplay.mem`` layout (leading dims [B, T+1] / [B, T]; ``state`` [B, T+1, state_dim] with a mixer)."""
        B, T, n = self.B, self.T, self.n
        self.obs.load(m["gt"].transpose(0, 1), m["ubs"].transpose(0, 1), m["agent"].transpose(0, 1),
                      m["d_u2u"].transpose(0, 1))
        self.h0.copy_(m["h"][:, 0].reshape(B * n, -1), non_blocking=True)
        self.h1.copy_(m["h"][:, 1].reshape(B * n, -1), non_blocking=True)
        self.acts.copy_(m["act"].permute(1, 0, 2).reshape(T, B * n, 1), non_blocking=True)
        self.rews.copy_(m["rew"].permute(1, 0, 2), non_blocking=True)
        self.dones.copy_(m["done"].permute(1, 0, 2), non_blocking=True)
        if self.states is not None:
            self.states.copy_(m["state"].transpose(0, 1), non_blocking=True)


class GraphedSingleUbsUpdate(_GraphedUpdateBase):
    """``QLearner.update`` on B stored sequences of T transitions of the single-UBS environment (experiment 1) as one graph replay:
    the batch ``SingleUbsSequenceReplay.gather`` builds - T+1 per-step observation batches plus the time-batched ones, all views of
    the graph's fixed-address buffers - then the update (time-batched encoder, recurrence, BPTT backward, clip + AdamW + polyak).

        gu = GraphedSingleUbsUpdate(learner, B, T, M, enc)
        out = gu(m)       # m: gt [B,T+1,M,4], agent [B,T+1,2], h [B,T+1,H], act / rew / done [B,T,1] (``SingleUbsSequenceReplay.mem``)

    Data-parallel runs are cut at the gradient all-reduce exactly as ``GraphedUpdate`` is."""

    def __init__(self, learner, B: int, T: int, M: int, enc: str = "gnn", warmup: int = 2, capture: bool = True,
                 weights: Optional[th.Tensor] = None):
        """capture=False: only the fixed-address buffers, ``_batch()`` and ``load`` / ``load_from``; weights: the importance weights [B] of
        a prioritised replay, ``td`` [T, B, 1] then receives the TD errors (see ``GraphedUpdate``)."""
        self.learner, self.B, self.T, self.M, self.enc = learner, B, T, M, _single_ubs_enc(enc)
        dev, H = learner.device, learner.args.hidden_size
        f = dict(dtype=th.float32, device=dev)
        self.gt, self.agent = th.zeros(T + 1, B, M, 4, **f), th.zeros(T + 1, B, 2, **f)          # time-major, as `gather` lays them out
        self.flat = th.zeros(T + 1, B, 2 + 4 * M, **f) if enc == "rnn" else None
        self.h0, self.h1 = th.zeros(B, H, **f), th.zeros(B, H, **f)
        self.acts = th.zeros(T, B, 1, dtype=th.int64, device=dev)
        self.rews, self.dones = th.zeros(T, B, 1, **f), th.zeros(T, B, 1, **f)
        self._bind_weights(weights, T, B, 1)
        if capture:
            self._capture_update(warmup)

    def _batch(self) -> Dict:
        T, B, M = self.T, self.B, self.M
        out = dict(h0=self.h0, h1=self.h1, acts=self.acts, rews=self.rews, dones=self.dones)
        if self.weights is not None:
            out.update(weights=self.weights, td_out=self.td)
        if self.enc == "gnn":
            gt, agent = self.gt, self.agent
            out["obs"] = [from_single_ubs_obs(gt[t], agent[t]) for t in range(T + 1)]
            out["obs_all"] = from_single_ubs_obs(gt.view((T + 1) * B, M, 4), agent.view((T + 1) * B, 2))
            out["obs_all_next"] = from_single_ubs_obs(gt[1:].view(T * B, M, 4), agent[1:].view(T * B, 2))
        else:
            flat = th.cat((self.agent, self.gt.view(T + 1, B, -1)), 2, out=self.flat)       # the one copy (inside the graph)
            out["obs"] = [flat[t] for t in range(T + 1)]
            out["obs_all"] = flat.view((T + 1) * B, -1)
            out["obs_all_next"] = flat[1:].view(T * B, -1)
        return out

    def load(self, m: Dict[str, th.Tensor]) -> None:
        """m: a gathered batch in ``SingleUbsSequenceReplay.mem`` layout (leading dims [B, T+1] / [B, T])."""
        self.gt.copy_(m["gt"].transpose(0, 1), non_blocking=True)
        self.agent.copy_(m["agent"].transpose(0, 1), non_blocking=True)
        self.h0.copy_(m["h"][:, 0], non_blocking=True)
        self.h1.copy_(m["h"][:, 1], non_blocking=True)
        self.acts.copy_(m["act"].transpose(0, 1), non_blocking=True)
        self.rews.copy_(m["rew"].transpose(0, 1), non_blocking=True)
        self.dones.copy_(m["done"].transpose(0, 1), non_blocking=True)


class GraphedCycle:
    """A whole acting / training cycle on FIXED-ADDRESS inputs - e.g. T ``learner.act`` calls on stored graphs followed by one
    ``learner.update`` - as one graph replay.  For batches of a few thousand agents (BASELINE config 2: 4 x 40, B = 1024) the
    ~4000 launches of a cycle are 5-20 us each and the launch thread, not the device, sets the pace; the replay removes the gaps.

        cyc = GraphedCycle(learner, body)      # body(): learner calls only, every input at a fixed device address, no host
        out = cyc()                            # round trip; returns body()'s value (the graph's own buffers)

    ``body`` runs ``warmup`` times for real before the capture (allocator pools, lazy kernels, plane caches); parameters,
    target and optimiser state are restored afterwards.  Single-process only: a data-parallel update holds a
    collective (``GraphedUpdate`` cuts the capture there).  The learning rate is pushed to the device before each replay
    and the rollout's weight-plane store is emptied after it (the replay moved the parameters without passing through
    ``learner.apply``)."""

    def __init__(self, learner, body, warmup: int = 2):
        assert learner.fused_tail, "graph capture needs the device-resident update tail (CUDA learner)"
        assert not learner.needs_collective(), "a data-parallel update cannot be captured whole: use GraphedUpdate"
        self.learner, self.body = learner, body
        window = _Window(learner._gen)
        # flush: `learner.act` calls in `body` keep their planes in the learner's store, and the graph must hold the launches that build them
        self.out = _warm_up_and_capture(warmup, body, window, learner=learner, flush=True)
        self.graph = window.graphs[0]

    def __call__(self):
        self.learner.optimizer.sync_lr()
        self.graph.replay()
        self.learner.invalidate_weight_cache()
        return self.out


INFO_KEYS = ("EpRet", "EpLen", "AvgGlobalUtility", "TotalThroughput", "FairIdx", "ProbCollision")


def info_keys(single: bool):
    """The statistics ``env.step`` returns (run.py:93 ``logger.store(**info)``; ProbCollision: the multi-UBS simulator only)."""
    return INFO_KEYS[:-1] if single else INFO_KEYS


class _EnvObs:
    """Which device simulator an episode or an evaluation runs on, decided once by ``_bind_env``: ``single`` (experiment 1), ``keys``
    (its info keys), ``_reset`` (its reset on the device) and, for the multi-UBS simulator, ``_build`` / ``with_comm``; ``_obs()`` is
    the policy's observation batch straight from its output buffers.  ``env.reset_rng`` is the reset counter of either."""

    def _bind_env(self, learner, env, enc: str) -> None:
        from .sim import BatchedSingleUbsCoverageEnv
        self.env, self.enc = env, enc
        self.single = isinstance(env, BatchedSingleUbsCoverageEnv)
        self.keys = info_keys(self.single)
        if self.single:
            _single_ubs_enc(enc)
            self._reset = env.reset
        else:
            self._build = _builder(enc)
            if env.spec is None:
                raise ValueError("env: an environment with a map expected (BatchedUbsCoverageEnv.from_map): the reset draws on the device")
            self.with_comm = learner.args.c is not None
            self._reset = env.reset_from_map

    def _obs(self):
        o = self.env.out
        if self.single:
            return o["obs_flat"] if self.enc == "rnn" else from_single_ubs_obs(o["obs_gt"], o["obs_agent"])
        return self._build(o["obs_gt"], o["obs_ubs"], o["obs_agent"], o["d_u2u"] if self.with_comm else None, self.env.p.r_comm,
                           static=True)


class Episode(_EnvObs):
    """One whole training episode of the device loop with NO host state in it (run.py:81-99 for E parallel environments): the
    simulator's reset, then ``episode_limit / T`` segments of T rollout steps - ``stage_obs``, the exploration schedule on the device
    (uavgnn_eps_schedule: epsilon from a device counter of environment interactions, +E per step), the policy forward and
    uavgnn_eps_greedy_dev, ``env.step``, ``learner.cache(..., staged=True)`` - whose last ``cache`` commits the E sequences into the
    ring; when ``train``, ``updates_per_segment`` x (sample, gather, ``learner.update``) follow each commit.  Ring position, sampler
    counter, exploration counter and the simulator's reset counter are all read on the device, and the per-step writes into the
    sequences under construction walk the fixed sequence ptr = 0 .. T-1, so the same launches serve every episode: ``Episode`` runs
    them eagerly, ``GraphedEpisode`` replays them as one graph.

        ep = Episode(learner, env, replay, batch_size, eps=(1.0, 0.05, 5e4))       # replay: device_state=True, n_envs = env.B
        out = ep()                 # {LossQ, QVals} of the last update (None when train=False); env's info tensors hold the statistics

    env: ``BatchedUbsCoverageEnv.from_map(...)`` with enc 'gnn' / 'mlp' (exp3 / exp2) or ``BatchedSingleUbsCoverageEnv`` with enc
    'gnn' / 'rnn' (exp1).  ``idx`` keeps the last sampled batch, ``eps`` / ``t`` the exploration rate and its counter.
    A learner with ``mixer=True`` (QMIX) trains here as well: the replay must store the simulator's ``state`` at the mixer's width and ONE
    shared reward (``state_dim=env.state_dim, rew_dim=1``, ``args.share_reward``), else ``ValueError``.
    replay: a ``replay.CompactSequenceReplay`` (built ``for_env(env, ...)``) instead stages ``env.replay_state()`` and the hidden state at
    every step and rebuilds observations and the mixer's state in its gather; it needs no stored ``state``, only ``rew_dim=1`` under QMIX.

    replay: built with ``prioritized=(alpha, beta, eta, eps)`` - every update is draw (proportional to priority), gather, ``learner.update``
    on a batch that carries the draw's importance weights (``replay.is_weights``, shared with the update's buffer: no copy), then
    ``replay.update_priorities(idx, upd.td)`` with the TD errors the loss left - after ``apply``, so with ``updates_per_segment > 1`` the
    next draw already sees the new priorities.

    stats: a ``stats.EpochStats`` holding the info keys (EpRet, EpLen, AvgGlobalUtility, TotalThroughput, FairIdx, and ProbCollision for
    the multi-UBS simulator) and, when ``train``, LossQ: the body pushes the info tensors once at the end of the episode and LossQ after
    every update (run.py:93, :99) - launches on fixed addresses, so they replay with the graph.  None: nothing is pushed.

    explore_seed: None - the uniforms of the selection come from ``learner._gen`` (``th.rand`` + uavgnn_eps_greedy_dev).  An integer - the
    selection is uavgnn_eps_greedy_philox (the same rule: one exploration draw per team, first maximum) with the schedule's device ``eps``
    and the uniforms drawn inside the kernel from ``explore``, a device int64 {seed, step} pair of this object that advances by one per
    step: the random state of the exploration is a plain tensor that can be saved, restored and handed from one episode object to another
    by value (``b.explore.copy_(a.explore)``), and ``learner._gen`` is never touched."""

    def __init__(self, learner, env, replay, batch_size: int, eps=(1.0, 0.05, 5e4), train: bool = True,
                 updates_per_segment: int = 1, enc: str = "gnn", stats=None, explore_seed: Optional[int] = None):
        assert learner.fused_tail, "the device loop needs the device-resident update tail (CUDA learner)"
        self.learner, self.replay, self.batch_size = learner, replay, int(batch_size)
        self.train, self.updates_per_segment = bool(train), int(updates_per_segment)
        if not getattr(replay, "device_state", False):
            raise ValueError("replay: a device-state replay expected (device_state=True)")
        if replay.n_envs != env.B:
            raise ValueError(f"replay.n_envs = {replay.n_envs} but the simulator runs {env.B} environments")
        if replay.ptr != 0:
            raise ValueError("replay: a sequence is under construction (ptr != 0)")
        self.T, self.E = replay.T, env.B
        if env.episode_limit % self.T != 0:
            raise ValueError(f"episode_limit = {env.episode_limit} is no multiple of the sequence length T = {self.T}")
        if self.updates_per_segment < 1:
            raise ValueError("updates_per_segment must be at least 1")
        self.segments = env.episode_limit // self.T
        self.eps_start, self.eps_end, self.decay_steps = (float(v) for v in eps)
        if not self.decay_steps > 0:
            raise ValueError("eps = (start, end, decay_steps): decay_steps must be positive")
        dev = learner.device
        self._bind_env(learner, env, enc)
        self.compact = False
        # a prioritised ring: the update reads the draw's importance weights where the sampler leaves them (one tensor, no copy)
        self.prioritized = getattr(replay, "prioritized", None) is not None
        weights = replay.reserve_batch(self.batch_size) if self.prioritized and self.train else None
        if self.single:
            self.upd = GraphedSingleUbsUpdate(learner, self.batch_size, self.T, env.n_gts, enc, capture=False,
                                              weights=weights) if self.train else None
        else:
            from .replay import CompactSequenceReplay
            # a compact ring stores the simulator's state, not its observations: nothing of `state` is staged, the gather rebuilds it
            self.compact = isinstance(replay, CompactSequenceReplay)
            self.with_state = not self.compact and replay.mem["state"].shape[-1] > 0
            if getattr(learner, "mixer", None) is not None:      # QMIX: q_tot is one value per environment, mixed from the stored global state
                sd, rd = replay.state_dim if self.compact else replay.mem["state"].shape[-1], replay.mem["rew"].shape[-1]
                if sd != learner.mixer.state_dim:
                    raise ValueError(f"replay: the mixer reads a state of width {learner.mixer.state_dim} but the replay stores "
                                     f"state_dim = {sd}")
                if rd != 1:
                    raise ValueError(f"replay: the mixer's q_tot is one value per environment (share_reward) but the replay stores "
                                     f"rew_dim = {rd}")
            self.upd = GraphedUpdate(learner, self.batch_size, self.T, env.n_agents, env.n_gts, env.p.r_comm,
                                     replay.mem["rew"].shape[-1], enc=enc, capture=False, weights=weights) if self.train else None
        # built here, outside any capture: init_hidden moves a CPU row to the device, the scalars below are host-to-device copies
        self.h_zero = learner.init_hidden(self.E)
        self.eps = th.full((1,), self.eps_start, dtype=th.float32, device=dev)
        self.t = th.zeros(1, dtype=th.int64, device=dev)
        self.explore = None if explore_seed is None else th.tensor([int(explore_seed), 0], dtype=th.int64, device=dev)
        self.idx: Optional[th.Tensor] = None
        self.out: Optional[Dict] = None
        self.stats, self.info = stats, None
        if stats is not None:
            missing = [k for k in self.keys + (("LossQ",) if self.train else ()) if k not in stats.index]
            if missing:
                raise ValueError(f"stats: keys {missing} are missing")

    @th.no_grad()
    def _step(self, h: th.Tensor) -> th.Tensor:
        lr, env, rb, E = self.learner, self.env, self.replay, self.E
        o = env.observations()
        if self.single:
            rb.stage_obs(dict(gt=o["gt"], agent=o["agent"], h=h))
        elif self.compact:
            rb.stage_obs(dict(env.replay_state(), h=h.view(E, lr.n_agents, -1)))
        else:
            staged = dict(gt=o["gt"], ubs=o["ubs"], agent=o["agent"], d_u2u=o["d_u2u"], h=h.view(E, lr.n_agents, -1))
            if self.with_state:
                staged["state"] = o["state"]
            rb.stage_obs(staged)
        L.check(L.lib().uavgnn_eps_schedule(self.t.data_ptr(), E, self.eps_start, self.eps_end, self.decay_steps,
                                            self.eps.data_ptr(), L.stream()), "uavgnn_eps_schedule")
        with lr.rollout_noise():
            logits, h2 = lr.policy_net(self._obs(), h)
        acts = _select(lr, logits, self.eps, self.explore)
        o2, rew, done, info = env.step(acts)
        if self.single:
            lr.cache(rb, None, None, acts, rew, o2, h2, done, info["BadMask"], staged=True)
        elif self.compact:
            lr.cache(rb, None, None, None, acts, rew, env.replay_state(), h2, None, done, info["BadMask"], staged=True)
        else:
            st = o2["state"] if self.with_state else None      # `cache` stores next_state only when a state is given (staged: not read)
            lr.cache(rb, None, None, st, acts, rew, o2, h2, st, done, info["BadMask"], staged=True)
        self.info = info
        return h2

    def _update(self, batch) -> Dict:
        """One gradient step of the body.  Data-parallel: ``learner.update`` holds the run's only collective, the all-reduce of the flat
        gradient buffer between ``accumulate`` and ``apply`` - the one place ``GraphedEpisode`` cuts its capture."""
        return self.learner.update(batch)

    def _body(self) -> Optional[Dict]:
        rb = self.replay
        self._reset()
        h, out = self.h_zero, None
        for _ in range(self.segments):
            with ops.frozen_weights():        # nothing moves a parameter inside a segment's rollout: weight planes are split once
                for _ in range(self.T):
                    h = self._step(h)
            assert rb.ptr == 0, "the segment did not end on a commit"
            if self.train:
                for _ in range(self.updates_per_segment):
                    self.idx = rb.sample_indices(self.batch_size)
                    rb.gather_into(self.idx, self.upd)
                    out = self._update(self.upd._batch())
                    if self.prioritized:          # after `apply`: the next draw of this segment already sees the new priorities
                        rb.update_priorities(self.idx, self.upd.td)
                    if self.stats is not None:
                        self.stats.push(LossQ=out["LossQ"])
        if self.stats is not None:
            self.stats.push(**{k: self.info[k] for k in self.keys})
        return out

    def __call__(self) -> Optional[Dict]:
        self.out = self._body()
        return self.out


class GraphedEpisode(Episode):
    """``Episode`` as ONE graph replay: reset, every rollout step, caching, commits, sampling, gathers and updates of a whole episode
    without host work in between (at the reference's batch sizes the loop is launch-bound: ~20 launches per ``act``, ~3000 per
    ``update``).

        ge = GraphedEpisode(learner, env, replay, batch_size, eps=(1.0, 0.05, 5e4), train=True, enc="gnn")
        out = ge()                 # replays; the last update's {LossQ, QVals} (the graph's buffers), env.step's info tensors updated
        replay.check()             # now and then: raises when a batch was sampled from fewer sequences than it holds

    train=False: the collect-only graph for the steps before ``update_after``.  The body runs ``warmup`` times for real before the
    capture; parameters, target, optimiser state, the random state (``_RngSnapshot``), the replay's ``state`` / ``rng`` / ``status``,
    the exploration counter, the exploration pair of ``explore_seed``, the simulator's reset counter and the accumulator of ``stats`` are
    restored afterwards, so a graphed run starts where an eager one starts (the ring ROWS the warm-up wrote stay, beyond ``size``, where
    nothing samples them).  Captured on one stream without forks.  The learning rate is pushed to the device before each replay and the
    rollout's weight-plane store is emptied after it.

    Data-parallel runs (``learner.needs_collective()`` at construction, ``train=True``): the gradient all-reduce is NOT captured.  The body
    is cut at every update into ``segments * updates_per_segment + 1`` graphs that share the first one's memory pool (``graphs``) - rollout,
    commits, sample, gather and ``learner.accumulate`` | ``learner.apply``, the LossQ push, the next rollout ... up to the next
    ``accumulate`` | ... - and a call replays them in order with ``learner.grads.all_reduce_mean_(learner.group)`` issued eagerly on the
    same stream between two pieces (``collectives_per_replay`` of them), as ``GraphedUpdate`` does for one update.  The warm-up episodes
    run their collectives eagerly, so every rank must construct the object at the same point of its program.  Without a collective, and
    with ``train=False`` (no update), the episode is ONE graph: ``graphs == [graph]``."""

    def __init__(self, learner, env, replay, batch_size: int, eps=(1.0, 0.05, 5e4), train: bool = True,
                 updates_per_segment: int = 1, enc: str = "gnn", warmup: int = 2, stats=None, explore_seed: Optional[int] = None):
        super().__init__(learner, env, replay, batch_size, eps, train, updates_per_segment, enc, stats, explore_seed)
        collective = learner.needs_collective()
        self.split = self.train and collective
        self.collectives_per_replay = self.segments * self.updates_per_segment if self.split else 0
        self._window = _Window(learner._gen)           # every piece registers the generator
        self.graphs = self._window.graphs
        self.graph = self.graphs[0]
        state = [replay.state, replay.rng, replay.status, self.t, self.eps, env.reset_rng]
        if self.explore is not None:
            state.append(self.explore)
        if self.prioritized:                           # the warm-up's commits and priority updates are undone as well
            state += [replay.prio, replay.prio_max]
        if stats is not None:
            state += stats.state_tensors()             # the warm-up episodes' pushes are undone as well
        # flush: as GraphedCycle (the body's stores are its own, so nothing of the learner's store is read); sync: whenever the learner
        # holds a collective, also with train=False, whose warm-up ran none
        self.out = _warm_up_and_capture(warmup, self._body, self._window, learner=learner, state=state, sync=collective, flush=True)
        assert len(self.graphs) == self.collectives_per_replay + 1

    def _update(self, batch) -> Dict:
        if not (self.split and self._window.open):     # warm-up, or a run without a collective: the whole update
            return super()._update(batch)
        out = self.learner.accumulate(batch)
        self._window.cut()                 # this graph ends on the gradient, the next begins with `apply`
        self.learner.apply()
        return out

    def __call__(self) -> Optional[Dict]:
        self.learner.optimizer.sync_lr()
        self.graph.replay()
        for graph in self.graphs[1:]:      # data-parallel: the all-reduce of the flat gradient buffer, eagerly, at every cut
            self.learner.grads.all_reduce_mean_(self.learner.group)
            graph.replay()
        self.learner.invalidate_weight_cache()
        return self.out


class Evaluation(_EnvObs):
    """The reference's ``test_agent()`` / ``load_and_run_policy`` loop (run.py:63-74, :132-178) on the device: ``episodes`` evaluation
    episodes on the caller's EVALUATION simulator, ``env.B`` at a time, acting with a fixed exploration rate (0.05 there) and storing
    nothing in a replay.  A call runs ``episodes / env.B`` rounds of: the simulator's reset, zero hidden state, ``episode_limit`` steps
    of (no-grad policy forward, uavgnn_eps_greedy_philox, ``env.step``); the info tensors at the end of a round go to columns
    r B .. (r+1) B of a [K, episodes] float64 table and, with ``stats``, into ``stats`` under ``prefix + key``.

        ev = Evaluation(learner, test_env, episodes=10, eps=0.05, seed=0)
        table = ev()               # {EpRet, EpLen, AvgGlobalUtility, TotalThroughput, FairIdx[, ProbCollision]: float64 [episodes]} (device)

    It leaves the training run untouched: the uniforms come from the evaluation's own device {seed, step} (``rng``), never from
    ``learner._gen``; the weight planes live in a store of the call's own, not in the learner's rollout store; no parameter is
    written; every ``rng_state`` of the policy's modules (DiscreteComm's in-kernel noise counter) is copied on the device before the
    rounds and copied back after them.  A comm module that no training forward has seeded yet seeds itself from torch's host generator
    during the call: it is put back to unseeded and the host generator's state restored, so the training run later draws the seed it
    would have drawn (until then every such evaluation draws the same noise).  No host state enters the launches, so
    ``GraphedEvaluation`` replays them as one graph.

    env / enc: as for ``Episode``.  ``eps`` lives in device memory (``eps``: float32 [1]) and may be refilled between calls.

    film: a ``film.Film`` of exactly ``episodes`` episodes of env's shape - the reference's ``record=True`` (run.py:73-74): every round
    reloads it after the reset and clicks it after every step, one launch each (csrc/film.hip), so a call overwrites the film with the
    trajectories of the episodes it just ran.  None: no such launch is issued."""

    def __init__(self, learner, env, episodes: int, eps: float = 0.05, seed: int = 0, enc: str = "gnn", stats=None,
                 prefix: str = "Test", film=None):
        self.learner, self.stats, self.prefix, self.film = learner, stats, prefix, film
        self.episodes = int(episodes)
        if self.episodes < 1 or self.episodes % env.B != 0:
            raise ValueError(f"episodes = {episodes} is no positive multiple of the simulator's {env.B} environments")
        self.rounds = self.episodes // env.B
        if film is not None:
            if film.episodes != self.episodes:
                raise ValueError(f"film: it holds {film.episodes} episodes, the evaluation runs {self.episodes}")
            film.match(env)
        self._bind_env(learner, env, enc)
        if stats is not None:
            missing = [prefix + k for k in self.keys if prefix + k not in stats.index]
            if missing:
                raise ValueError(f"stats: keys {missing} are missing")
        dev = learner.device
        # built here, outside any capture (host-to-device copies)
        self.h_zero = learner.init_hidden(env.B)
        self.eps = th.tensor([float(eps)], dtype=th.float32, device=dev)
        self.rng = th.tensor([int(seed), 0], dtype=th.int64, device=dev)       # {seed, step} of the selection's uniforms
        self.table = th.zeros(len(self.keys), self.episodes, dtype=th.float64, device=dev)
        self.out = {k: self.table[i] for i, k in enumerate(self.keys)}

    def _comm_modules(self):
        return [m for m in self.learner.policy_net.modules() if hasattr(m, "rng_state")]

    def _comm_save(self):
        """The policy's comm ``rng_state``s before the rounds: device copies of the ones that exist; for a module that was never
        seeded (no training forward yet) the host generator's state, which its first forward draws the seed from."""
        mods = self._comm_modules()
        saved = [(m, m.rng_state.clone() if isinstance(m.rng_state, th.Tensor) else None) for m in mods]
        host = th.get_rng_state() if any(st is None for _, st in saved) else None
        return saved, host

    def _comm_restore(self, saved, host, unseed: bool = True):
        """Copies the saved states back.  A module this evaluation seeded itself goes back to unseeded and the host generator to
        where it stood (``unseed``), so the training run's first forward draws the seed it would have drawn without the evaluation."""
        for m, st in saved:
            if st is not None:
                m.rng_state.copy_(st)
            elif isinstance(m.rng_state, th.Tensor):
                if unseed:
                    m.rng_state = None
                else:
                    m.rng_state[1:].zero_()
        if host is not None and unseed:
            th.set_rng_state(host)

    @th.no_grad()
    def _rounds(self) -> None:
        lr, env, B, film = self.learner, self.env, self.env.B, self.film
        with ops.frozen_weights():            # a store of this call's own: the learner's rollout store is not touched
            for r in range(self.rounds):
                self._reset()
                if film is not None:
                    film.reload(env, r * B)
                h, info = self.h_zero, None
                for _ in range(env.episode_limit):
                    logits, h = lr.policy_net(self._obs(), h)
                    acts = _select(lr, logits, self.eps, self.rng)
                    _, _, _, info = env.step(acts)
                    if film is not None:
                        film.click(env, acts, r * B)
                for i, k in enumerate(self.keys):
                    self.table[i, r * B:(r + 1) * B].copy_(info[k], non_blocking=True)
                if self.stats is not None:
                    self.stats.push(**{self.prefix + k: info[k] for k in self.keys})

    def _body(self, unseed: bool = True) -> Dict[str, th.Tensor]:
        saved, host = self._comm_save()
        self._rounds()
        self._comm_restore(saved, host, unseed)
        return self.out

    def __call__(self) -> Dict[str, th.Tensor]:
        return self._body()


class GraphedEvaluation(Evaluation):
    """``Evaluation`` as ONE graph replay covering all rounds.

        gev = GraphedEvaluation(learner, test_env, episodes=10, stats=st)
        table = gev()              # replays; the table rows are the graph's fixed buffers

    The body runs ``warmup`` times for real on a side stream before the single-stream capture; the evaluation's {seed, step}, the
    simulator's reset counter, the policy's comm ``rng_state``s, the accumulator of ``stats`` and the status word of ``film`` are restored
    afterwards, so a graphed evaluation starts where an eager one starts.  The weight planes are rebuilt inside the graph, so a replay evaluates the CURRENT
    parameters."""

    def __init__(self, learner, env, episodes: int, eps: float = 0.05, seed: int = 0, enc: str = "gnn", stats=None,
                 prefix: str = "Test", warmup: int = 2, film=None):
        super().__init__(learner, env, episodes, eps, seed, enc, stats, prefix, film)
        window = _Window()               # the generator is not registered: the selection draws from the evaluation's own `rng`
        self.graph = window.graphs[0]
        state = [self.rng, env.reset_rng]
        state += [m.rng_state for m in self._comm_modules() if isinstance(m.rng_state, th.Tensor)]
        if stats is not None:
            state += stats.state_tensors()
        if film is not None:
            state.append(film.status)                # the film ROWS the warm-up wrote are overwritten by the first replay
        # a comm module no training forward has seeded yet is seeded by the warm-up (a host round trip the capture cannot hold) and stays
        # seeded through the capture; afterwards the graph keeps ITS tensor (``_held``: the address it reads, saves and restores), the
        # module goes back to unseeded and the host generator to where it stood
        unseeded, host = self._comm_save()
        # no learner: the evaluation writes no parameter, never draws from the generator and keeps its planes in a store of its own;
        # at least one warm-up: the seeding above
        _warm_up_and_capture(max(int(warmup), 1), lambda: self._body(unseed=False), window, state=state)
        self._held = [m.rng_state for m, st in unseeded if st is None and isinstance(m.rng_state, th.Tensor)]
        for t in self._held:
            t[1:].zero_()
        self._comm_restore(unseeded, host, unseed=True)

    def __call__(self) -> Dict[str, th.Tensor]:
        self.graph.replay()
        return self.out
