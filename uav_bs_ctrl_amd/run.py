"""``train()`` of the reference's two ``run.py`` (algos/madrqn/run.py:22-129, algos/drqn/run.py:22-125) over the device loop: epochs,
log rows, checkpoints, trajectory films and resume.

    run = Run.create(exp="exp3", env="8ubs", args=args, output_dir="data/exp3_8ubs_s0", seed=0, n_envs=32)
    run.train()                          # all remaining epochs; run.train(epochs=k): k more
    run = Run.resume("data/exp3_8ubs_s0")    # rebuilds everything from config.json + state.pt and goes on, bit for bit
    python -m uav_bs_ctrl_amd.run --exp exp3 --env 8ubs --args-json args.json --out data/exp3_8ubs_s0 [--seed 0 --envs 32 --resume --eager --compact-replay
                                  --prioritized ALPHA BETA ETA EPS --returns nstep 3 | --returns lambda 0.8 --noisy SIGMA0
                                  --quantiles K]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N -m uav_bs_ctrl_amd.run ...     # data-parallel: N ranks, one GPU each

This is host orchestration over launches that exist: a collect-only and a training ``graphs.GraphedEpisode``, one
``graphs.GraphedEvaluation`` with a ``film.Film``, one ``stats.EpochStats``.  It adds no launch and no host synchronisation to an
episode or to an evaluation; per epoch it adds one ``EpochStats.summary()`` copy, ``replay.check()``, ``film.check()`` and file I/O.

Data-parallel over a ``torch.distributed`` process group: every rank runs this driver on its own environments, ring
and sampler; the training episode is a list of graphs cut at each update's gradient all-reduce.  Rank 0 evaluates and writes the
directory, rank r >= 1 writes ``state.rank{r}.pt`` only; per epoch every rank adds one all-gather of the statistics (``stats.merge_acc``),
one of a parameter checksum (``ReplicasDiverged``) and a barrier between writing and renaming the state files.

The run directory is the reference's (utils/logx.py): ``config.json``, ``progress.txt`` (tab-separated, the reference's columns),
``checkpoint_epoch{k}.pt`` (``learner.save_checkpoint``: the reference's keys, for interchange), ``epoch{k}_episode{n}/`` (``Film.write``)
- so ``plot_results.py``, ``collect_curves.py`` and ``test_policies.py`` read it - plus ``state.pt``, everything a resumed run needs that
a checkpoint does not hold: the target network, the optimiser's moments and counters, the replay ring and its counters, the exploration
counter and its random pair, the simulators' reset counters, the evaluation's random pair, every DiscreteComm ``rng_state`` of policy
AND target network.

Arguments: ``args`` (a namespace or a dict) carries every key the learner reads plus the driver's (``DRIVER_KEYS``); a missing key is a
``ValueError`` that names it - the package holds no table of defaults (README: one complete example).  Interactions are counted as the
device loop counts them, E per step of E environments (``plan``); ``updates_per_segment = n_envs`` keeps the reference's ratio of
updates per environment interaction (one update per ``max_seq_len`` interactions), the default 1 is one update per ``max_seq_len`` steps
of all E environments."""
from __future__ import annotations

import dataclasses
import json
import os
import time
from types import SimpleNamespace
from typing import Dict, NamedTuple, Optional

EXPS = ("exp1", "exp2", "exp3")
DRIVER_KEYS = ("steps_per_epoch", "epochs", "update_after", "num_test_episodes", "save_freq", "decay_steps", "batch_size", "replay_size",
               "max_seq_len", "anneal_lr")
_MULTI_KEYS = ("device", "o", "c", "share_reward", "hidden_size", "n_layers", "n_heads", "msg_size", "key_size", "n_rounds", "lr", "gamma",
               "polyak", "double_q", "dueling", "mixer")
LEARNER_KEYS = {"exp1": ("device", "agent", "hidden_size", "n_layers", "n_heads", "lr", "gamma", "polyak"), "exp2": _MULTI_KEYS,
                "exp3": _MULTI_KEYS}
EPS_START, EPS_END, TEST_EPS = 1.0, 0.05, 0.05                     # run.py:60, :68
# the log row between Episode and TotalEnvInteracts (madrqn run.py:117-123, drqn run.py:113-118): (key, with_min_and_max, average_only)
ROW_KEYS = {False: (("EpRet", True, False), ("EpLen", False, True), ("AvgGlobalUtility", True, False), ("TotalThroughput", False, True),
                    ("FairIdx", False, True), ("ProbCollision", False, True), ("TestEpRet", True, False)),
            True: (("EpRet", True, False), ("EpLen", False, True), ("AvgGlobalUtility", True, False), ("FairIdx", False, True),
                   ("TotalThroughput", False, True), ("TestEpRet", True, False))}
STATE_VERSION = 1


class TrainingDiverged(RuntimeError):
    """An epoch's updates produced a non-finite loss: the row was written, ``state.pt`` was not."""


class RunDirectoryError(RuntimeError):
    """``Run.resume`` refuses the directory; the message says why."""


class ReplicasDiverged(RuntimeError):
    """A data-parallel run whose ranks no longer hold the same parameters, bit for bit: raised on every rank at the end of the epoch."""


# ---- arguments and the plan -------------------------------------------------------------------------------------------------------------
def check_args(exp: str, args) -> SimpleNamespace:
    """A namespace copy of ``args`` (a namespace or a dict) holding every key ``exp`` needs; ``mixer`` forces ``share_reward``
    (algos/common.py:21-25, the one rule of ``check_args_sanity`` that matters here: the device is the caller's)."""
    if exp not in EXPS:
        raise ValueError(f"exp must be one of {EXPS}, got {exp!r}")
    d = dict(args) if isinstance(args, dict) else dict(vars(args))
    need = LEARNER_KEYS[exp] + DRIVER_KEYS + (("embed_dim",) if d.get("mixer") else ())
    missing = [k for k in need if k not in d]
    if missing:
        raise ValueError(f"args: missing {', '.join(missing)} ({exp} needs {', '.join(need)}; the package holds no defaults)")
    if d.get("mixer") and not d["share_reward"]:
        d["share_reward"] = True
    for k in ("steps_per_epoch", "epochs", "num_test_episodes", "save_freq", "batch_size", "replay_size"):
        if int(d[k]) < 1:
            raise ValueError(f"args.{k} = {d[k]}: a positive integer expected")
    return SimpleNamespace(**d)


class Plan(NamedTuple):
    total_steps: int            # run.py:55
    update_after_eff: int       # run.py:56: max(update_after, world * batch_size * T)
    update_every: int           # run.py:57: T
    steps_per_episode: int      # interactions of one episode replay on all ranks: world * E * episode_limit
    episodes_per_epoch: int     # ceil(steps_per_epoch / steps_per_episode)
    interacts_per_epoch: int    # what an epoch actually runs: episodes_per_epoch * steps_per_episode
    epochs: int

    def collect_only(self, interactions_before: int) -> bool:
        """An episode replay is collect-only iff the interactions before it are fewer than ``update_after_eff``."""
        return interactions_before < self.update_after_eff


def plan(args, E: int, episode_limit: int, T: int, world: int = 1) -> Plan:
    """The numbers of run.py:55-57 and their counterparts for E environments that end their episodes together on each of ``world``
    data-parallel ranks: interactions count all ranks, and training starts once EVERY rank's ring holds a batch (``world * batch_size *
    T`` interactions).  Pure host arithmetic on values that are equal on all ranks, so they switch from collecting to training on the
    same episode replay."""
    g = (lambda k: args[k]) if isinstance(args, dict) else (lambda k: getattr(args, k))
    E, episode_limit, T, world = int(E), int(episode_limit), int(T), int(world)
    if E < 1 or episode_limit < 1 or T < 1 or world < 1:
        raise ValueError("plan: E, episode_limit, T and world must be positive")
    per_episode = world * E * episode_limit
    episodes = -(-int(g("steps_per_epoch")) // per_episode)
    return Plan(int(g("steps_per_epoch")) * int(g("epochs")), max(int(g("update_after")), world * int(g("batch_size")) * T), T,
                per_episode, episodes, episodes * per_episode, int(g("epochs")))


def eps_thres(t: int, decay_steps: float) -> float:
    """run.py:61 on the host (the ``ExploreEps`` column of exp1; the device loop evaluates uavgnn_eps_schedule)."""
    return max(EPS_END, -(EPS_START - EPS_END) / decay_steps * t + EPS_START)


RANK_SEED_STRIDE = 4096
RANK_SEEDS = ("train_env", "replay", "explore", "comm")            # what differs between the ranks of a data-parallel run


def derive_seeds(seed: int, rank: int = 0) -> Dict[str, int]:
    """The seeds of a run's random states, all from ``seed``: torch's generator (parameter initialisation), the two simulators' placement
    samplers, the replay's sampler, the exploration pair, the evaluation's pair, the DiscreteComm noise (+ the module's index).  Rank r of
    a data-parallel run shifts ``RANK_SEEDS`` by 4096 r: its own environments, ring samples, exploration and noise; ``torch`` is every
    rank's (the parameters are rank 0's anyway), ``test_env`` and ``evaluation`` are read on rank 0 only."""
    base = 1000003 * int(seed)
    seeds = dict(torch=int(seed), train_env=base + 1, test_env=base + 2, replay=base + 3, explore=base + 4, evaluation=base + 5,
                 comm=base + 16)
    return _rank_seeds(seeds, rank)


def _rank_seeds(seeds: Dict[str, int], rank: int) -> Dict[str, int]:
    if int(rank) < 0:
        raise ValueError("rank must not be negative")
    return {k: int(v) + (RANK_SEED_STRIDE * int(rank) if k in RANK_SEEDS else 0) for k, v in seeds.items()}


def state_file(rank: int) -> str:
    """The name of rank ``rank``'s state file in the run directory."""
    return "state.pt" if int(rank) == 0 else f"state.rank{int(rank)}.pt"


def _gather_ints(value: int, device, group):
    """[value of every rank of ``group``], through one all-gather of an int64 on ``device``."""
    import torch as th
    import torch.distributed as dist
    mine = th.tensor([int(value)], dtype=th.int64, device=device)
    parts = [th.empty_like(mine) for _ in range(dist.get_world_size(group))]
    dist.all_gather(parts, mine, group=group)
    return [int(p) for p in parts]


def comm_modules(learner):
    """[(name, module)] of every module with a device ``rng_state`` (DiscreteComm), policy network first, then target network."""
    return [(f"{net_name}.{name}", m) for net_name, net in (("policy", learner.policy_net), ("target", learner.target_net))
            for name, m in net.named_modules() if hasattr(m, "rng_state")]


def seed_comm_modules(learner, seed: int) -> None:
    """Gives every DiscreteComm module its ``rng_state`` {seed + index, 0} now, instead of on its first forward from torch's host
    generator: the tensor exists before any graph is captured, so the captures snapshot it and ``state.pt`` can restore it in place."""
    import torch as th
    for i, (_, m) in enumerate(comm_modules(learner)):
        m.rng_state = th.tensor([int(seed) + i, 0], dtype=th.int64, device=learner.device)


# ---- the run directory ------------------------------------------------------------------------------------------------------------------
def _jsonable(obj):
    """utils/serialization_utils.py ``convert_json``: what serialises stays, containers are walked, a named object becomes its name, an
    object with attributes {str(obj): its attributes}, anything else its ``str``."""
    try:
        json.dumps(obj)
        return obj
    except (TypeError, ValueError):
        pass
    if isinstance(obj, dict):
        return {_jsonable(k): _jsonable(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [_jsonable(x) for x in obj]
    name = getattr(obj, "__name__", None)
    if name is not None and "lambda" not in name:
        return _jsonable(name)
    if getattr(obj, "__dict__", None):
        return {str(obj): {_jsonable(k): _jsonable(v) for k, v in obj.__dict__.items()}}
    return str(obj)


def config_text(config: dict, exp_name: Optional[str] = None) -> str:
    """The text of ``config.json`` by the rule of utils/logx.py:126-134."""
    out = _jsonable(config)
    if exp_name is not None:
        out["exp_name"] = exp_name
    return json.dumps(out, separators=(",", ":\t"), indent=4, sort_keys=True)


class RunLogger:
    """``progress.txt`` and ``config.json`` of the reference's ``EpochLogger`` (utils/logx.py), fed from an ``EpochStats.summary()``
    instead of ``store``.

        log = RunLogger(output_dir, exp_name)           # append=True: re-opens progress.txt without a second header
        log.save_config(dict(env_fn=..., env_kwargs=..., seed=..., args=namespace))
        log.summary = stats.summary()
        log.log_tabular("Epoch", 3); log.log_tabular("EpRet", with_min_and_max=True); log.log_tabular("EpLen", average_only=True)
        log.dump_tabular()                              # header once, one tab-separated row, flushed (logx.py:207-233)

    ``log_tabular`` without a value applies the naming rule of logx.py:302-307 to ``summary``: ``Average<key>`` (``<key>`` alone with
    ``average_only``), ``Std<key>`` unless ``average_only``, ``Max<key>`` and ``Min<key>`` with ``with_min_and_max``."""

    def __init__(self, output_dir: str, exp_name: Optional[str] = None, append: bool = False, output_fname: str = "progress.txt"):
        self.output_dir, self.exp_name = output_dir, exp_name
        os.makedirs(output_dir, exist_ok=True)
        path = os.path.join(output_dir, output_fname)
        self.headers, self.first_row = [], True
        if append and os.path.exists(path):
            with open(path) as f:
                head = f.readline().rstrip("\n")
            if head:
                self.headers, self.first_row = head.split("\t"), False
        self.file = open(path, "a" if append else "w")
        self.row: Dict[str, object] = {}
        self.summary: Dict[str, float] = {}

    def save_config(self, config: dict) -> None:
        with open(os.path.join(self.output_dir, "config.json"), "w") as f:
            f.write(config_text(config, self.exp_name))

    def _put(self, key: str, val) -> None:
        if self.first_row:
            self.headers.append(key)
        elif key not in self.headers:
            raise KeyError(f"progress.txt has no column {key!r}: the columns are fixed by the first row")
        if key in self.row:
            raise KeyError(f"{key!r} was already set in this row")
        self.row[key] = val

    def log_tabular(self, key: str, val=None, with_min_and_max: bool = False, average_only: bool = False) -> None:
        if val is not None:
            self._put(key, val)
            return
        s = self.summary
        self._put(key if average_only else "Average" + key, s["Average" + key])
        if not average_only:
            self._put("Std" + key, s["Std" + key])
        if with_min_and_max:
            self._put("Max" + key, s["Max" + key])
            self._put("Min" + key, s["Min" + key])

    def dump_tabular(self) -> None:
        if self.first_row:
            self.file.write("\t".join(self.headers) + "\n")
        self.file.write("\t".join(str(self.row.get(k, "")) for k in self.headers) + "\n")
        self.file.flush()
        self.row.clear()
        self.first_row = False

    def close(self) -> None:
        if not self.file.closed:
            self.file.close()


# ---- the environment of a run and its description in config.json ----------------------------------------------------------------------
def _env_to_config(exp: str, env) -> dict:
    from .sim import MAPS, MapSpec, SingleUbsParams
    if exp == "exp1":
        if not isinstance(env, SingleUbsParams):
            raise ValueError(f"exp1 runs the single-UBS simulator: env must be a SingleUbsParams, got {type(env).__name__}")
        return dict(single=dataclasses.asdict(env))
    if isinstance(env, str):
        if env not in MAPS:
            raise ValueError(f"unknown map {env!r}: one of {sorted(MAPS)}")
        return dict(map=env)
    if isinstance(env, MapSpec):
        return dict(map_spec=dataclasses.asdict(env))
    raise ValueError(f"{exp} runs the multi-UBS simulator: env must be a map id or a MapSpec, got {type(env).__name__}")


def _tuples(x):
    return tuple(_tuples(v) for v in x) if isinstance(x, (list, tuple)) else x


def _env_from_config(d: dict):
    from .sim import MapParams, MapSpec, SingleUbsParams
    if "single" in d:
        return SingleUbsParams(**{k: _tuples(v) for k, v in d["single"].items()})
    if "map" in d:
        return d["map"]
    spec = {k: _tuples(v) for k, v in d["map_spec"].items() if k != "params"}
    return MapSpec(params=MapParams(**{k: _tuples(v) for k, v in d["map_spec"]["params"].items()}), **spec)


def _reference_env(exp: str, env) -> tuple:
    """(env_fn, env_kwargs) as the reference's launchers pass them (run_exp1.py, run_exp2.py, run_exp3.py): what test_policies.py reads."""
    if exp == "exp1":
        keys = ("range_pos", "episode_limit", "n_grps", "gts_per_grp", "r_cov", "n_rbs", "vels", "n_dirs")
        return "SingleUbsCoverageEnv", {k: getattr(env, k) for k in keys}
    from .sim import MAPS
    p = (MAPS[env] if isinstance(env, str) else env).params
    return "MultiUbsCoverageEnv", dict(map_id=env if isinstance(env, str) else None, fair_service=bool(p.fair_service),
                                       avoid_collision=bool(p.avoid_collision))


def run_config(exp: str, env, ns, seed: int = 0, n_envs: int = 32, n_test_envs: Optional[int] = None, updates_per_segment: int = 1,
               graphed: bool = True, save_replay: bool = True, world: int = 1, force_collective: bool = False,
               compact_replay: bool = False, prioritized=None, returns=None, noisy=None, quantiles=None) -> dict:
    """The ``uav_bs_ctrl_amd`` entry of ``config.json``: everything of ``Run.create``'s arguments that ``Run.resume`` needs to rebuild the
    same run (host only).  compact_replay with exp1 is a ``ValueError``: the single-UBS observations are M x 4 floats already.
    prioritized: None, or (alpha, beta, eta, eps) - the key ``prioritized`` enters the entry ONLY when set (absent means off, so a
    directory written before the option existed resumes unchanged).  returns: None, ("nstep", n) or ("lambda", lam) - the learner's
    multi-step TD target; the key ``returns`` likewise enters ONLY when set.  noisy: None or sigma0, a number - the noisy-net Q head;
    the key ``noisy`` likewise enters ONLY when set.  quantiles: None or K, the number of quantiles of the distributional Q head; the key
    ``quantiles`` likewise enters ONLY when set."""
    if compact_replay and exp == "exp1":
        raise ValueError("compact_replay: the compact ring stores the multi-UBS simulator's state (exp2 / exp3); exp1's observations "
                         "are already n_gts x 4 floats per step")
    out = dict(exp=exp, env=_env_to_config(exp, env), n_envs=int(n_envs),
               n_test_envs=int(ns.num_test_episodes if n_test_envs is None else n_test_envs),
               updates_per_segment=int(updates_per_segment), graphed=bool(graphed), save_replay=bool(save_replay),
               seeds=derive_seeds(seed), world=int(world), force_collective=bool(force_collective), compact_replay=bool(compact_replay))
    if prioritized is not None:
        out["prioritized"] = _prioritized(prioritized)
    if returns is not None:
        out["returns"] = _returns(returns)
    if noisy is not None:
        out["noisy"] = _noisy(noisy)
    if quantiles is not None:
        out["quantiles"] = _quantiles(quantiles)
    return out


def _quantiles(value) -> int:
    """K of the quantile-regression Q head as config.json holds it: one of the kernel's quantile counts (8, 16, 32, 64)."""
    if isinstance(value, bool) or not isinstance(value, int) or value not in (8, 16, 32, 64):
        raise ValueError(f"quantiles: None or K in (8, 16, 32, 64) expected, got {value!r}")
    return int(value)


def _noisy(value) -> float:
    """sigma0 of the noisy-net Q head as config.json holds it: a non-negative number."""
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not value >= 0:
        raise ValueError(f"noisy: None or sigma0, a non-negative number, expected, got {value!r}")
    return float(value)


def _returns(values) -> list:
    """["nstep", n] / ["lambda", lam] as config.json holds them (checked by ``ops.normalize_returns``, host only)."""
    from .ops import normalize_returns
    return list(normalize_returns(tuple(values) if isinstance(values, list) else values))


def parse_returns(words) -> tuple:
    """The two words of ``--returns KIND VALUE`` -> ("nstep", n) or ("lambda", lam)."""
    kind, value = words
    try:
        number = float(value)
    except ValueError:
        raise ValueError(f"--returns {kind} {value}: the value is a number") from None
    return tuple(_returns((kind, number)))


def _prioritized(values) -> list:
    """[alpha, beta, eta, eps] as floats (the ring's constructor checks their ranges)."""
    try:
        out = [float(v) for v in values]
    except (TypeError, ValueError):
        out = []
    if len(out) != 4:
        raise ValueError(f"prioritized: None or four numbers (alpha, beta, eta, eps) expected, got {values!r}")
    return out


# ---- the driver -------------------------------------------------------------------------------------------------------------------------
class Run:
    """One training run and its directory.  Build it with ``Run.create`` or ``Run.resume``.

    Attributes a caller may read: ``learner``, ``env`` / ``test_env`` (the training and the evaluation simulator), ``replay``, ``stats``,
    ``film``, ``collect`` / ``train_episode`` (the collect-only and the training episode), ``evaluation``, ``plan``, ``seeds``, and the
    host counters ``epoch`` (epochs finished), ``replays`` (episode replays finished), ``interacts``, ``elapsed``.

    Data-parallel (``torch.distributed`` initialised when the run is built): ``world`` / ``rank`` / ``group``.  Every rank owns its
    ``n_envs`` environments, its ring and its sampler (``seeds``: this rank's), the parameters are replicated and an update is
    ``batch_size`` sequences per rank followed by one all-reduce.  ``test_env``, ``film``, ``evaluation`` and ``logger`` exist on rank 0
    only (None elsewhere); ``interacts`` counts all ranks."""

    def __init__(self, ours: dict, args: SimpleNamespace, output_dir: str, exp_name: Optional[str], resuming: bool, group=None):
        import torch as th
        import torch.distributed as dist

        from .film import Film
        from .graphs import Episode, Evaluation, GraphedEpisode, GraphedEvaluation, info_keys
        from .learner import MultiAgentQLearner, QLearner
        from .replay import CompactSequenceReplay, SequenceReplay, SingleUbsSequenceReplay
        from .sim import BatchedSingleUbsCoverageEnv, BatchedUbsCoverageEnv
        from .stats import EpochStats
        self.ours, self.args, self.output_dir, self.exp_name = ours, args, output_dir, exp_name
        self.distributed = dist.is_available() and dist.is_initialized()
        self.group = group if self.distributed else None
        self.world, self.rank = (dist.get_world_size(group), dist.get_rank(group)) if self.distributed else (1, 0)
        if self.rank < 0:
            raise ValueError("this process is no member of `group`")
        force = bool(ours.get("force_collective", False))
        if force and not self.distributed:
            raise ValueError("force_collective needs an initialised torch.distributed process group")
        if int(ours.get("world", 1)) != self.world:
            raise ValueError(f"the run is described for world size {ours.get('world', 1)}, the process group holds {self.world} ranks")
        # the statistics merge, the replica check and the barrier of the state files run whenever the update holds its collective
        self.collective = self.world > 1 or force
        exp, E, seeds = ours["exp"], int(ours["n_envs"]), _rank_seeds(ours["seeds"], self.rank)      # config.json holds rank 0's
        self.exp, self.single, self.seeds, self.save_replay = exp, exp == "exp1", seeds, bool(ours["save_replay"])
        E_test = int(ours["n_test_envs"])
        self.compact_replay = bool(ours.get("compact_replay", False))     # absent in a config.json written before the option existed
        if self.compact_replay and self.single:
            raise ValueError("compact_replay: the compact ring stores the multi-UBS simulator's state (exp2 / exp3), not exp1's")
        # absent in a config.json written without the option: the uniform sampler, no priority tensors
        self.prioritized = tuple(_prioritized(ours["prioritized"])) if ours.get("prioritized") is not None else None
        # absent likewise: the reference's one-step target
        self.returns = tuple(_returns(ours["returns"])) if ours.get("returns") is not None else None
        # absent likewise: the plain / dueling head, the reference's exploration alone
        self.noisy = _noisy(ours["noisy"]) if ours.get("noisy") is not None else None
        # absent likewise: a scalar Q value per action
        self.quantiles = _quantiles(ours["quantiles"]) if ours.get("quantiles") is not None else None
        if getattr(args, "mixer", False):
            raise ValueError("mixer = True is not covered by the driver yet: graphs.Episode / GraphedEpisode train with a mixer, "
                             "Run does not build one")
        if E < 1 or E_test < 1 or int(args.num_test_episodes) % E_test != 0:
            raise ValueError(f"n_test_envs = {E_test} must divide num_test_episodes = {args.num_test_episodes} (n_envs = {E}: positive)")
        spec = _env_from_config(ours["env"])
        dev = args.device
        if self.single:
            enc = args.agent
            make = lambda B, k: BatchedSingleUbsCoverageEnv(spec, B, dev, seed=seeds[k])     # noqa: E731
        else:
            enc = "gnn" if exp == "exp3" else "mlp"
            if args.o != enc:
                raise ValueError(f"{exp} runs the {enc!r} observation encoder, args.o = {args.o!r}")
            make = lambda B, k: BatchedUbsCoverageEnv.from_map(spec, B, dev, seed=seeds[k])  # noqa: E731
        self.enc, self.env, self.test_env = enc, make(E, "train_env"), make(E_test, "test_env") if self.rank == 0 else None
        env, test_env = self.env, self.test_env
        th.manual_seed(seeds["torch"])           # parameter initialisation (data-parallel: rank 0's are broadcast)
        opts = dict(quantiles=self.quantiles) if self.quantiles is not None else {}
        self.learner = learner = (QLearner if self.single else MultiAgentQLearner)(env.get_env_info(enc), args, process_group=self.group,
                                                                                   returns=self.returns, noisy=self.noisy, **opts)
        if force:
            learner.grads.force_collective = True        # before anything is captured: the episode graphs are cut at the all-reduce
        assert learner.needs_collective() == self.collective
        seed_comm_modules(learner, seeds["comm"])
        T = int(args.max_seq_len) if args.max_seq_len else env.episode_limit
        self.plan = plan(args, E, env.episode_limit, T, self.world)
        if self.single:
            self.replay = SingleUbsSequenceReplay(int(args.replay_size), T, env.n_gts, args.hidden_size, n_envs=E, device=dev,
                                                  device_state=True, seed=seeds["replay"], prioritized=self.prioritized)
        elif self.compact_replay:                # simulator state instead of observations: the same update inputs, bit for bit
            self.replay = CompactSequenceReplay.for_env(env, int(args.replay_size), T, args.hidden_size,
                                                        rew_dim=1 if args.share_reward else None, seed=seeds["replay"],
                                                        prioritized=self.prioritized)
        else:
            self.replay = SequenceReplay(int(args.replay_size), T, env.n_agents, env.n_gts, args.hidden_size, n_envs=E,
                                         r_comm=env.p.r_comm, rew_dim=1 if args.share_reward else None, device=dev,
                                         device_state=True, seed=seeds["replay"], prioritized=self.prioritized)
        graphed = bool(ours["graphed"])
        ep_cls, ev_cls = (GraphedEpisode, GraphedEvaluation) if graphed else (Episode, Evaluation)
        kw = dict(eps=(EPS_START, EPS_END, float(args.decay_steps)), updates_per_segment=int(ours["updates_per_segment"]), enc=enc)
        self.info_keys = info_keys(self.single)
        self.stats = EpochStats(list(self.info_keys) + ["LossQ"] + ["Test" + k for k in self.info_keys], dev, cap=max(64, E, E_test))
        self.film = Film(test_env, int(args.num_test_episodes)) if self.rank == 0 else None
        # the three captures run on the fresh, empty state - also when resuming: a warm-up episode commits into the ring at the restored
        # head, so captured after a full ring was loaded it would overwrite the oldest sequences.  `_load_state` copies IN PLACE afterwards
        self.collect = ep_cls(learner, env, self.replay, int(args.batch_size), train=False, stats=self.stats,
                              explore_seed=seeds["explore"], **kw)
        self.train_episode = ep_cls(learner, env, self.replay, int(args.batch_size), train=True, stats=self.stats,
                                    explore_seed=seeds["explore"], **kw)
        self.evaluation = ev_cls(learner, test_env, int(args.num_test_episodes), eps=TEST_EPS, seed=seeds["evaluation"], enc=enc,
                                 stats=self.stats, film=self.film) if self.rank == 0 else None
        self.epoch = self.replays = self.interacts = 0
        self.elapsed = 0.0
        self.active = "collect"          # the episode object whose `t` / `explore` are current
        self.ring_base = 0               # interactions when the ring was last empty: training starts update_after_eff later
        self.logger = RunLogger(output_dir, exp_name, append=resuming) if self.rank == 0 else None

    # ---- construction -------------------------------------------------------------------------------------------------------------
    @classmethod
    def create(cls, exp: str, env, args, output_dir: str, exp_name: Optional[str] = None, seed: int = 0, n_envs: int = 32,
               n_test_envs: Optional[int] = None, updates_per_segment: int = 1, graphed: bool = True, save_replay: bool = True,
               group=None, force_collective: bool = False, compact_replay: bool = False, prioritized=None, returns=None,
               noisy=None, quantiles=None) -> "Run":
        """Builds simulators, learner, replay, statistics, film and the three graphs (``graphed=False``: their eager forms) as
        run.py:47-61 builds them and writes ``config.json``; sets torch's generator (``torch.manual_seed(seed)``, as the reference's
        ``set_rand_seed`` does) for the parameter initialisation.  env: a map id of ``sim.MAPS`` or a ``MapSpec`` (exp2 / exp3), a
        ``SingleUbsParams`` (exp1).  n_test_envs: evaluation environments (default ``num_test_episodes``; must divide it).
        save_replay=False: ``state.pt`` leaves the ring out (gigabytes at exp3 sizes); a resumed run then collects ``update_after_eff``
        interactions again before it trains and is NOT bit-identical to an uninterrupted one.
        compact_replay=True (exp2 / exp3): the ring is a ``replay.CompactSequenceReplay`` - simulator state instead of observations,
        about 18 x fewer bytes per sequence in HBM and in ``state.pt``, the same update inputs bit for bit; exp1: ``ValueError``.
        prioritized=(alpha, beta, eta, eps): proportional prioritised replay over sequences on the device (``replay._RingState``) - the
        ring draws by priority, the loss carries the importance weights and every update rewrites the priorities of its batch;
        ``state.pt`` then holds ``replay.prio`` / ``replay.prio_max``.  None (the default): the uniform sampler, nothing changes.
        returns=("nstep", n) / ("lambda", lam): the learner trains on n-step / lambda returns over the stored sequence instead of the
        one-step target (``MultiAgentQLearner(returns=...)``); None (the default): the reference's update, not one launch differs.
        noisy=sigma0: the noisy-net Q head (``MultiAgentQLearner(noisy=...)``) - per-row draws in the rollouts, one folded draw per
        network and update, the means in evaluations; the sigmas travel in the state_dict, both networks' noise pairs in ``state.pt``
        (``comm.*``) and the policy's in checkpoints (``comm_rng_state``).  The epsilon schedule is untouched.  None: not one launch differs.
        quantiles=K (8, 16, 32 or 64): the distributional value function in quantile-regression form
        (``MultiAgentQLearner(quantiles=...)``) - ``f_out.weight`` is [n_actions * K, H] in checkpoints, rollouts and evaluations act on the
        quantile means, the update is the quantile-Huber loss on one-step or ``("nstep", n)`` targets; with ``("lambda", lam)``, ``noisy``
        or a dueling head: ``ValueError``.  It adds no collective and no random stream.  None: not one launch differs.

        With ``torch.distributed`` initialised the run is data-parallel over ``group`` (default: the world) and EVERY rank calls
        ``create`` with the same arguments but its own ``args.device``; ``n_envs`` and ``args.batch_size`` are per rank.
        force_collective: the gradient all-reduce (and with it the cut episode graphs) also at world size 1."""
        import torch.distributed as dist
        ns = check_args(exp, args)
        world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        ours = run_config(exp, env, ns, seed, n_envs, n_test_envs, updates_per_segment, graphed, save_replay, world, force_collective,
                          compact_replay, prioritized, returns, noisy, quantiles)
        run = cls(ours, ns, output_dir, exp_name, resuming=False, group=group)
        if run.rank == 0:
            env_fn, env_kwargs = _reference_env(exp, env)
            config = dict(env_fn=env_fn, env_kwargs=env_kwargs, seed=int(seed), args=ns, uav_bs_ctrl_amd=ours)
            run.logger.save_config(config)
            # a new run in an old directory must not be resumable from the old state: no rank writes a state file before the first
            # epoch's collectives, which rank 0 enters after this
            for name in os.listdir(output_dir):
                if name.startswith("state.") and (name.endswith(".pt") or name.endswith(".pt.tmp")):
                    os.remove(os.path.join(output_dir, name))
        return run

    @classmethod
    def resume(cls, output_dir: str, device=None, group=None) -> "Run":
        """Rebuilds the run of ``output_dir`` from ``config.json`` exactly as ``create`` built it - captures included, on the fresh
        state - then copies ``state.pt`` in place into the tensors the graphs hold addresses of, and re-opens ``progress.txt`` for
        append.  Raises ``RunDirectoryError`` for a directory without ``state.pt``, a ``config.json`` that does not rebuild the saved
        shapes, and a run that is already complete.

        device: overrides ``args.device`` of ``config.json`` (a rank's own ``cuda:{LOCAL_RANK}``).  A data-parallel run is resumed by
        every rank of a group of the saved world size, rank r from ``state.rank{r}.pt``; another world size, a rank file that is
        missing and rank files of different epochs raise ``RunDirectoryError`` on EVERY rank, so none walks into a collective alone."""
        import torch as th
        import torch.distributed as dist
        distributed = dist.is_available() and dist.is_initialized()
        world, rank = (dist.get_world_size(group), dist.get_rank(group)) if distributed else (1, 0)
        cfg_path, state_path = os.path.join(output_dir, "config.json"), os.path.join(output_dir, state_file(rank))
        if not os.path.exists(os.path.join(output_dir, "state.pt")):
            raise RunDirectoryError(f"{output_dir}: no state.pt - nothing to resume (no epoch of this run was finished, or it is not a "
                                    f"run directory of this package)")
        try:
            with open(cfg_path) as f:
                config = json.load(f)
            ours = config["uav_bs_ctrl_amd"]
            ns = check_args(ours["exp"], next(iter(config["args"].values())))
        except (OSError, KeyError, ValueError, StopIteration, AttributeError, TypeError) as e:
            raise RunDirectoryError(f"{output_dir}: config.json does not describe a run of this package ({type(e).__name__}: {e})") from e
        if device is not None:
            ns.device = str(device)
        saved_world = int(ours.get("world", 1))
        if saved_world != world:             # read from the same file on every rank: all of them raise
            raise RunDirectoryError(f"{output_dir}: the run was saved at world size {saved_world}, this process group holds {world} "
                                    f"rank{'s' if world != 1 else ''}")
        if world > 1:
            have = _gather_ints(os.path.exists(state_path), ns.device, group)
            if not all(have):
                missing = ", ".join(state_file(r) for r, h in enumerate(have) if not h)
                raise RunDirectoryError(f"{output_dir}: a rank file is missing ({missing}): every rank of the saved run needs its own")
        state = th.load(state_path, map_location="cpu")
        if world > 1:
            epochs = _gather_ints(state["epoch"], ns.device, group)
            if len(set(epochs)) != 1:
                raise RunDirectoryError(f"{output_dir}: the rank files hold different epochs ({epochs} in rank order): the job was killed "
                                        f"between their renames")
        if int(state["epoch"]) >= int(ns.epochs):
            raise RunDirectoryError(f"{output_dir}: the run is already complete ({state['epoch']} of {ns.epochs} epochs)")
        run = cls(ours, ns, output_dir, config.get("exp_name"), resuming=True, group=group)
        run._load_state(state)
        return run

    # ---- state.pt -------------------------------------------------------------------------------------------------------------------
    def _tensors(self) -> Dict[str, object]:
        """name -> the live tensor a graph holds the address of."""
        lr, rb = self.learner, self.replay
        out = dict(zip(("learner.flat", "learner.flat_target", "learner.m", "learner.v", "learner.hyper"), lr.state_tensors()))
        out.update({"replay.state": rb.state, "replay.rng": rb.rng, "replay.status": rb.status, "env.rng": self.env.reset_rng})
        if self.rank == 0:                       # the evaluation is rank 0's alone
            out.update({"test_env.rng": self.test_env.reset_rng, "evaluation.rng": self.evaluation.rng})
        for name, ep in (("collect", self.collect), ("train", self.train_episode)):
            out.update({f"{name}.t": ep.t, f"{name}.eps": ep.eps, f"{name}.explore": ep.explore})
        out.update({"comm." + name: m.rng_state for name, m in comm_modules(lr)})
        if self.prioritized is not None:
            out.update({"replay.prio": rb.prio, "replay.prio_max": rb.prio_max})
        return out

    def _save_state(self) -> None:
        """Written to a temporary name and renamed: a killed job leaves the previous state intact.  Data-parallel: every rank writes
        its own file (``state_file``: its tensors, its ring), and renames it after a barrier that all temporary files precede."""
        import torch as th
        lr = self.learner
        state = dict(version=STATE_VERSION, epoch=self.epoch, replays=self.replays, interacts=self.interacts, elapsed=self.elapsed,
                     active=self.active, ring_base=self.ring_base, lr=float(lr.optimizer.param_groups[0]["lr"]),
                     lr_scheduler=lr.lr_scheduler.state_dict() if lr.anneal_lr else None,
                     tensors={k: v.detach().cpu() for k, v in self._tensors().items()}, mem=None)
        if self.save_replay:
            size = int(state["tensors"]["replay.state"][1])
            state["mem"] = {k: v[:size].cpu() for k, v in self.replay.mem.items()}
        path = os.path.join(self.output_dir, state_file(self.rank))
        th.save(state, path + ".tmp")
        if self.collective:
            import torch.distributed as dist
            dist.barrier(group=self.group)
        os.replace(path + ".tmp", path)

    def _load_state(self, state: dict) -> None:
        lr, rb = self.learner, self.replay
        live = self._tensors()
        saved = state.get("tensors", {})
        bad = sorted(set(live) ^ set(saved)) + [f"{k}: {tuple(saved[k].shape)} saved, {tuple(live[k].shape)} rebuilt"
                                                for k in live if k in saved and (saved[k].shape != live[k].shape
                                                                                 or saved[k].dtype != live[k].dtype)]
        mem = state.get("mem")
        if mem is not None:
            bad += [f"mem.{k}" for k in rb.mem if k not in mem or mem[k].shape[1:] != rb.mem[k].shape[1:] or mem[k].shape[0] > rb.capacity]
        if state.get("version") != STATE_VERSION or bad:
            raise RunDirectoryError(f"{self.output_dir}: config.json does not rebuild the shapes {state_file(self.rank)} holds (version "
                                    f"{state.get('version')}; {'; '.join(bad) or 'unknown layout'})")
        for k, v in live.items():
            v.copy_(saved[k])
        opt = lr.optimizer
        opt.param_groups[0]["lr"] = state["lr"]
        opt._lr_on_device = float("nan")         # the next replay's sync_lr pushes it, as it does after lr_scheduler.step()
        opt._steps = int(opt.hyper[1])
        if lr.anneal_lr:
            lr.lr_scheduler.load_state_dict(state["lr_scheduler"])
        lr.invalidate_weight_cache()
        self.epoch, self.replays, self.interacts = int(state["epoch"]), int(state["replays"]), int(state["interacts"])
        self.elapsed, self.active, self.ring_base = float(state["elapsed"]), state["active"], int(state["ring_base"])
        if mem is not None:
            for k, v in mem.items():
                rb.mem[k][:v.shape[0]].copy_(v)
        else:                                    # the ring was dropped: collect update_after_eff interactions again
            rb.state.zero_()
            self.ring_base = self.interacts

    # ---- training -------------------------------------------------------------------------------------------------------------------
    def _episode(self) -> None:
        name = "collect" if self.plan.collect_only(self.interacts - self.ring_base) else "train"
        eps = {"collect": self.collect, "train": self.train_episode}
        if name != self.active:                  # two graphs share the schedule and the exploration pair by VALUE
            eps[name].t.copy_(eps[self.active].t)
            eps[name].explore.copy_(eps[self.active].explore)
            self.active = name
        eps[name]()
        self.replays += 1
        self.interacts += self.plan.steps_per_episode

    def train(self, epochs: Optional[int] = None) -> None:
        """Runs all remaining epochs, or ``epochs`` more."""
        last = self.plan.epochs if epochs is None else min(self.plan.epochs, self.epoch + int(epochs))
        start = time.time() - self.elapsed       # `Time` accumulates across a resume
        while self.epoch < last:
            for _ in range(self.plan.episodes_per_epoch):
                self._episode()
            self._end_epoch(self.epoch + 1, start)

    def _end_epoch(self, k: int, start: float) -> None:
        """run.py:102-127 in its order: evaluation, lr_scheduler, checkpoint, films, checks, the row, then state.pt."""
        args, lr, log = self.args, self.learner, self.logger
        first = self.rank == 0                           # data-parallel: rank 0 evaluates and writes, every rank checks and merges
        if first:
            self.evaluation()
        if lr.anneal_lr:
            lr.lr_scheduler.step()
        saving = k % int(args.save_freq) == 0
        if first and (saving or k == self.plan.epochs):
            lr.save_checkpoint(os.path.join(self.output_dir, f"checkpoint_epoch{k}.pt"), stamp=dict(epoch=k, t=self.interacts - 1))
        host = None
        if first and saving:
            host = self.film.numpy()
            for n in range(self.film.episodes):
                self.film.write(os.path.join(self.output_dir, f"epoch{k}_episode{n}"), n, host=host)
        self.replay.check()
        if first:
            self.film.check(host)
        if self.collective:
            import torch.distributed as dist
            self._check_replicas(k)
            row = self.stats.summary(self.group or dist.group.WORLD)     # all ranks' values: one all-gather of the accumulators
        else:
            row = self.stats.summary()                   # the one device-to-host copy of the epoch's statistics
        self.elapsed = time.time() - start
        if first:
            log.summary = row
            log.log_tabular("Epoch", k)
            log.log_tabular("Episode", self.replays * self.env.B * self.world)
            for key, mm, avg in ROW_KEYS[self.single]:
                log.log_tabular(key, with_min_and_max=mm, average_only=avg)
            log.log_tabular("TotalEnvInteracts", self.interacts)
            log.log_tabular("LossQ", average_only=True)  # nan in an epoch without an update (the reference would raise there)
            if self.single:                              # the schedule counts a rank's OWN interactions (graphs.Episode: +E per step)
                log.log_tabular("ExploreEps", eps_thres(self.interacts // self.world - 1, float(args.decay_steps)))
            log.log_tabular("Time", self.elapsed)
            log.dump_tabular()
        self.stats.reset()
        if row["NonFiniteLossQ"] > 0:
            raise TrainingDiverged(f"epoch {k}: {row['NonFiniteLossQ']} of {row['NonFiniteLossQ'] + row['NLossQ']} updates returned a "
                                   f"non-finite LossQ; the row was written, state.pt was not")
        self.epoch = k
        self._save_state()

    def _check_replicas(self, k: int) -> None:
        """An exact checksum of the flat parameter buffer (its bits as int32, summed in int64) from every rank: what bench.py reports
        as ``replicas_identical``, enforced once per epoch."""
        import torch as th
        sums = _gather_ints(self.learner.flat.flat.view(th.int32).sum(dtype=th.int64), self.args.device, self.group)
        if len(set(sums)) != 1:
            raise ReplicasDiverged(f"epoch {k}: the ranks' parameters differ (checksums in rank order: {sums}); the row and the state "
                                   f"files were not written")


# ---- command line (run.py:181-195) ----------------------------------------------------------------------------------------------------
def _parse_env(exp: str, text: str):
    """exp2 / exp3: a map id.  exp1: 'GxS' (n_grps x gts_per_grp, run_exp1.py: 2x5, 3x5, 4x5)."""
    if exp != "exp1":
        return text
    from .sim import SingleUbsParams
    try:
        g, s = (int(v) for v in text.lower().split("x"))
    except ValueError:
        raise SystemExit(f"--env {text!r}: exp1 expects n_grps x gts_per_grp, e.g. 4x5")
    return SingleUbsParams(n_grps=g, gts_per_grp=s)


def _parser():
    import argparse
    ap = argparse.ArgumentParser(prog="python -m uav_bs_ctrl_amd.run", description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", required=True, help="the run directory")
    ap.add_argument("--resume", action="store_true", help="go on from OUT/state.pt (every other option is read from OUT/config.json)")
    ap.add_argument("--exp", choices=EXPS)
    ap.add_argument("--env", help="exp2 / exp3: a map id (sim.MAPS); exp1: n_grps x gts_per_grp, e.g. 4x5")
    ap.add_argument("--args-json", help="a JSON file holding the complete arguments (README)")
    ap.add_argument("--seed", "-s", type=int, default=0)
    ap.add_argument("--envs", type=int, default=32, help="training environments per replay")
    ap.add_argument("--test-envs", type=int, default=None)
    ap.add_argument("--updates-per-segment", type=int, default=1)
    ap.add_argument("--exp-name", default=None)
    ap.add_argument("--eager", action="store_true", help="graphs.Episode / Evaluation instead of their graphs")
    ap.add_argument("--no-save-replay", action="store_true")
    ap.add_argument("--compact-replay", action="store_true",
                    help="exp2 / exp3: the ring stores simulator state and rebuilds the observations (replay.CompactSequenceReplay)")
    ap.add_argument("--prioritized", type=float, nargs=4, default=None, metavar=("ALPHA", "BETA", "ETA", "EPS"),
                    help="proportional prioritised replay over sequences: priority exponent, importance-weight exponent, max/mean mix "
                         "of |TD| per sequence, and the constant added before the exponent (no defaults: four numbers)")
    ap.add_argument("--returns", nargs=2, default=None, metavar=("KIND", "VALUE"),
                    help="multi-step TD targets over the stored sequence: 'nstep N' (integer N >= 1) or 'lambda LAM' (0 <= LAM <= 1); "
                         "without it the reference's one-step target")
    ap.add_argument("--noisy", type=float, default=None, metavar="SIGMA0",
                    help="noisy-net Q head (factorised Gaussian, sigma = SIGMA0 / sqrt(hidden_size)): per-row draws in the rollouts, one "
                         "draw per network and update, the means in evaluations (no default: a number)")
    ap.add_argument("--quantiles", type=int, default=None, metavar="K", choices=(8, 16, 32, 64),
                    help="distributional Q head in quantile-regression form (QR-DQN): K quantiles per action, the quantile-Huber loss on "
                         "one-step or '--returns nstep N' targets; not with --noisy, a dueling head or '--returns lambda'")
    ap.add_argument("--epochs", type=int, default=None, help="run this many more epochs, not all remaining ones")
    ap.add_argument("--dist-backend", choices=("nccl", "gloo"), default="nccl", help="under a launcher that sets RANK: the backend of the group")
    ap.add_argument("--dist-timeout", type=float, default=600.0, help="seconds after which a collective gives up on a missing rank")
    ap.add_argument("--one-device", action="store_true", help="every rank stays on args.device instead of cuda:{LOCAL_RANK}")
    return ap


def main(argv=None) -> None:
    ap = _parser()
    a = ap.parse_args(argv)
    if not a.resume and not (a.exp and a.env and a.args_json):
        ap.error("--exp, --env and --args-json are required without --resume")
    try:
        returns = parse_returns(a.returns) if a.returns is not None else None
    except ValueError as e:
        ap.error(str(e))
    device = _init_distributed(a) if "RANK" in os.environ else None
    try:
        if a.resume:
            run = Run.resume(a.out, device=device)
        else:
            with open(a.args_json) as f:
                args = json.load(f)
            if device is not None:
                args["device"] = device
            run = Run.create(a.exp, _parse_env(a.exp, a.env), args, a.out, exp_name=a.exp_name or a.exp, seed=a.seed, n_envs=a.envs,
                             n_test_envs=a.test_envs, updates_per_segment=a.updates_per_segment, graphed=not a.eager,
                             save_replay=not a.no_save_replay, compact_replay=a.compact_replay, prioritized=a.prioritized,
                             returns=returns, noisy=a.noisy, quantiles=a.quantiles)
        run.train(a.epochs)
        if run.rank == 0:
            print(f"{a.out}: epoch {run.epoch} of {run.plan.epochs}, {run.interacts} interactions, {run.elapsed:.1f} s")
    finally:
        if "RANK" in os.environ:
            import torch.distributed as dist
            if dist.is_initialized():
                dist.destroy_process_group()


def _init_distributed(a) -> Optional[str]:
    """A process started by ``python -m torch.distributed.run`` (RANK in its environment) initialises the group itself; returns the
    device of this rank, ``cuda:{LOCAL_RANK}``, or None with ``--one-device`` (every rank on ``args.device``: world-size-2 tests on one
    GPU over gloo)."""
    import datetime
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # RCCL across processes: dmabuf IPC, set before the first HIP call
    import torch as th
    import torch.distributed as dist
    device = None if a.one_device else f"cuda:{int(os.environ.get('LOCAL_RANK', 0))}"
    if device is not None:
        th.cuda.set_device(device)
    kw = dict(timeout=datetime.timedelta(seconds=a.dist_timeout))
    if a.dist_backend == "nccl" and device is not None:
        kw["device_id"] = th.device(device)
    dist.init_process_group(a.dist_backend, **kw)
    return device


if __name__ == "__main__":
    main()
