"""``train()`` of the reference's two ``run.py`` (algos/madrqn/run.py:22-129, algos/drqn/run.py:22-125) over the device loop: epochs,
log rows, checkpoints, trajectory films and resume.

    run = Run.create(exp="exp3", env="8ubs", args=args, output_dir="data/exp3_8ubs_s0", seed=0, n_envs=32)
    run.train()                          # all remaining epochs; run.train(epochs=k): k more
    run = Run.resume("data/exp3_8ubs_s0")    # rebuilds everything from config.json + state.pt and goes on, bit for bit
    python -m uav_bs_ctrl_amd.run --exp exp3 --env 8ubs --args-json args.json --out data/exp3_8ubs_s0 [--seed 0 --envs 32 --resume --eager]

This is host orchestration over launches that exist: a collect-only and a training ``graphs.GraphedEpisode``, one
``graphs.GraphedEvaluation`` with a ``film.Film``, one ``stats.EpochStats``.  It adds no launch and no host synchronisation to an
episode or to an evaluation; per epoch it adds one ``EpochStats.summary()`` copy, ``replay.check()``, ``film.check()`` and file I/O.

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
    update_after_eff: int       # run.py:56: max(update_after, batch_size * T)
    update_every: int           # run.py:57: T
    steps_per_episode: int      # interactions of one episode replay: E * episode_limit
    episodes_per_epoch: int     # ceil(steps_per_epoch / steps_per_episode)
    interacts_per_epoch: int    # what an epoch actually runs: episodes_per_epoch * steps_per_episode
    epochs: int

    def collect_only(self, interactions_before: int) -> bool:
        """An episode replay is collect-only iff the interactions before it are fewer than ``update_after_eff``."""
        return interactions_before < self.update_after_eff


def plan(args, E: int, episode_limit: int, T: int) -> Plan:
    """The numbers of run.py:55-57 and their counterparts for E environments that end their episodes together.  Pure host arithmetic."""
    g = (lambda k: args[k]) if isinstance(args, dict) else (lambda k: getattr(args, k))
    E, episode_limit, T = int(E), int(episode_limit), int(T)
    if E < 1 or episode_limit < 1 or T < 1:
        raise ValueError("plan: E, episode_limit and T must be positive")
    per_episode = E * episode_limit
    episodes = -(-int(g("steps_per_epoch")) // per_episode)
    return Plan(int(g("steps_per_epoch")) * int(g("epochs")), max(int(g("update_after")), int(g("batch_size")) * T), T, per_episode,
                episodes, episodes * per_episode, int(g("epochs")))


def eps_thres(t: int, decay_steps: float) -> float:
    """run.py:61 on the host (the ``ExploreEps`` column of exp1; the device loop evaluates uavgnn_eps_schedule)."""
    return max(EPS_END, -(EPS_START - EPS_END) / decay_steps * t + EPS_START)


def derive_seeds(seed: int) -> Dict[str, int]:
    """The seeds of a run's random states, all from ``seed``: torch's generator (parameter initialisation), the two simulators' placement
    samplers, the replay's sampler, the exploration pair, the evaluation's pair, the DiscreteComm noise (+ the module's index)."""
    base = 1000003 * int(seed)
    return dict(torch=int(seed), train_env=base + 1, test_env=base + 2, replay=base + 3, explore=base + 4, evaluation=base + 5,
                comm=base + 16)


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


# ---- the driver -------------------------------------------------------------------------------------------------------------------------
class Run:
    """One training run and its directory.  Build it with ``Run.create`` or ``Run.resume``.

    Attributes a caller may read: ``learner``, ``env`` / ``test_env`` (the training and the evaluation simulator), ``replay``, ``stats``,
    ``film``, ``collect`` / ``train_episode`` (the collect-only and the training episode), ``evaluation``, ``plan``, ``seeds``, and the
    host counters ``epoch`` (epochs finished), ``replays`` (episode replays finished), ``interacts``, ``elapsed``."""

    def __init__(self, ours: dict, args: SimpleNamespace, output_dir: str, exp_name: Optional[str], resuming: bool):
        import torch as th

        from .film import Film
        from .graphs import INFO_KEYS, Episode, Evaluation, GraphedEpisode, GraphedEvaluation
        from .learner import MultiAgentQLearner, QLearner
        from .replay import SequenceReplay, SingleUbsSequenceReplay
        from .sim import BatchedSingleUbsCoverageEnv, BatchedUbsCoverageEnv
        from .stats import EpochStats
        self.ours, self.args, self.output_dir, self.exp_name = ours, args, output_dir, exp_name
        exp, E, seeds = ours["exp"], int(ours["n_envs"]), ours["seeds"]
        self.exp, self.single, self.seeds, self.save_replay = exp, exp == "exp1", seeds, bool(ours["save_replay"])
        E_test = int(ours["n_test_envs"])
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
        self.enc, self.env, self.test_env = enc, make(E, "train_env"), make(E_test, "test_env")
        env, test_env = self.env, self.test_env
        th.manual_seed(seeds["torch"])           # parameter initialisation
        self.learner = learner = (QLearner if self.single else MultiAgentQLearner)(env.get_env_info(enc), args)
        if learner.needs_collective():
            raise ValueError("a data-parallel run is not covered: the episode graphs hold the whole update (graphs.GraphedEpisode)")
        seed_comm_modules(learner, seeds["comm"])
        T = int(args.max_seq_len) if args.max_seq_len else env.episode_limit
        self.plan = plan(args, E, env.episode_limit, T)
        if self.single:
            self.replay = SingleUbsSequenceReplay(int(args.replay_size), T, env.n_gts, args.hidden_size, n_envs=E, device=dev,
                                                  device_state=True, seed=seeds["replay"])
        else:
            self.replay = SequenceReplay(int(args.replay_size), T, env.n_agents, env.n_gts, args.hidden_size, n_envs=E,
                                         r_comm=env.p.r_comm, rew_dim=1 if args.share_reward else None, device=dev,
                                         device_state=True, seed=seeds["replay"])
        graphed = bool(ours["graphed"])
        ep_cls, ev_cls = (GraphedEpisode, GraphedEvaluation) if graphed else (Episode, Evaluation)
        kw = dict(eps=(EPS_START, EPS_END, float(args.decay_steps)), updates_per_segment=int(ours["updates_per_segment"]), enc=enc)
        self.info_keys = tuple(k for k in INFO_KEYS if not (self.single and k == "ProbCollision"))
        self.stats = EpochStats(list(self.info_keys) + ["LossQ"] + ["Test" + k for k in self.info_keys], dev, cap=max(64, E, E_test))
        self.film = Film(test_env, int(args.num_test_episodes))
        # the three captures run on the fresh, empty state - also when resuming: a warm-up episode commits into the ring at the restored
        # head, so captured after a full ring was loaded it would overwrite the oldest sequences.  `_load_state` copies IN PLACE afterwards
        self.collect = ep_cls(learner, env, self.replay, int(args.batch_size), train=False, stats=self.stats,
                              explore_seed=seeds["explore"], **kw)
        self.train_episode = ep_cls(learner, env, self.replay, int(args.batch_size), train=True, stats=self.stats,
                                    explore_seed=seeds["explore"], **kw)
        self.evaluation = ev_cls(learner, test_env, int(args.num_test_episodes), eps=TEST_EPS, seed=seeds["evaluation"], enc=enc,
                                 stats=self.stats, film=self.film)
        self.epoch = self.replays = self.interacts = 0
        self.elapsed = 0.0
        self.active = "collect"          # the episode object whose `t` / `explore` are current
        self.ring_base = 0               # interactions when the ring was last empty: training starts update_after_eff later
        self.logger = RunLogger(output_dir, exp_name, append=resuming)

    # ---- construction -------------------------------------------------------------------------------------------------------------
    @classmethod
    def create(cls, exp: str, env, args, output_dir: str, exp_name: Optional[str] = None, seed: int = 0, n_envs: int = 32,
               n_test_envs: Optional[int] = None, updates_per_segment: int = 1, graphed: bool = True, save_replay: bool = True) -> "Run":
        """Builds simulators, learner, replay, statistics, film and the three graphs (``graphed=False``: their eager forms) as
        run.py:47-61 builds them and writes ``config.json``; sets torch's generator (``torch.manual_seed(seed)``, as the reference's
        ``set_rand_seed`` does) for the parameter initialisation.  env: a map id of ``sim.MAPS`` or a ``MapSpec`` (exp2 / exp3), a
        ``SingleUbsParams`` (exp1).  n_test_envs: evaluation environments (default ``num_test_episodes``; must divide it).
        save_replay=False: ``state.pt`` leaves the ring out (gigabytes at exp3 sizes); a resumed run then collects ``update_after_eff``
        interactions again before it trains and is NOT bit-identical to an uninterrupted one."""
        ns = check_args(exp, args)
        ours = dict(exp=exp, env=_env_to_config(exp, env), n_envs=int(n_envs),
                    n_test_envs=int(ns.num_test_episodes if n_test_envs is None else n_test_envs),
                    updates_per_segment=int(updates_per_segment), graphed=bool(graphed), save_replay=bool(save_replay),
                    seeds=derive_seeds(seed))
        run = cls(ours, ns, output_dir, exp_name, resuming=False)
        env_fn, env_kwargs = _reference_env(exp, env)
        config = dict(env_fn=env_fn, env_kwargs=env_kwargs, seed=int(seed), args=ns, uav_bs_ctrl_amd=ours)
        run.logger.save_config(config)
        for name in ("state.pt", "state.pt.tmp"):            # a new run in an old directory must not be resumable from the old state
            if os.path.exists(os.path.join(output_dir, name)):
                os.remove(os.path.join(output_dir, name))
        return run

    @classmethod
    def resume(cls, output_dir: str) -> "Run":
        """Rebuilds the run of ``output_dir`` from ``config.json`` exactly as ``create`` built it - captures included, on the fresh
        state - then copies ``state.pt`` in place into the tensors the graphs hold addresses of, and re-opens ``progress.txt`` for
        append.  Raises ``RunDirectoryError`` for a directory without ``state.pt``, a ``config.json`` that does not rebuild the saved
        shapes, and a run that is already complete."""
        import torch as th
        cfg_path, state_path = os.path.join(output_dir, "config.json"), os.path.join(output_dir, "state.pt")
        if not os.path.exists(state_path):
            raise RunDirectoryError(f"{output_dir}: no state.pt - nothing to resume (no epoch of this run was finished, or it is not a "
                                    f"run directory of this package)")
        try:
            with open(cfg_path) as f:
                config = json.load(f)
            ours = config["uav_bs_ctrl_amd"]
            ns = check_args(ours["exp"], next(iter(config["args"].values())))
        except (OSError, KeyError, ValueError, StopIteration, AttributeError, TypeError) as e:
            raise RunDirectoryError(f"{output_dir}: config.json does not describe a run of this package ({type(e).__name__}: {e})") from e
        state = th.load(state_path, map_location="cpu")
        if int(state["epoch"]) >= int(ns.epochs):
            raise RunDirectoryError(f"{output_dir}: the run is already complete ({state['epoch']} of {ns.epochs} epochs)")
        run = cls(ours, ns, output_dir, config.get("exp_name"), resuming=True)
        run._load_state(state)
        return run

    # ---- state.pt -------------------------------------------------------------------------------------------------------------------
    def _tensors(self) -> Dict[str, object]:
        """name -> the live tensor a graph holds the address of."""
        lr, rb, opt = self.learner, self.replay, self.learner.optimizer
        out = {"learner.flat": lr.flat.flat, "learner.flat_target": lr.flat_target, "learner.m": opt.m, "learner.v": opt.v,
               "learner.hyper": opt.hyper, "replay.state": rb.state, "replay.rng": rb.rng, "replay.status": rb.status,
               "env.rng": self.env.rng if self.single else self.env.map_rng,
               "test_env.rng": self.test_env.rng if self.single else self.test_env.map_rng, "evaluation.rng": self.evaluation.rng}
        for name, ep in (("collect", self.collect), ("train", self.train_episode)):
            out.update({f"{name}.t": ep.t, f"{name}.eps": ep.eps, f"{name}.explore": ep.explore})
        out.update({"comm." + name: m.rng_state for name, m in comm_modules(lr)})
        return out

    def _save_state(self) -> None:
        """Written to a temporary name and renamed: a killed job leaves the previous state intact."""
        import torch as th
        lr = self.learner
        state = dict(version=STATE_VERSION, epoch=self.epoch, replays=self.replays, interacts=self.interacts, elapsed=self.elapsed,
                     active=self.active, ring_base=self.ring_base, lr=float(lr.optimizer.param_groups[0]["lr"]),
                     lr_scheduler=lr.lr_scheduler.state_dict() if lr.anneal_lr else None,
                     tensors={k: v.detach().cpu() for k, v in self._tensors().items()}, mem=None)
        if self.save_replay:
            size = int(state["tensors"]["replay.state"][1])
            state["mem"] = {k: v[:size].cpu() for k, v in self.replay.mem.items()}
        tmp = os.path.join(self.output_dir, "state.pt.tmp")
        th.save(state, tmp)
        os.replace(tmp, os.path.join(self.output_dir, "state.pt"))

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
            raise RunDirectoryError(f"{self.output_dir}: config.json does not rebuild the shapes state.pt holds (version "
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
        self.evaluation()
        if lr.anneal_lr:
            lr.lr_scheduler.step()
        saving = k % int(args.save_freq) == 0
        if saving or k == self.plan.epochs:
            lr.save_checkpoint(os.path.join(self.output_dir, f"checkpoint_epoch{k}.pt"), stamp=dict(epoch=k, t=self.interacts - 1))
        host = None
        if saving:
            host = self.film.numpy()
            for n in range(self.film.episodes):
                self.film.write(os.path.join(self.output_dir, f"epoch{k}_episode{n}"), n, host=host)
        self.replay.check()
        self.film.check(host)
        log.summary = row = self.stats.summary()         # the one device-to-host copy of the epoch's statistics
        log.log_tabular("Epoch", k)
        log.log_tabular("Episode", self.replays * self.env.B)
        for key, mm, avg in ROW_KEYS[self.single]:
            log.log_tabular(key, with_min_and_max=mm, average_only=avg)
        log.log_tabular("TotalEnvInteracts", self.interacts)
        log.log_tabular("LossQ", average_only=True)      # nan in an epoch without an update (the reference would raise there)
        if self.single:
            log.log_tabular("ExploreEps", eps_thres(self.interacts - 1, float(args.decay_steps)))
        self.elapsed = time.time() - start
        log.log_tabular("Time", self.elapsed)
        log.dump_tabular()
        self.stats.reset()
        if row["NonFiniteLossQ"] > 0:
            raise TrainingDiverged(f"epoch {k}: {row['NonFiniteLossQ']} of {row['NonFiniteLossQ'] + row['NLossQ']} updates returned a "
                                   f"non-finite LossQ; the row was written, state.pt was not")
        self.epoch = k
        self._save_state()


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


def main(argv=None) -> None:
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
    ap.add_argument("--epochs", type=int, default=None, help="run this many more epochs, not all remaining ones")
    a = ap.parse_args(argv)
    if a.resume:
        run = Run.resume(a.out)
    else:
        if not (a.exp and a.env and a.args_json):
            ap.error("--exp, --env and --args-json are required without --resume")
        with open(a.args_json) as f:
            args = json.load(f)
        run = Run.create(a.exp, _parse_env(a.exp, a.env), args, a.out, exp_name=a.exp_name or a.exp, seed=a.seed, n_envs=a.envs,
                         n_test_envs=a.test_envs, updates_per_segment=a.updates_per_segment, graphed=not a.eager,
                         save_replay=not a.no_save_replay)
    run.train(a.epochs)
    print(f"{a.out}: epoch {run.epoch} of {run.plan.epochs}, {run.interacts} interactions, {run.elapsed:.1f} s")


if __name__ == "__main__":
    main()
