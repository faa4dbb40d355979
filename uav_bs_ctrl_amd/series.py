"""``test_series`` of the reference's ``test_policies.py`` (:36-104) on the device: one named checkpoint of every run directory under a
list of log directories is evaluated, the seeds of an experiment name are merged, and ``test_summary.csv``, ``test_summary_t.csv`` and a
box plot are written - the stage between training the arms (``run.Run``) and plotting.

    rsts = test_series(["EpRet", "FairIdx"], ["data/exp3_8ubs_tarmac", "data/exp3_8ubs_disc"], "checkpoint_epoch100.pt", 10, "data/test_exp3/8ubs")
    python -m uav_bs_ctrl_amd.series --logdirs A B ... --checkpoint checkpoint_epoch50.pt --episodes 10 \
        --metrics EpRet AvgGlobalUtility TotalThroughput FairIdx --out DIR [--envs E --device cuda --eager]

    d = describe("data/exp3_8ubs_tarmac/s0")         # RunDescription of a directory written by ``Run`` OR by the reference's logger
    runner = PolicyRunner(d, n_episodes=10)          # simulator, learner, film and ONE captured evaluation for d.key
    table = runner("data/exp3_8ubs_tarmac/s0/checkpoint_epoch100.pt", d.seed, "films/s0")     # what film.load_and_run_policy returns

This is host orchestration over launches that exist (``graphs.GraphedEvaluation`` with a ``film.Film``): it adds no kernel.  What it
adds on the device side is reuse.  ``film.load_and_run_policy`` warms up and captures a new evaluation per call; a series evaluates many
checkpoints of few configurations (the seeds of an arm differ in nothing that shapes the model or the simulator), so ``test_series``
builds one ``PolicyRunner`` per distinct ``RunDescription.key`` and every run of that key loads its parameters and its seeds IN PLACE
into the tensors the captured graph holds the addresses of.

A directory of the reference (no ``uav_bs_ctrl_amd`` key in ``config.json``) is read by inference from ``env_fn`` / ``env_kwargs`` /
``args`` - the inverse of ``run._reference_env``.  ``args.mixer`` becomes False: an evaluation needs no mixer, and the runner loads
``model_state_dict`` alone (``load_policy``: a QMIX checkpoint's optimiser state holds the mixer's parameters and would not load into a
learner without one), so a ``none_qmix`` checkpoint the reference trained is evaluated like any other.

Seeds: the runner takes everything random from ``run.derive_seeds(seed)`` - ``test_env`` (the placements), ``evaluation`` (the
selection's uniforms), ``comm`` (DiscreteComm's noise, + the module's index).  A ``comm_rng_state`` a checkpoint carries - the position
of the TRAINING run's noise stream - is not read (``film.load_and_run_policy`` continues from it): the result is a function of the
checkpoint's parameters and the seed alone."""
from __future__ import annotations

import dataclasses
import json
import os
from types import SimpleNamespace
from typing import Dict, List, NamedTuple, Optional, Sequence

import numpy as np

from . import run as R
from .run import RunDirectoryError

MODEL_KEYS = ("o", "c", "agent", "hidden_size", "n_layers", "n_heads", "msg_size", "key_size", "n_rounds", "dueling", "noisy", "quantiles")
SUMMARY, SUMMARY_T, FIGURE = "test_summary.csv", "test_summary_t.csv", "test_summary.png"
INFO_KEYS = ("EpRet", "EpLen", "AvgGlobalUtility", "TotalThroughput", "FairIdx", "ProbCollision")       # graphs.INFO_KEYS, without torch


class RunDescription(NamedTuple):
    exp_name: str               # config.json's (the directory's own name where it holds none)
    seed: int
    exp: str                    # exp1 / exp2 / exp3
    env: object                 # a SingleUbsParams (exp1) or a MapSpec
    enc: str                    # the observation encoder: args.agent (exp1), 'gnn' (exp3), 'mlp' (exp2)
    args: SimpleNamespace
    key: tuple                  # hashable: the environment + the arguments that shape the model; equal keys share one PolicyRunner

    @property
    def single(self) -> bool:
        return self.exp == "exp1"

    @property
    def metrics(self) -> tuple:
        """The columns of this run's table (``graphs.info_keys``)."""
        return INFO_KEYS[:-1] if self.single else INFO_KEYS


# ---- reading a run directory --------------------------------------------------------------------------------------------------------------
def _reference_exp_env(run_dir: str, config: dict, args: dict):
    """(exp, env) of a directory the reference's logger wrote: the inverse of ``run._reference_env``."""
    from .sim import MAPS, SingleUbsParams
    env_fn, kw = config.get("env_fn"), dict(config.get("env_kwargs") or {})
    if env_fn == "SingleUbsCoverageEnv":
        try:
            return "exp1", SingleUbsParams(**{k: R._tuples(v) for k, v in kw.items()})
        except TypeError as e:
            raise RunDirectoryError(f"{run_dir}: config.json's env_kwargs do not describe a SingleUbsCoverageEnv ({e})") from e
    if env_fn != "MultiUbsCoverageEnv":
        raise RunDirectoryError(f"{run_dir}: unknown env_fn {env_fn!r} in config.json: SingleUbsCoverageEnv or MultiUbsCoverageEnv expected")
    map_id = kw.get("map_id")
    if not isinstance(map_id, str) or map_id not in MAPS:
        raise RunDirectoryError(f"{run_dir}: unknown map_id {map_id!r} in config.json's env_kwargs: one of {sorted(MAPS)}")
    if "o" not in args:
        raise RunDirectoryError(f"{run_dir}: config.json's arguments miss the key o (it tells exp2, 'mlp', from exp3, 'gnn')")
    if args["o"] not in ("gnn", "mlp"):
        raise RunDirectoryError(f"{run_dir}: config.json's args.o = {args['o']!r}: 'gnn' (exp3) or 'mlp' (exp2) expected")
    spec = MAPS[map_id]
    switches = {k: bool(kw[k]) for k in ("fair_service", "avoid_collision") if k in kw}
    return ("exp3" if args["o"] == "gnn" else "exp2"), dataclasses.replace(spec, params=dataclasses.replace(spec.params, **switches))


def describe(run_dir: str, device="cuda") -> RunDescription:
    """Reads ``run_dir/config.json`` of either kind: a directory ``Run`` wrote (key ``uav_bs_ctrl_amd``: ``exp``, ``env`` and the seed
    are taken from there, as ``Run.resume`` does) or one the reference's logger wrote (inferred from ``env_fn``, ``env_kwargs`` and
    ``args.o``).  The arguments are the first value of ``config["args"]`` through ``run.check_args``, with ``device`` replaced by the
    caller's (the reference stores ``cpu`` or ``cuda:0``) and ``mixer`` set to False.  Raises ``RunDirectoryError`` - saying which
    case it is - for a missing or unreadable ``config.json``, an unknown ``env_fn``, an unknown ``map_id`` and a missing argument key."""
    from .sim import MAPS
    path = os.path.join(run_dir, "config.json")
    try:
        with open(path) as f:
            config = json.load(f)
        if not isinstance(config, dict):
            raise ValueError("not a JSON object")
    except (OSError, ValueError) as e:
        raise RunDirectoryError(f"{run_dir}: config.json is missing or unreadable ({type(e).__name__}: {e})") from e
    try:
        args = dict(next(iter(config["args"].values())))
    except (KeyError, StopIteration, AttributeError, TypeError, ValueError) as e:
        raise RunDirectoryError(f"{run_dir}: config.json is unreadable: it holds no arguments under 'args' ({type(e).__name__}: {e})") from e
    ours = config.get("uav_bs_ctrl_amd")
    if ours is not None:
        try:
            exp, env, seed = ours["exp"], R._env_from_config(ours["env"]), int(ours["seeds"]["torch"])
            if isinstance(env, str):
                env = MAPS[env]
        except (KeyError, TypeError, ValueError) as e:
            raise RunDirectoryError(f"{run_dir}: config.json is unreadable: its uav_bs_ctrl_amd entry does not describe a run "
                                    f"({type(e).__name__}: {e})") from e
    else:
        exp, env = _reference_exp_env(run_dir, config, args)
        try:
            seed = int(config["seed"])
        except (KeyError, TypeError, ValueError) as e:
            raise RunDirectoryError(f"{run_dir}: config.json is unreadable: it holds no seed ({type(e).__name__}: {e})") from e
    if exp not in R.EXPS:
        raise RunDirectoryError(f"{run_dir}: config.json is unreadable: exp = {exp!r}, one of {R.EXPS} expected")
    if "mixer" in args:
        args["mixer"] = False
    missing = [k for k in R.LEARNER_KEYS[exp] + R.DRIVER_KEYS if k not in args]
    if missing:
        raise RunDirectoryError(f"{run_dir}: config.json's arguments miss the key{'s' if len(missing) > 1 else ''} {', '.join(missing)} "
                                f"({exp}; the package holds no defaults)")
    try:
        ns = R.check_args(exp, args)
    except ValueError as e:
        raise RunDirectoryError(f"{run_dir}: config.json's arguments are refused ({e})") from e
    ns.device, ns.mixer = str(device), False
    if ours is not None and ours.get("noisy") is not None:
        # the run trained the noisy-net Q head (``Run.create(noisy=sigma0)``): the learner builds it, the checkpoint's sigmas load into it,
        # and the evaluation - like every evaluation - uses the means
        try:
            ns.noisy = R._noisy(ours["noisy"])
        except ValueError as e:
            raise RunDirectoryError(f"{run_dir}: config.json is unreadable: {e}") from e
    if ours is not None and ours.get("quantiles") is not None:
        # the run trained the quantile-regression Q head (``Run.create(quantiles=K)``): the learner builds it, the checkpoint's
        # [n_actions * K, H] head loads into it, and the evaluation acts on the quantile means
        try:
            ns.quantiles = R._quantiles(ours["quantiles"])
        except ValueError as e:
            raise RunDirectoryError(f"{run_dir}: config.json is unreadable: {e}") from e
    if exp == "exp1":
        enc = ns.agent
    else:
        enc = "gnn" if exp == "exp3" else "mlp"
        if ns.o != enc:
            raise RunDirectoryError(f"{run_dir}: config.json describes {exp}, which runs the {enc!r} observation encoder, with args.o = {ns.o!r}")
    env_key = json.dumps(dataclasses.asdict(env), sort_keys=True)
    key = (exp, env_key) + tuple((k, _hashable(getattr(ns, k, None))) for k in MODEL_KEYS)
    exp_name = config.get("exp_name") or os.path.basename(os.path.normpath(run_dir))
    return RunDescription(str(exp_name), seed, exp, env, enc, ns, key)


def _hashable(v):
    return tuple(_hashable(x) for x in v) if isinstance(v, (list, tuple)) else v


# ---- one captured evaluation for every checkpoint of a configuration -------------------------------------------------------------------
def load_policy(learner, model_path: str) -> dict:
    """What an evaluation needs of a checkpoint: ``model_state_dict`` into ``learner.policy_net``, copied IN PLACE into the parameters
    (on the device: the views of the learner's flat buffer a captured graph reads).  Unlike ``learner.load_checkpoint`` it reads
    neither the optimiser's state - a checkpoint trained WITH a mixer holds the mixer's parameters in the optimiser's one group, which a
    learner without a mixer cannot load - nor ``mixer_state_dict``, the scheduler or ``comm_rng_state``, and it replaces no tensor.
    Returns the checkpoint's stamp {epoch, t}."""
    import torch as th

    from . import _lib as L
    ck = th.load(model_path, map_location=learner.device)
    if "model_state_dict" not in ck:
        raise RunDirectoryError(f"{model_path}: no model_state_dict: not a checkpoint of learner.save_checkpoint or of the reference")
    learner.invalidate_weight_cache()
    learner.policy_net.load_state_dict(ck["model_state_dict"])
    flat = getattr(learner, "flat", None)
    if flat is not None and not flat.intact():
        raise L.UavGnnError(f"{model_path}: loading the checkpoint moved a parameter out of the learner's flat buffer")
    return dict(epoch=ck.get("epoch"), t=ck.get("t"))


class PolicyRunner:
    """Everything ``film.load_and_run_policy`` needs, built ONCE for a ``RunDescription``: the evaluation simulator with ``n_envs``
    environments (default ``n_episodes``; must divide it), a learner, a ``Film`` of ``n_episodes`` episodes and one
    ``GraphedEvaluation`` (``graphed=False``: ``Evaluation``) at the reference's test-time exploration rate.

        table = runner(model_path, seed, output_dir=None)

    loads the checkpoint's policy in place (``load_policy``), sets the simulator's reset pair, the evaluation's pair and every DiscreteComm ``rng_state`` in
    place from ``run.derive_seeds(seed)``, replays, checks the film, writes ``output_dir/episode{k}/`` and returns what
    ``load_and_run_policy`` returns.  The result is a function of (checkpoint, seed) only: nothing the runner evaluated before
    enters it.  ``calls`` counts the evaluations."""

    def __init__(self, description: RunDescription, n_episodes: int, n_envs: Optional[int] = None, graphed: bool = True):
        from .film import Film
        from .graphs import Evaluation, GraphedEvaluation
        from .learner import MultiAgentQLearner, QLearner
        from .sim import BatchedSingleUbsCoverageEnv, BatchedUbsCoverageEnv
        d = self.description = description
        self.n_episodes = int(n_episodes)
        n_envs = self.n_episodes if n_envs is None else int(n_envs)
        if self.n_episodes < 1 or n_envs < 1 or self.n_episodes % n_envs != 0:
            raise ValueError(f"n_envs = {n_envs} must divide n_episodes = {n_episodes} (both positive)")
        dev = d.args.device
        if d.single:
            self.env = BatchedSingleUbsCoverageEnv(d.env, n_envs, dev, seed=0)
        else:
            self.env = BatchedUbsCoverageEnv.from_map(d.env, n_envs, dev, seed=0)
        self.learner = (QLearner if d.single else MultiAgentQLearner)(self.env.get_env_info(d.enc), d.args)
        # every comm module gets its rng_state tensor NOW: the capture below holds its address, a call copies the seed into it
        R.seed_comm_modules(self.learner, 0)
        self._comm = [(m, m.rng_state) for _, m in R.comm_modules(self.learner)]
        self.film = Film(self.env, self.n_episodes)
        self.evaluation = (GraphedEvaluation if graphed else Evaluation)(self.learner, self.env, self.n_episodes, eps=R.TEST_EPS, seed=0,
                                                                         enc=d.enc, film=self.film)
        self.calls = 0

    def _set_pair(self, pair, seed: int) -> None:
        import torch as th
        pair.copy_(th.tensor([int(seed), 0], dtype=th.int64))

    def __call__(self, model_path: str, seed: int, output_dir: Optional[str] = None) -> Dict[str, np.ndarray]:
        lr, ev, film = self.learner, self.evaluation, self.film
        load_policy(lr, model_path)
        seeds = R.derive_seeds(seed)
        self._set_pair(self.env.reset_rng, seeds["test_env"])
        self._set_pair(ev.rng, seeds["evaluation"])
        for i, (_, held) in enumerate(self._comm):
            self._set_pair(held, seeds["comm"] + i)
        film.clear()
        ev()
        self.calls += 1
        table = ev.table.cpu().numpy()
        host = film.numpy()
        film.check(host)
        if output_dir is not None:
            for k in range(self.n_episodes):
                film.write(os.path.join(output_dir, f"episode{k}"), k, host=host)
        return {key: np.array(table[i, :self.n_episodes], dtype=np.float64) for i, key in enumerate(ev.keys)}


# ---- the summary tables ----------------------------------------------------------------------------------------------------------------
def insert_data(dataset: Dict[str, Dict[str, np.ndarray]], exp_name: str, new_data: Dict[str, np.ndarray]) -> Dict[str, Dict[str, np.ndarray]]:
    """test_policies.py:20-33: the results under one experiment name are concatenated in the order they arrive."""
    have = dataset.setdefault(exp_name, {})
    for k, v in new_data.items():
        v = np.asarray(v, dtype=np.float64)
        have[k] = np.concatenate([have[k], v]) if k in have else v
    return dataset


def _cell(column: np.ndarray, i: int) -> str:
    """``repr`` of the float64 value; nothing past the column's end and for NaN (pandas' ``na_rep``)."""
    if i >= len(column) or column[i] != column[i]:
        return ""
    return repr(float(column[i]))


def _rows(dataset, metrics) -> int:
    return max(len(dataset[e][m]) for e in dataset for m in metrics)


def summary_text(dataset: Dict[str, Dict[str, np.ndarray]], metrics: Sequence[str]) -> str:
    """The text of ``test_summary.csv`` (test_policies.py:72-82): a ``metric`` and an ``exp_name`` header line, the columns sorted
    by (metric, exp_name), one row per episode index, an empty cell where an experiment has fewer episodes."""
    cols = sorted({(m, e) for e in dataset for m in metrics})
    lines = [["metric"] + [m for m, _ in cols], ["exp_name"] + [e for _, e in cols]]
    lines += [[str(i)] + [_cell(dataset[e][m], i) for m, e in cols] for i in range(_rows(dataset, metrics))]
    return "".join(",".join(r) + "\n" for r in lines)


def summary_t_text(dataset: Dict[str, Dict[str, np.ndarray]], metrics: Sequence[str]) -> str:
    """The text of ``test_summary_t.csv`` (test_policies.py:84-91): an ``exp_name`` and an ``episode`` header line, one row per
    metric in the caller's order, the experiments in first-seen order, each as wide as the longest."""
    n = _rows(dataset, metrics)
    lines = [["exp_name"] + [e for e in dataset for _ in range(n)], ["episode"] + [str(i) for _ in dataset for i in range(n)]]
    lines += [[m] + [_cell(dataset[e][m], i) for e in dataset for i in range(n)] for m in metrics]
    return "".join(",".join(r) + "\n" for r in lines)


def _box_plot(path: str, dataset, metrics) -> bool:
    """test_policies.py:93-103 with the Agg backend and without ``show``: one box plot per metric on a two-column grid.  False when
    matplotlib is not installed."""
    try:
        import matplotlib
        matplotlib.use("Agg", force=False)
        import matplotlib.pyplot as plt
    except ImportError:
        return False
    n_rows = 2
    while 2 * n_rows < len(metrics):
        n_rows += 1
    fig, axes = plt.subplots(nrows=n_rows, ncols=2, figsize=(6, 4))
    fig.subplots_adjust(wspace=0.35, hspace=0.5)
    names = sorted(dataset)
    for i, m in enumerate(metrics):
        ax = axes[i // 2, i % 2]
        columns = [dataset[e][m][np.isfinite(dataset[e][m])] for e in names]
        try:
            ax.boxplot(columns, tick_labels=names)
        except TypeError:                                # matplotlib < 3.9 names the argument `labels`
            ax.boxplot(columns, labels=names)
        ax.set_title(m)
    fig.savefig(path)
    plt.close(fig)
    return True


def find_runs(all_logdirs: Sequence[str], checkpoint: str) -> List[str]:
    """Every directory under ``all_logdirs`` whose files include ``checkpoint``: the log directories in the given order, each walked
    with sorted directory names (the reference takes the file system's order)."""
    out = []
    for logdir in all_logdirs:
        for root, dirs, files in os.walk(logdir):
            dirs.sort()
            if checkpoint in files:
                out.append(root)
    return out


def test_series(metrics: Sequence[str], all_logdirs: Sequence[str], checkpoint: str, n_episodes: int, output_dir: str, device="cuda",
                graphed: bool = True, n_envs: Optional[int] = None) -> dict:
    """test_policies.py:36-104: evaluates ``checkpoint`` of every run directory under ``all_logdirs`` (``find_runs``) for
    ``n_episodes`` episodes, films to ``output_dir/{exp_name}_seed{seed}/episode{k}/``, merges the results by ``exp_name`` in visit
    order (``insert_data``) and writes ``test_summary.csv``, ``test_summary_t.csv`` and - when matplotlib can be imported -
    ``test_summary.png`` into ``output_dir``.  One ``PolicyRunner`` per distinct ``RunDescription.key`` serves every run of that key;
    n_envs: its evaluation environments (default ``n_episodes``; must divide it).

    A metric that a run's table does not hold (``ProbCollision`` for exp1) raises ``ValueError`` naming the metric and the directory
    before anything is evaluated or written; a directory ``describe`` refuses raises its ``RunDirectoryError`` then, too.

    Returns {dataset: {exp_name: {key: float64 [episodes]}} (every key of the tables, not only ``metrics``), runs: the number of run
    directories, captures: the number of runners built, run_dirs, summary / summary_t / figure: the paths written (figure: None and
    figure_skipped: the reason, without matplotlib)}."""
    metrics = list(metrics)
    if not metrics:
        raise ValueError("metrics: at least one metric expected")
    run_dirs = find_runs(all_logdirs, checkpoint)
    if not run_dirs:
        raise ValueError(f"no directory under {list(all_logdirs)} holds a file {checkpoint!r}")
    described = [describe(d, device) for d in run_dirs]
    for d, desc in zip(run_dirs, described):
        for m in metrics:
            if m not in desc.metrics:
                raise ValueError(f"metric {m!r} is not in the table of {d} ({desc.exp}: {', '.join(desc.metrics)})")
    runners: Dict[tuple, PolicyRunner] = {}
    dataset: Dict[str, Dict[str, np.ndarray]] = {}
    for d, desc in zip(run_dirs, described):
        if desc.key not in runners:
            runners[desc.key] = PolicyRunner(desc, n_episodes, n_envs=n_envs, graphed=graphed)
        subdir = os.path.join(output_dir, f"{desc.exp_name}_seed{desc.seed}")
        os.makedirs(subdir, exist_ok=True)
        insert_data(dataset, desc.exp_name, runners[desc.key](os.path.join(d, checkpoint), desc.seed, subdir))
    os.makedirs(output_dir, exist_ok=True)
    paths = {k: os.path.join(output_dir, name) for k, name in (("summary", SUMMARY), ("summary_t", SUMMARY_T), ("figure", FIGURE))}
    for k, text in (("summary", summary_text(dataset, metrics)), ("summary_t", summary_t_text(dataset, metrics))):
        with open(paths[k], "w", newline="") as f:
            f.write(text)
    out = dict(dataset=dataset, runs=len(run_dirs), captures=len(runners), run_dirs=run_dirs, summary=paths["summary"],
               summary_t=paths["summary_t"], figure=paths["figure"])
    if not _box_plot(paths["figure"], dataset, metrics):
        out.update(figure=None, figure_skipped="matplotlib is not installed: test_summary.png was not written")
    return out


test_series.__test__ = False            # the reference's name for it; no test for pytest to collect


def main(argv=None) -> None:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m uav_bs_ctrl_amd.series", description=__doc__.split("\n\n")[0])
    ap.add_argument("--logdirs", nargs="+", required=True, help="log directories; every directory under them that holds CHECKPOINT is a run")
    ap.add_argument("--checkpoint", required=True, help="the checkpoint's file name, e.g. checkpoint_epoch50.pt")
    ap.add_argument("--episodes", type=int, default=10)
    ap.add_argument("--metrics", nargs="+", required=True, help=f"columns of the tables: {' '.join(INFO_KEYS)}")
    ap.add_argument("--out", required=True, help="the directory of the films and the summary tables")
    ap.add_argument("--envs", type=int, default=None, help="evaluation environments (default: EPISODES; must divide it)")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--eager", action="store_true", help="graphs.Evaluation instead of its graph")
    a = ap.parse_args(argv)
    out = test_series(a.metrics, a.logdirs, a.checkpoint, a.episodes, a.out, device=a.device, graphed=not a.eager, n_envs=a.envs)
    print(f"{a.out}: {out['runs']} runs of {len(out['dataset'])} experiments, {out['captures']} evaluations built"
          + ("" if out["figure"] else f" ({out['figure_skipped']})"))


if __name__ == "__main__":
    main()
