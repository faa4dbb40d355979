"""Trajectory films of the evaluation simulators: the reference's ``Recorder`` (envs/mubs_cov/recorder.py, envs/subs_cov/recorder.py)
for B device environments, and ``load_and_run_policy`` (algos/madrqn/run.py:132-178, algos/drqn/run.py) on top of it.

The reference builds every evaluation environment with ``record=True``: ``reset`` reloads the recorder with the initial UBS positions
(mubs_cov.py:99-100, subs_cov.py:87-88), every ``step`` clicks the new positions and a few scalars into it (mubs_cov.py:126-127,
subs_cov.py:128-131), and ``replay(save_dir=...)`` writes ``path_ubs.csv``, ``pos_gts.csv``, ``others.csv`` and ``trajectories.png``
(envs/common.py:80-100).  Here the film lives in device memory and one launch per step fills it (csrc/film.hip): the slot comes from
the simulator's own device step counter ``env.t``, so ``reload`` / ``click`` take no host state but the round's first episode index
and capture into the graph of ``GraphedEvaluation``.

    film = Film(test_env, episodes)         # device buffers for `episodes` episodes of test_env's shape; either simulator
    film.reload(env, episode_base)          # after a reset: slot 0 and the GT positions
    film.click(env, actions, episode_base)  # after env.step(actions): slot env.t
    film.check()                            # raises when a click fell outside the film (bit 0 of `status`)
    ep = film.episode(k)                    # dict of NumPy arrays: the reference's film keys (+ pos_gts), one episode
    film.write(save_dir, k, plot=False)     # path_ubs.csv, pos_gts.csv, others.csv of episode k

Film keys          multi-UBS: pos_ubs [T+1, n, 2], fair_idx [T], reward [T] (the team's mean reward)
                   single-UBS: pos_ubs [T+1, 2], global_utility, reward, total_throughput, fair_idx, velocity [T], rate_per_gt [T, M]
Unwritten slots hold NaN (``FILL``).  The whole film - status word included - is ONE device buffer, so reading it back is one copy."""
from __future__ import annotations

import math
import os
from typing import Dict, Optional

import numpy as np
import torch as th

from . import _lib as L

FILL = float("nan")
_SERIES = {False: ("fair_idx", "reward"),
           True: ("total_throughput", "fair_idx", "global_utility", "reward", "velocity")}
# the named series of others.csv (recorder.py: write_to_disk(..., fair_idx=, reward=) for the single-UBS simulator, none for the other)
_OTHERS = {False: (), True: ("fair_idx", "reward")}


def _is_single(env) -> bool:
    from .sim import BatchedSingleUbsCoverageEnv
    return isinstance(env, BatchedSingleUbsCoverageEnv)


def _shape_of(env):
    return (_is_single(env), int(env.B), 1 if _is_single(env) else int(env.n_agents), int(env.n_gts), int(env.episode_limit))


def _cell(v, f32: bool) -> str:
    """One numeric CSV cell as pandas prints it: the shortest text that parses back to the value IN ITS OWN FORMAT (a float32 is printed
    as a float32), nothing for NaN."""
    if v != v:
        return ""
    return str(np.float32(v)) if f32 else repr(float(v))


def _csv_text(rows) -> str:
    return "".join(",".join(r) + "\n" for r in rows)


class Film:
    def __init__(self, env, episodes: int):
        self.single, self.B, self.n, self.M, self.T = _shape_of(env)
        self.episodes = int(episodes)
        if self.episodes < 1:
            raise ValueError(f"episodes = {episodes}: a film holds at least one episode")
        if self.T < 1:
            raise ValueError("the simulator's episode_limit must be at least 1")
        self.device = th.device(env.device)
        self.dt = float(env.p.dt)
        self.n_actions = int(env.n_actions)
        p = env.p
        # what the plot draws besides the film (recorder.py: the square's border and the circles around the final positions)
        self.plot_consts = dict(range_pos=float(p.range_pos), r_cov=float(p.r_cov), r_sns=float(getattr(p, "r_sns", math.inf)),
                                r_comm=float(getattr(p, "r_comm", math.inf)))
        E, T, n, M = self.episodes, self.T, self.n, self.M
        pos = (E, T + 1, 2) if self.single else (E, T + 1, n, 2)
        layout = [("pos_ubs", np.float64, pos)] + [(k, np.float64, (E, T)) for k in _SERIES[self.single]]
        if self.single:
            layout.append(("rate_per_gt", np.float32, (E, T, M)))
        layout.append(("pos_gts", np.float32, (E, M, 2)))
        # one buffer: 8 bytes for the status word, the float64 fields, the float32 fields
        self._layout, off = [], 8
        for name, dt, shape in layout:
            nbytes = int(np.prod(shape)) * np.dtype(dt).itemsize
            self._layout.append((name, dt, shape, off, nbytes))
            off += nbytes
        self.buf = th.zeros(off, dtype=th.uint8, device=self.device)
        self.status = self.buf[:4].view(th.int32)
        self.fields: Dict[str, th.Tensor] = {}
        for name, dt, shape, o, nbytes in self._layout:
            tdt = th.float64 if dt is np.float64 else th.float32
            self.fields[name] = self.buf[o:o + nbytes].view(tdt).view(shape)
        self.clear()

    def clear(self) -> None:
        """Every slot back to the fill value, the status word to 0."""
        for v in self.fields.values():
            v.fill_(FILL)
        self.status.zero_()

    def match(self, env) -> None:
        got = _shape_of(env)
        if got != (self.single, self.B, self.n, self.M, self.T):
            names = ("single-UBS", "B", "n", "M", "episode_limit")
            want = (self.single, self.B, self.n, self.M, self.T)
            diff = ", ".join(f"{k} = {g} (film: {w})" for k, g, w in zip(names, got, want) if g != w)
            raise ValueError(f"this film was built for another environment shape: {diff}")

    def _launch(self, env, actions: Optional[th.Tensor], episode_base: int) -> None:
        self.match(env)
        L.require_gpu(self.buf, env.pos_ubs, actions)
        f, o = self.fields, env.out
        if self.single:
            if actions is not None:
                actions = actions.to(th.int64).contiguous()
                if actions.numel() != self.B:
                    raise ValueError(f"actions must hold one action per environment ({self.B}), got {tuple(actions.shape)}")
            L.check(L.lib().uavgnn_film_click_subs(
                self.B, self.M, self.T, self.n_actions, self.dt, self.episodes, int(episode_base), env.t.data_ptr(), L.ptr(actions),
                env.moves.data_ptr(), env.pos_ubs.data_ptr(), env.pos_gts.data_ptr(), env.run_f64.data_ptr(), o["reward"].data_ptr(),
                o["rate_per_gt"].data_ptr(), f["pos_ubs"].data_ptr(), f["total_throughput"].data_ptr(), f["fair_idx"].data_ptr(),
                f["global_utility"].data_ptr(), f["reward"].data_ptr(), f["rate_per_gt"].data_ptr(), f["velocity"].data_ptr(),
                f["pos_gts"].data_ptr(), self.status.data_ptr(), L.stream()), "uavgnn_film_click_subs")
        else:
            L.check(L.lib().uavgnn_film_click_mubs(
                self.B, self.n, self.M, self.T, self.episodes, int(episode_base), env.t.data_ptr(), env.pos_ubs.data_ptr(),
                env.pos_gts.data_ptr(), env.run_f32.data_ptr(), o["reward"].data_ptr(), f["pos_ubs"].data_ptr(),
                f["fair_idx"].data_ptr(), f["reward"].data_ptr(), f["pos_gts"].data_ptr(), self.status.data_ptr(), L.stream()),
                "uavgnn_film_click_mubs")

    def reload(self, env, episode_base: int = 0) -> None:
        """After ``env.reset``: the initial UBS positions into slot 0 and the GT positions of episodes ``episode_base + b``
        (``Recorder.reload``).  One launch, no host synchronisation."""
        self._launch(env, None, episode_base)

    def click(self, env, actions: Optional[th.Tensor], episode_base: int = 0) -> None:
        """After ``env.step(actions)``: slot ``env.t`` of episodes ``episode_base + b`` (``Recorder.click``).  One launch, no host
        synchronisation.  actions: what the step was taken with (the single-UBS film derives ``velocity`` from it)."""
        if self.single and actions is None:
            raise ValueError("click: the single-UBS film needs the step's actions (velocity)")
        self._launch(env, actions, episode_base)

    # ---- the host side ---------------------------------------------------------------------------------------------------------
    def numpy(self) -> Dict[str, np.ndarray]:
        """The whole film on the host, ONE device-to-host copy: {field: array over all episodes} + ``status``."""
        host = self.buf.cpu().numpy()
        out = {name: host[o:o + nbytes].view(dt).reshape(shape) for name, dt, shape, o, nbytes in self._layout}
        out["status"] = host[:4].view(np.int32)
        return out

    def check(self, host: Optional[Dict[str, np.ndarray]] = None) -> None:
        """Raises when a click fell outside the film - a step slot beyond ``episode_limit`` or an episode index beyond ``episodes`` -
        and was therefore not recorded.  One device-to-host copy of the status word (none with ``host``, a ``numpy()`` result)."""
        status = int(self.status.item()) if host is None else int(host["status"][0])
        if status & 1:
            raise L.UavGnnError("film: a click fell outside the film (step slot beyond episode_limit, episode index beyond `episodes`, or "
                                "a missing / illegal action) and was not recorded")

    def episode(self, k: int, host: Optional[Dict[str, np.ndarray]] = None) -> Dict[str, np.ndarray]:
        """Episode k as the reference's ``recorder.film`` holds it, stacked, plus ``pos_gts``.  host: a ``numpy()`` result to read from
        (otherwise the film is copied to the host)."""
        if not 0 <= k < self.episodes:
            raise IndexError(f"episode {k} of a film of {self.episodes}")
        host = self.numpy() if host is None else host
        return {name: host[name][k] for name, *_ in self._layout}

    def put(self, k: int, **arrays) -> None:
        """Writes host arrays into episode k (a film filled elsewhere: tests, a reference recording)."""
        for name, v in arrays.items():
            dst = self.fields[name][k]
            dst.copy_(th.as_tensor(np.ascontiguousarray(v)).to(dst.dtype).reshape(dst.shape))

    def write(self, save_dir: str, k: int, plot: bool = False, host: Optional[Dict[str, np.ndarray]] = None) -> None:
        """``recorder.replay(save_dir=...)`` for episode k: ``path_ubs.csv``, ``pos_gts.csv`` and ``others.csv`` in the layout of
        envs/common.py:80-100 (``write_to_disk``), written directly - no pandas -, and with ``plot`` also ``trajectories.png``."""
        ep = self.episode(k, host)
        os.makedirs(save_dir, exist_ok=True)
        path = ep["pos_ubs"].reshape(self.T + 1, -1)
        n = path.shape[1] // 2
        rows = [[""] + [f"UBS-{i}" for i in range(n) for _ in "xy"], [""] + ["position"] * (2 * n), [""] + ["x", "y"] * n]
        rows += [[str(t)] + [_cell(v, False) for v in path[t]] for t in range(self.T + 1)]
        texts = {"path_ubs.csv": _csv_text(rows)}
        gts = ep["pos_gts"]
        texts["pos_gts.csv"] = _csv_text([["", "x", "y"]] + [[f"GT-{m}"] + [_cell(v, True) for v in gts[m]] for m in range(self.M)])
        names = _OTHERS[self.single]
        if names:
            texts["others.csv"] = _csv_text([[""] + list(names)] + [[str(t)] + [_cell(ep[c][t], False) for c in names]
                                                                     for t in range(self.T)])
        else:
            texts["others.csv"] = '""\n'                    # pandas' text of a frame without rows and columns
        for name, text in texts.items():
            with open(os.path.join(save_dir, name), "w", newline="") as f:
                f.write(text)
        if plot:
            self._plot(os.path.join(save_dir, "trajectories.png"), ep)

    def _plot(self, path: str, ep: Dict[str, np.ndarray]) -> None:
        """recorder.py ``replay``: paths dashed, start squares, end circles, GTs, the circles around the final positions, the square's
        border; for the single-UBS film also the fairness / reward panel."""
        try:
            import matplotlib
            matplotlib.use("Agg", force=False)
            import matplotlib.pyplot as plt
        except ImportError as e:
            raise ImportError("Film.write(plot=True) needs matplotlib, which is not installed; plot=False writes the three CSV files "
                              "without it") from e
        c = self.plot_consts
        rp = c["range_pos"]
        pos = ep["pos_ubs"].reshape(self.T + 1, -1, 2)
        steps = int(np.isfinite(pos[:, 0, 0]).sum())              # slots recorded so far
        pos = pos[:max(steps, 1)]
        if self.single:
            fig = plt.figure(tight_layout=True)
            gs = fig.add_gridspec(2, 4)
            ax = fig.add_subplot(gs[:, 0:2])
        else:
            fig, ax = plt.subplots()
        ax.set_aspect("equal")
        if pos.shape[0] > 1:
            ax.scatter(pos[0, :, 0], pos[0, :, 1], marker="s", color="r")
            for i in range(pos.shape[1]):
                ax.plot(pos[:, i, 0], pos[:, i, 1], linestyle="dashed", color="r", linewidth=0.5)
        last = pos[-1]
        ax.scatter(last[:, 0], last[:, 1], marker="o", s=75, color="r", label="UBS" if self.single else "UBSs")
        ax.scatter(ep["pos_gts"][:, 0], ep["pos_gts"][:, 1], marker="o", color="b", label="GTs")
        ang = np.linspace(0, 2 * np.pi, 100)
        for i in range(last.shape[0]):
            for r, style in ((c["r_cov"], dict(color="black")), (c["r_sns"], dict(color="b", alpha=0.25, linewidth=0.5)),
                             (c["r_comm"], dict(color="r", alpha=0.25, linewidth=0.5))):
                if math.isfinite(r):
                    ax.plot(last[i, 0] + r * np.cos(ang), last[i, 1] + r * np.sin(ang), linestyle="dashed", **style)
            ax.annotate("UBS" if self.single else f"UBS-{i}", xy=last[i], xycoords="data", xytext=(0, 5), textcoords="offset points",
                        size="medium")
        ax.plot([0, rp, rp, 0, 0], [0, 0, rp, rp, 0], color="black")
        ax.axis([-0.1 * rp, 1.1 * rp, -0.1 * rp, 1.1 * rp])
        ax.legend(loc="lower right")
        ax.set_xlabel("x (m)")
        ax.set_ylabel("y (m)")
        if self.single:
            ax = fig.add_subplot(gs[:, 2:4])
            ax.set_xlabel("Timestep")
            ax.set_box_aspect(1)
            ax.plot(ep["fair_idx"], color="tab:red")
            ax.set_ylabel("Jain's Fairness Index", color="tab:red")
            ax.tick_params(axis="y", labelcolor="tab:red")
            ax = ax.twinx()
            ax.set_box_aspect(1)
            ax.plot(ep["reward"], color="tab:blue")
            ax.set_ylabel("Reward", color="tab:blue")
            ax.tick_params(axis="y", labelcolor="tab:blue")
        else:
            ax.set_title("Trajectories")
        fig.savefig(path)
        plt.close(fig)


def load_and_run_policy(model_path: str, learner, env, n_episodes: int, output_dir: Optional[str] = None, eps: float = 0.05,
                        seed: int = 0, enc: str = "gnn", graphed: bool = True) -> Dict[str, np.ndarray]:
    """run.py:132-178 on the device: loads the checkpoint into ``learner``, runs ``ceil(n_episodes / env.B)`` rounds of the recording
    evaluation (``GraphedEvaluation``, or ``Evaluation`` with ``graphed=False``) on the evaluation simulator ``env``, writes
    ``output_dir/episode{k}/`` (``Film.write``) for the first ``n_episodes`` episodes when ``output_dir`` is given and returns
    {EpRet, EpLen, AvgGlobalUtility, TotalThroughput, FairIdx[, ProbCollision]: float64 [n_episodes]} - the columns of the reference's
    DataFrame.  One device-to-host copy of the table and one of the film."""
    from .graphs import Evaluation, GraphedEvaluation
    n_episodes = int(n_episodes)
    if n_episodes < 1:
        raise ValueError(f"n_episodes = {n_episodes}: at least one episode")
    learner.load_checkpoint(model_path)
    episodes = -(-n_episodes // env.B) * env.B
    film = Film(env, episodes)
    ev = (GraphedEvaluation if graphed else Evaluation)(learner, env, episodes, eps=eps, seed=seed, enc=enc, film=film)
    ev()
    table = ev.table.cpu().numpy()
    host = film.numpy()
    film.check(host)
    if output_dir is not None:
        for k in range(n_episodes):
            film.write(os.path.join(output_dir, f"episode{k}"), k, host=host)
    return {key: np.array(table[i, :n_episodes], dtype=np.float64) for i, key in enumerate(ev.keys)}
