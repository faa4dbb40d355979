#!/usr/bin/env python
"""Wall time of an EPOCH of ``uav_bs_ctrl_amd.run.Run.train`` at the reference's sizes against (i) the event-timed sum of the graph replays
inside that epoch and (ii) an epoch of the loop of INTEGRATION.md written out by hand from ``GraphedEpisode`` (learner generator draws, no
``explore_seed``: the pieces as they stood before the driver), ``GraphedEvaluation``, ``EpochStats`` and ``lr_scheduler.step()`` - the two
loops alternating, epoch by epoch, in one process.

  exp3   map '8ubs' (8 x 50, episode limit 50 = T), TarMAC, H = 256, 32 environments, batch 32, 5 evaluation episodes
  exp1   n_grps = 4 x gts_per_grp = 5 (episode limit 200, T = 10), 'gnn' agent, H = 256, 32 environments, batch 32, 5 evaluation episodes

    python tools/train_probe.py [--episodes 8] [--repeats 4] [--points exp3 exp1] [--out profiles/train_probe.txt]

An epoch is ``--episodes`` training replays + one evaluation; every timed epoch trains (the collect-only replay falls into the warm-up
epoch).  The driver's epoch also writes its row and ``state.pt`` (ring included: ``--ring`` sequences); that part is timed by itself and
reported next to the total.  Measurements, not thresholds: host clock around work that ends in a device synchronise; spread = max - min
over the repeats.  One JSON row per arm; --out also writes them as a table.

    python tools/train_probe.py --dp [--episodes 8] [--repeats 4] [--out profiles/train_probe.txt]

--dp: what cutting the episode graph at the gradient all-reduce costs.  One epoch of exp3 at the sizes above on two runs of one process,
alternating epoch by epoch: a non-distributed ``Run`` (every training episode ONE graph) against a ``Run`` in a world-size-1 process group
with ``force_collective`` (every training episode cut into ``segments * updates_per_segment + 1`` graphs with the RCCL all-reduce of the
flat gradient buffer issued eagerly at each cut).  Both with ``save_replay=False``, so ``state.pt`` is the small file in either arm.  RCCL
at N > 1 is not what this measures.  --out APPENDS these rows to the table."""
import argparse
import json
import os
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

E, BATCH, TEST_EPISODES = 32, 32, 5


def _args(point, episodes, limit, ring):
    a = dict(device="cuda", hidden_size=256, n_layers=2, n_heads=4, lr=5e-4 if point == "exp1" else 2.5e-4, gamma=0.99, polyak=0.999,
             batch_size=BATCH, replay_size=ring, decay_steps=2e5, steps_per_epoch=episodes * E * limit, epochs=10 ** 6, update_after=0,
             num_test_episodes=TEST_EPISODES, save_freq=10 ** 6, anneal_lr=True)
    if point == "exp1":
        a.update(agent="gnn", max_seq_len=10)
    else:
        a.update(o="gnn", c="tarmac", share_reward=False, msg_size=64, key_size=16, n_rounds=1, double_q=True, dueling=False, mixer=False,
                 max_seq_len=None)
    return a


def _env(point):
    from uav_bs_ctrl_amd.sim import MAPS, SingleUbsParams
    return (SingleUbsParams(n_grps=4, gts_per_grp=5), 200) if point == "exp1" else ("8ubs", MAPS["8ubs"].params.episode_limit)


class _EventSum:
    """Wraps ``graph.replay`` of the driver's graphs: a HIP event pair per replay, summed after a synchronise."""

    def __init__(self, *graphs):
        import torch as th
        self.th, self.pairs = th, []
        for g in graphs:
            g.replay = self._timed(g.replay)

    def _timed(self, replay):
        def run():
            e0, e1 = self.th.cuda.Event(enable_timing=True), self.th.cuda.Event(enable_timing=True)
            e0.record()
            replay()
            e1.record()
            self.pairs.append((e0, e1))
        return run

    def take_ms(self):
        self.th.cuda.synchronize()
        ms, self.pairs = sum(a.elapsed_time(b) for a, b in self.pairs), []
        return ms


def _hand_loop(point, args, env_spec, episodes):
    """INTEGRATION.md's loop from public pieces; returns a closure that runs one epoch."""
    import torch as th

    from uav_bs_ctrl_amd.film import Film
    from uav_bs_ctrl_amd.graphs import INFO_KEYS, GraphedEpisode, GraphedEvaluation
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner, QLearner
    from uav_bs_ctrl_amd.replay import SequenceReplay, SingleUbsSequenceReplay
    from uav_bs_ctrl_amd.sim import BatchedSingleUbsCoverageEnv, BatchedUbsCoverageEnv
    from uav_bs_ctrl_amd.stats import EpochStats
    a = types.SimpleNamespace(**args)
    th.manual_seed(0)
    if point == "exp1":
        enc = a.agent
        env, test_env = BatchedSingleUbsCoverageEnv(env_spec, E, seed=1), BatchedSingleUbsCoverageEnv(env_spec, TEST_EPISODES, seed=2)
        learner = QLearner(env.get_env_info(enc), a)
        rb = SingleUbsSequenceReplay(a.replay_size, a.max_seq_len, env.n_gts, a.hidden_size, n_envs=E, device_state=True, seed=3)
    else:
        enc = "gnn"
        env, test_env = BatchedUbsCoverageEnv.from_map(env_spec, E, seed=1), BatchedUbsCoverageEnv.from_map(env_spec, TEST_EPISODES, seed=2)
        learner = MultiAgentQLearner(env.get_env_info(enc), a)
        rb = SequenceReplay(a.replay_size, env.episode_limit, env.n_agents, env.n_gts, a.hidden_size, n_envs=E, r_comm=env.p.r_comm,
                            device_state=True, seed=3)
    keys = [k for k in INFO_KEYS if not (point == "exp1" and k == "ProbCollision")]
    st = EpochStats(keys + ["LossQ"] + ["Test" + k for k in keys], "cuda")
    film = Film(test_env, TEST_EPISODES)
    eps = (1.0, 0.05, a.decay_steps)
    collect = GraphedEpisode(learner, env, rb, BATCH, eps=eps, train=False, enc=enc, stats=st)
    train = GraphedEpisode(learner, env, rb, BATCH, eps=eps, train=True, enc=enc, stats=st)
    test_agent = GraphedEvaluation(learner, test_env, TEST_EPISODES, eps=0.05, seed=4, enc=enc, stats=st, film=film)
    collect()
    train.t.copy_(collect.t)
    rows = []

    def epoch():
        for _ in range(episodes):
            train()
        test_agent()
        learner.lr_scheduler.step()
        rb.check()
        film.check()
        rows.append(st.summary())
        st.reset()
    return epoch


def point_rows(point, episodes, repeats, ring, out_dir):
    import torch as th

    from uav_bs_ctrl_amd.run import Run
    env_spec, limit = _env(point)
    args = _args(point, episodes, limit, ring)
    run = Run.create(point, env_spec, args, os.path.join(out_dir, point), exp_name="train_probe", seed=0, n_envs=E, n_test_envs=TEST_EPISODES)
    events = _EventSum(run.collect.graph, run.train_episode.graph, run.evaluation.graph)
    saves, save_state = [], run._save_state

    def timed_save():
        th.cuda.synchronize()
        t0 = time.perf_counter()
        save_state()
        saves.append(time.perf_counter() - t0)
    run._save_state = timed_save
    hand = _hand_loop(point, args, env_spec, episodes)
    run.train(epochs=1)                      # warm-up epoch of both: the collect-only replay, allocator pools, the first state.pt
    hand()
    events.take_ms()
    saves.clear()
    wall = dict(driver=[], hand=[])
    replay_ms, save_ms = [], []
    for _ in range(repeats):
        th.cuda.synchronize()
        t0 = time.perf_counter()
        run.train(epochs=1)
        th.cuda.synchronize()
        wall["driver"].append(1e3 * (time.perf_counter() - t0))
        replay_ms.append(events.take_ms())
        save_ms.append(1e3 * saves.pop())
        t0 = time.perf_counter()
        hand()
        th.cuda.synchronize()
        wall["hand"].append(1e3 * (time.perf_counter() - t0))
    run.logger.close()
    r3 = lambda v: [round(x, 2) for x in v]  # noqa: E731
    spread = lambda v: round(max(v) - min(v), 2)  # noqa: E731
    without = [d - s for d, s in zip(wall["driver"], save_ms)]
    what = f"{point}: {episodes} training replays + 1 evaluation per epoch, {E} environments, ring {ring}"
    rows = [dict(what=what, arm="Run.train, one epoch (wall)", ms=r3(wall["driver"]), spread_ms=spread(wall["driver"])),
            dict(what=what, arm="  of which state.pt (ring included)", ms=r3(save_ms), spread_ms=spread(save_ms)),
            dict(what=what, arm="  Run.train without state.pt", ms=r3(without), spread_ms=spread(without)),
            dict(what=what, arm="  its graph replays (HIP events, summed)", ms=r3(replay_ms), spread_ms=spread(replay_ms)),
            dict(what=what, arm="hand-written loop, one epoch (wall)", ms=r3(wall["hand"]), spread_ms=spread(wall["hand"]))]
    for r in rows:
        print(json.dumps(r), flush=True)
    return rows


def dp_rows(episodes, repeats, ring, out_dir):
    """The whole-episode graph against the graphs cut at the all-reduce (world size 1 over RCCL), alternating in this process."""
    import socket

    import torch as th
    import torch.distributed as dist

    from uav_bs_ctrl_amd.run import Run
    env_spec, limit = _env("exp3")
    args = _args("exp3", episodes, limit, ring)
    kw = dict(exp_name="train_probe", seed=0, n_envs=E, n_test_envs=TEST_EPISODES, save_replay=False)
    whole = Run.create("exp3", env_spec, args, os.path.join(out_dir, "whole"), **kw)       # built BEFORE the group exists: not data-parallel
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    th.cuda.set_device(0)
    dist.init_process_group("nccl", device_id=th.device("cuda", 0))
    try:
        cut = Run.create("exp3", env_spec, args, os.path.join(out_dir, "cut"), force_collective=True, **kw)
        pieces = dict(whole=len(whole.train_episode.graphs), cut=len(cut.train_episode.graphs))
        runs = dict(whole=whole, cut=cut)
        for run in runs.values():
            run.train(epochs=1)                  # warm-up epoch: the collect-only replay, allocator pools, the communicator
        wall = dict(whole=[], cut=[])
        for _ in range(repeats):
            for name, run in runs.items():
                th.cuda.synchronize()
                t0 = time.perf_counter()
                run.train(epochs=1)
                th.cuda.synchronize()
                wall[name].append(1e3 * (time.perf_counter() - t0))
        for run in runs.values():
            run.logger.close()
    finally:
        dist.destroy_process_group()
    what = (f"exp3 --dp: {episodes} training replays + 1 evaluation per epoch, {E} environments, ring {ring}, state.pt without the ring; "
            f"world size 1")
    arms = (("whole", "Run.train, not distributed: one graph per episode"),
            ("cut", "Run.train, force_collective over RCCL: cut graphs"))
    rows = [dict(what=what, arm=f"{label} ({pieces[name]} piece{'s' if pieces[name] > 1 else ''})", pieces=pieces[name],
                 ms=[round(x, 2) for x in wall[name]], spread_ms=round(max(wall[name]) - min(wall[name]), 2)) for name, label in arms]
    for r in rows:
        print(json.dumps(r), flush=True)
    return rows


def _write_table(f, rows):
    what = None
    for r in rows:
        if r["what"] != what:
            what = r["what"]
            f.write(f"\n{what}\n")
        f.write(f"  {r['arm']:<42} {r['ms']}  spread {r['spread_ms']}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=8, help="training replays per epoch")
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--ring", type=int, default=8 * E, help="replay_size in sequences")
    ap.add_argument("--points", nargs="+", default=["exp3", "exp1"])
    ap.add_argument("--out", default=None, help="also write the rows as a table (--dp: append them to it)")
    ap.add_argument("--dp", action="store_true", help="exp3 only: the whole-episode graph against the graphs cut at the gradient all-reduce")
    a = ap.parse_args()
    if a.dp:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # before the first HIP call, as bench.py sets it for RCCL
    import torch as th
    if not th.cuda.is_available():
        raise SystemExit("train_probe: no GPU (there is no CPU fallback)")
    rows = []
    if a.dp:
        with tempfile.TemporaryDirectory() as d:
            rows = dp_rows(a.episodes, a.repeats, a.ring, d)
        if a.out:
            with open(a.out, "a") as f:
                _write_table(f, rows)
        return
    with tempfile.TemporaryDirectory() as d:
        for point in a.points:
            rows += point_rows(point, a.episodes if point == "exp3" else max(a.episodes // 4, 1), a.repeats, a.ring, d)
    if a.out:
        with open(a.out, "w") as f:
            f.write("train probe (tools/train_probe.py): MI355X, host clock around a device synchronise, the two loops alternating; ms per epoch\n")
            _write_table(f, rows)


if __name__ == "__main__":
    main()
