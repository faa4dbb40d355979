"""`-m gpu`: ``uav_bs_ctrl_amd.run.Run`` over a ``torch.distributed`` process group - the data-parallel ``train()`` driver and the episode
graphs cut at the gradient all-reduce (``graphs.GraphedEpisode.graphs``).

Sizes: those of tests/test_run_gpu.py - map 'debug' (3 UBSs x 4 GTs, episode limit 10), ``SingleUbsParams(2 x 3, episode_limit=10)`` with
T = 5 for exp1, H = 32, 4 training environments PER RANK, batch 4, a ring of 8, 3 epochs.  At world size 2 an epoch is 160 interactions:
two episode replays of 2 x 4 x 10, and training starts after 2 x 4 x 10 = 80 (``plan``), so the first replay collects and five train.

Every worker is spawned, reports through a queue of its own and joins a process group with a 120-s timeout, so a rank that dies fails the
test instead of hanging its peer; never more than two GPU processes at a time.  The box has one GPU and RCCL refuses two ranks on one
device: the world-size-2 tests run both ranks on cuda:0 over gloo (as tests/test_dp_gpu.py does), RCCL carries the world-size-1 test
with ``force_collective``.  RCCL at N > 1 stays untested here.

1. the cut graphs equal the whole graph;  2. world size 2: replicas, counters, merged statistics, who writes what;  3. graphed equals
eager at world size 2;  4. resume at world size 2 and the directories ``resume`` refuses;  5. the launcher."""
import datetime
import json
import math
import os
import socket
import subprocess
import sys

import pytest
import torch as th
import torch.multiprocessing as mp

from tests.run_args import small_args
from tests.util import wait_worker

pytestmark = pytest.mark.gpu

E, E_TEST, SEED, WORLD2_STEPS = 4, 2, 3, 160
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPLICATED = ("learner.flat", "learner.flat_target", "learner.m", "learner.v", "learner.hyper")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# ---- what runs inside a worker ----------------------------------------------------------------------------------------------------------
def _join(backend, rank, world, port):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    th.cuda.set_device(0)
    kw = dict(device_id=th.device("cuda", 0)) if backend == "nccl" else {}
    dist.init_process_group(backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120), **kw)


def _leave():
    import torch.distributed as dist
    if dist.is_initialized():
        dist.destroy_process_group()


def _create(name, out, **kw):
    from tests.test_run_gpu import _setup
    from uav_bs_ctrl_amd.run import Run
    over = {k: kw.pop(k) for k in list(kw) if k in ("epochs", "steps_per_epoch")}
    exp, env, args = _setup(name, **over)
    return Run.create(exp, env, args, str(out), exp_name=name, seed=SEED, n_envs=E, n_test_envs=E_TEST, **kw)


def _snap(run):
    """Every tensor of ``_tensors()`` and the ring rows below ``size``, on the host."""
    out = {k: v.detach().cpu().clone() for k, v in run._tensors().items()}
    size = int(run.replay.state[1])
    out.update({"mem." + k: v[:size].detach().cpu().clone() for k, v in run.replay.mem.items()})
    return out


def _differences(a, b):
    return sorted(set(a) ^ set(b)) + [k for k in a if k in b and (a[k].shape != b[k].shape or not th.equal(a[k], b[k]))]


def _numpy(d):
    return {k: v.numpy() for k, v in d.items()}          # pickled by value: nothing is shared with a worker that has exited


def _watch(run):
    """Counts the gradient all-reduces of every episode replay and keeps every epoch's LOCAL accumulator and the summary the run used."""
    grads, per_replay, accs, rows = run.learner.grads, [], [], []
    calls, reduce, episode, summary = [0], grads.all_reduce_mean_, run._episode, run.stats.summary

    def spy(group=None):
        calls[0] += 1
        return reduce(group)

    def counted():
        before = calls[0]
        episode()
        per_replay.append((run.active, calls[0] - before))

    def kept(group=None):
        accs.append(run.stats.acc.cpu().tolist())
        rows.append(summary(group))
        return rows[-1]
    grads.all_reduce_mean_, run._episode, run.stats.summary = spy, counted, kept
    return per_replay, accs, rows


def _report(q, fn, *a):
    try:
        q.put(("ok", fn(*a)))
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put(("err", traceback.format_exc() + repr(e)))
    finally:
        _leave()


def _cut_job(port, out, name, ups):
    from tests.test_run_gpu import _without_time
    from pathlib import Path
    out = Path(out)
    th.cuda.set_device(0)
    ref = _create(name, out / "ref", updates_per_segment=ups)                # no process group yet: ONE graph per episode
    assert len(ref.train_episode.graphs) == 1 and ref.train_episode.collectives_per_replay == 0 and ref.world == 1
    ref.train()
    ref.logger.close()
    want = _snap(ref)
    del ref
    _join("nccl", 0, 1, port)
    run = _create(name, out / "cut", updates_per_segment=ups, force_collective=True)
    per_replay, _, _ = _watch(run)
    ge = run.train_episode
    res = dict(pieces=len(ge.graphs), want_pieces=ge.segments * ups + 1, collectives=ge.collectives_per_replay,
               collect_pieces=len(run.collect.graphs), collect_collectives=run.collect.collectives_per_replay,
               first_is_graph=ge.graphs[0] is ge.graph, needs=run.learner.needs_collective())
    run.train()
    run.logger.close()
    res.update(diff=_differences(want, _snap(run)), per_replay=per_replay,
               rows_equal=_without_time(out / "cut") == _without_time(out / "ref"), n_rows=len(_without_time(out / "cut")[1]),
               config=json.loads((out / "cut" / "config.json").read_text())["uav_bs_ctrl_amd"])
    return res


def _cut_worker(port, q, out, name, ups):
    _report(q, _cut_job, port, out, name, ups)


def _dp_job(rank, world, port, out, name, graphed, epochs, resume):
    """One rank of a world-size-``world`` run over gloo on cuda:0: ``epochs`` epochs of a new run, or (``resume``) of the one in ``out``."""
    from uav_bs_ctrl_amd.run import Run, RunDirectoryError
    import torch.distributed as dist
    _join("gloo", rank, world, port)
    res = dict(rank=rank)
    if resume == "refused":                      # a world-size-1 group on a world-size-2 directory
        with pytest.raises(RunDirectoryError) as e:
            Run.resume(str(out))
        return dict(res, message=str(e.value))
    if resume:
        aside = os.path.join(out, "state.rank1.pt.aside")
        if rank == 1:
            os.replace(os.path.join(out, "state.rank1.pt"), aside)
        dist.barrier()
        with pytest.raises(RunDirectoryError) as e:          # on EVERY rank, though only rank 1 misses its file
            Run.resume(str(out), device="cuda:0")
        res["missing_message"] = str(e.value)
        dist.barrier()
        if rank == 1:
            os.replace(aside, os.path.join(out, "state.rank1.pt"))
        dist.barrier()
        th.manual_seed(12345)                    # nothing of the resumed run may depend on the process's generator
        run = Run.resume(str(out), device="cuda:0")
        res["resumed_at"] = (run.epoch, run.replays, run.interacts, run.active, run.world, run.rank)
    else:
        run = _create(name, out, graphed=graphed, steps_per_epoch=WORLD2_STEPS)
    res["initial"] = _numpy({k: v for k, v in _snap(run).items() if k in REPLICATED})
    per_replay, accs, rows = _watch(run)
    res.update(pieces=len(getattr(run.train_episode, "graphs", [])), rank0_only=[run.test_env is None, run.film is None,
                                                                                  run.evaluation is None, run.logger is None],
               seeds=run.seeds, plan=tuple(run.plan))
    run.train(epochs)
    if run.logger is not None:
        run.logger.close()
    res.update(final=_numpy(_snap(run)), per_replay=per_replay, accs=accs, rows=rows, counters=(run.epoch, run.replays, run.interacts))
    return res


def _dp_worker(rank, world, port, q, *a):
    _report(q, _dp_job, rank, world, port, *a)


# ---- what runs in the test process --------------------------------------------------------------------------------------------------------
def _spawn(target, argsets, timeout=420):
    """One spawned process per argument tuple, each with a queue of its own appended to its arguments' head; the reports in order."""
    ctx = mp.get_context("spawn")
    assert len(argsets) <= 2, "never more than two GPU processes"
    queues = [ctx.Queue() for _ in argsets]
    procs = [ctx.Process(target=target, args=(*head, q, *tail)) for (head, tail), q in zip(argsets, queues)]
    for p in procs:
        p.start()
    try:
        reports = [wait_worker(p, q, timeout=timeout) for p, q in zip(procs, queues)]
    finally:
        for p in procs:
            p.join(60)
            if p.is_alive():
                p.kill()
    for tag, res in reports:
        assert tag == "ok", res
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    return [res for _, res in reports]


def _world2(out, name="multi-tarmac", graphed=True, epochs=None, resume=False):
    port = _free_port()
    return _spawn(_dp_worker, [((r, 2, port), (str(out), name, graphed, epochs, resume)) for r in range(2)])


_CACHE = {}


def _three_epochs_world2(tmp_path_factory):
    """The graphed three-epoch run at world size 2, once per session: (directory, [rank 0's report, rank 1's report])."""
    if "run" not in _CACHE:
        out = tmp_path_factory.mktemp("dp2") / "run"
        _CACHE["run"] = (out, _world2(out))
    return _CACHE["run"]


def _rows(out):
    lines = (out / "progress.txt").read_text().split("\n")
    assert lines[-1] == ""
    return lines[0].split("\t"), [line.split("\t") for line in lines[1:-1]]


def _without_time(out):
    head, rows = _rows(out)
    i = head.index("Time")
    return head, [r[:i] + r[i + 1:] for r in rows]


def _same(a, b):
    return sorted(set(a) ^ set(b)) + [k for k in a if k in b and (a[k].shape != b[k].shape or not (a[k] == b[k]).all())]


# ---- 1. the cut graphs equal the whole graph ------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
@pytest.mark.parametrize("name, ups", [("multi-tarmac", 1), ("exp1-rnn", 2)])
def test_cut_graphs_over_rccl_at_world_size_one_end_where_the_whole_graph_ends(name, ups, tmp_path):
    (res,) = _spawn(_cut_worker, [((_free_port(),), (str(tmp_path), name, ups))])
    segments = 1 if name == "multi-tarmac" else 2
    assert res["needs"] and res["config"]["world"] == 1 and res["config"]["force_collective"] is True
    assert res["pieces"] == res["want_pieces"] == segments * ups + 1 and res["collectives"] == segments * ups and res["first_is_graph"]
    assert res["collect_pieces"] == 1 and res["collect_collectives"] == 0, "train=False holds no update: one graph"
    assert res["per_replay"] == [("collect", 0)] + [("train", segments * ups)] * 5, res["per_replay"]
    assert not res["diff"], res["diff"]
    assert res["rows_equal"] and res["n_rows"] == 3


# ---- 2. world size 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
def test_world_size_two_replicas_counters_statistics_and_files(tmp_path_factory):
    from uav_bs_ctrl_amd.run import derive_seeds, plan
    from uav_bs_ctrl_amd.stats import merge_acc
    out, (r0, r1) = _three_epochs_world2(tmp_path_factory)
    assert (r0["rank"], r1["rank"]) == (0, 1) and r0["pieces"] == r1["pieces"] == 2
    assert r0["rank0_only"] == [False] * 4 and r1["rank0_only"] == [True] * 4
    assert r0["seeds"] == derive_seeds(SEED, 0) and r1["seeds"] == derive_seeds(SEED, 1)
    want_plan = tuple(plan(small_args("exp3", steps_per_epoch=WORLD2_STEPS), E, 10, 10, world=2))
    assert r0["plan"] == r1["plan"] == want_plan and want_plan[1] == 80 and want_plan[3] == 80
    assert r0["per_replay"] == r1["per_replay"] == [("collect", 0)] + [("train", 1)] * 5
    assert r0["counters"] == r1["counters"] == (3, 6, 480)
    for k in REPLICATED:
        assert (r0["final"][k] == r1["final"][k]).all(), f"{k}: the replicas differ"
        assert (r0["initial"][k] == r1["initial"][k]).all() and not (r0["final"][k] == r0["initial"][k]).all(), k
    assert float(r0["final"]["learner.hyper"][1]) == 5, "five updates"
    ring = [k for k in r0["final"] if k.startswith("mem.")]
    assert ring and any(not (r0["final"][k] == r1["final"][k]).all() for k in ("mem.gt", "mem.act", "mem.rew")), "the rings are equal"
    assert not (r0["final"]["replay.rng"] == r1["final"]["replay.rng"]).all() and not (r0["final"]["env.rng"] == r1["final"]["env.rng"]).all()
    assert "evaluation.rng" in r0["final"] and "evaluation.rng" not in r1["final"] and "test_env.rng" not in r1["final"]
    # the row: both ranks counted, statistics merged in rank order
    head, rows = _rows(out)
    assert [r[head.index("TotalEnvInteracts")] for r in rows] == ["160", "320", "480"]
    assert [r[head.index("Episode")] for r in rows] == ["16", "32", "48"]
    keys = ["EpRet", "EpLen", "AvgGlobalUtility", "TotalThroughput", "FairIdx", "ProbCollision", "LossQ"]
    keys += ["Test" + k for k in keys[:6]]
    for epoch, cells in enumerate(rows):
        merged = dict(zip(keys, merge_acc([r0["accs"][epoch], r1["accs"][epoch]])))
        count, mean, m2, lo, hi, bad = merged["EpRet"]
        assert count == 16 and bad == 0 and r0["accs"][epoch][0][0] == r1["accs"][epoch][0][0] == 8
        assert r0["accs"][epoch][0][1] != r1["accs"][epoch][0][1], "the ranks saw the same returns"
        want = dict(AverageEpRet=mean, StdEpRet=math.sqrt(m2 / count), MinEpRet=lo, MaxEpRet=hi)
        n_loss, mean_loss = merged["LossQ"][0], merged["LossQ"][1]
        assert n_loss == (2, 4, 4)[epoch], "one LossQ per update and rank"
        want["LossQ"] = mean_loss                                             # the column of AverageLossQ
        for col, v in want.items():
            assert cells[head.index(col)] == str(v), (epoch, col, cells[head.index(col)], v)
        assert r1["accs"][epoch][keys.index("TestEpRet")][0] == 0 and merged["TestEpRet"][0] == 4, "rank 0 evaluates alone"
        for r in (r0, r1):                                                    # every rank got the merged summary
            assert r["rows"][epoch]["AverageEpRet"] == mean and r["rows"][epoch]["NEpRet"] == 16 and r["rows"][epoch]["AverageLossQ"] == mean_loss
    # who wrote what
    assert sorted(os.listdir(out)) == sorted(["config.json", "progress.txt", "state.pt", "state.rank1.pt", "checkpoint_epoch2.pt",
                                              "checkpoint_epoch3.pt"] + [f"epoch2_episode{n}" for n in range(4)])
    cfg = json.loads((out / "config.json").read_text())["uav_bs_ctrl_amd"]
    assert cfg["world"] == 2 and cfg["force_collective"] is False and cfg["seeds"] == derive_seeds(SEED)
    s0, s1 = (th.load(str(out / n), map_location="cpu") for n in ("state.pt", "state.rank1.pt"))
    assert s0["epoch"] == s1["epoch"] == 3 and s0["interacts"] == s1["interacts"] == 480
    assert th.equal(s0["tensors"]["learner.flat"], s1["tensors"]["learner.flat"]) and not th.equal(s0["mem"]["gt"], s1["mem"]["gt"])


# ---- 3. graphed equals eager ----------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
def test_world_size_two_eager_run_ends_where_the_graphed_run_ends(tmp_path, tmp_path_factory):
    out, graphed = _three_epochs_world2(tmp_path_factory)
    eager = _world2(tmp_path / "eager", graphed=False)
    for g, e in zip(graphed, eager):
        assert e["pieces"] == 0 and e["per_replay"] == g["per_replay"]
        assert not _same(g["final"], e["final"]), (g["rank"], _same(g["final"], e["final"]))
        assert e["accs"] == g["accs"]
    assert _without_time(tmp_path / "eager") == _without_time(out)


# ---- 4. resume --------------------------------------------------------------------------------------------------------------------------------
def _state_differences(a, b):
    """Two state files: every entry but the wall clock."""
    bad = [k for k in a if k not in ("tensors", "mem", "elapsed") and a[k] != b[k]]
    bad += ["tensors." + k for k in _differences(a["tensors"], b["tensors"])] + ["mem." + k for k in _differences(a["mem"], b["mem"])]
    return bad + sorted(set(a) ^ set(b))


@pytest.mark.timeout(900)
def test_world_size_two_resumed_run_ends_where_the_uninterrupted_run_ends(tmp_path, tmp_path_factory):
    whole, reports = _three_epochs_world2(tmp_path_factory)
    part = tmp_path / "part"
    first = _world2(part, epochs=2)
    assert [r["counters"] for r in first] == [(2, 4, 320)] * 2
    assert os.path.exists(part / "state.pt") and os.path.exists(part / "state.rank1.pt")
    assert not [n for n in os.listdir(part) if n.endswith(".tmp")]
    # a world-size-1 group on this directory
    (refused,) = _spawn(_dp_worker, [((0, 1, _free_port()), (str(part), "multi-tarmac", True, None, "refused"))])
    assert "world size 2" in refused["message"] and "1 rank" in refused["message"], refused["message"]
    # fresh processes: first with state.rank1.pt moved away (both ranks refuse), then the resume itself and the third epoch
    second = _world2(part, resume=True)
    for r in second:
        assert "rank file is missing" in r["missing_message"] and "state.rank1.pt" in r["missing_message"], r["missing_message"]
        assert r["resumed_at"] == (2, 4, 320, "train", 2, r["rank"]) and r["counters"] == (3, 6, 480)
    for r, w in zip(second, reports):
        assert not _same(w["final"], r["final"]), (r["rank"], _same(w["final"], r["final"]))
    for name in ("state.pt", "state.rank1.pt"):
        a, b = (th.load(str(d / name), map_location="cpu") for d in (whole, part))
        assert not _state_differences(a, b), (name, _state_differences(a, b))
    head, rows = _without_time(part)
    assert (head, rows) == _without_time(whole) and len(rows) == 3
    assert (part / "progress.txt").read_text().count("Epoch\t") == 1, "one header"


# ---- 5. the launcher --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
def test_the_launcher_runs_two_ranks_on_one_device_over_gloo(tmp_path):
    (tmp_path / "args.json").write_text(json.dumps(small_args("exp3", epochs=1, steps_per_epoch=WORLD2_STEPS)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    done = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                           "--master-port", str(_free_port()), "-m", "uav_bs_ctrl_amd.run", "--exp", "exp3", "--env", "debug",
                           "--args-json", str(tmp_path / "args.json"), "--out", str(tmp_path / "run"), "--seed", str(SEED), "--envs", str(E),
                           "--test-envs", str(E_TEST), "--dist-backend", "gloo", "--dist-timeout", "120", "--one-device"],
                          cwd=ROOT, env=env, capture_output=True, text=True, timeout=420)
    assert done.returncode == 0, done.stderr[-3000:]
    head, rows = _rows(tmp_path / "run")
    assert len(rows) == 1 and rows[0][head.index("Epoch")] == "1" and rows[0][head.index("TotalEnvInteracts")] == "160"
    assert rows[0][head.index("Episode")] == "16" and math.isfinite(float(rows[0][head.index("LossQ")]))
    assert os.path.exists(tmp_path / "run" / "state.pt") and os.path.exists(tmp_path / "run" / "state.rank1.pt")
    assert done.stdout.count("epoch 1 of 1") == 1, "one line, from rank 0"
