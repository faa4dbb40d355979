"""C-ABI call trace and state hashes of every capturing class of ``uav_bs_ctrl_amd/graphs.py`` - the record behind
profiles/graphs_one_capture_trace.txt.  One arm per process:

    python tools/graphs_capture_trace.py --root <checkout> --out arm.json        # a fresh process per checkout, same seeds
    python tools/graphs_capture_trace.py --compare parent.json new.json          # prints the table, exit 1 on any difference

Per object: the ordered call list during construction (warm-up and capture pass; entry name, every non-pointer argument, NULL / non-NULL
per pointer) as a count and a SHA-256, the number of graphs built, and the SHA-256 of the state after construction and after three calls."""
import argparse
import ctypes
import hashlib
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root"), ap.add_argument("--out"), ap.add_argument("--compare", nargs=2)
    a = ap.parse_args()
    if a.compare:
        return compare(*a.compare)
    sys.path.insert(0, os.path.abspath(a.root))
    import torch as th

    from tests import test_graphed_episode_gpu as TE
    from tests.gpu_util import _LibSpy
    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd import graphs as G
    from uav_bs_ctrl_amd.film import Film
    from uav_bs_ctrl_amd.run import seed_comm_modules
    spy, built, rows = _LibSpy(L.lib()), [0], {}
    L.lib = lambda: spy
    real_graph = th.cuda.CUDAGraph

    def counting(*args, **kw):
        built[0] += 1
        return real_graph(*args, **kw)
    th.cuda.CUDAGraph = counting

    def sha(tensors):
        h = hashlib.sha256()
        for t in tensors:
            if t is not None:
                h.update(t.detach().cpu().contiguous().numpy().tobytes())
        return h.hexdigest()[:16]

    def trace():
        ptr = lambda t: t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, (ctypes._Pointer, ctypes.Array))  # noqa: E731
        return [(name,) + tuple(("A" if isinstance(v, ctypes.Array) else "P" if v else "0") if ptr(t) else v
                                for t, v in zip(L.SIGNATURES[name][1], args)) for name, args in spy.calls]

    def learner_state(lr):
        opt = lr.optimizer
        comm = [m.rng_state for net in (lr.policy_net, lr.target_net) for m in net.modules() if isinstance(getattr(m, "rng_state", None), th.Tensor)]
        return [lr.flat.flat, lr.flat_target, opt.m, opt.v, opt.hyper, lr._gen.get_state()] + comm

    def record(name, lr, make, state, call):
        """make() -> object; state(obj) -> tensors; call(obj) -> one replay."""
        spy.calls.clear(), spy.names.clear()
        built[0] = 0
        obj = make()
        th.cuda.synchronize()
        t = trace()
        row = dict(calls=len(t), distinct=len({c[0] for c in t}), trace=hashlib.sha256(repr(t).encode()).hexdigest()[:16], graphs=built[0],
                   built=sha(learner_state(lr) + state(obj)))
        for _ in range(3):
            call(obj)
        th.cuda.synchronize()
        row["after3"] = sha(learner_state(lr) + state(obj))
        rows[name] = row
        print(name, row, flush=True)
        return obj

    def multi(c):
        lr, env, rb, kw = TE._multi()
        if c != "tarmac":           # the same sizes with another communication module
            import types
            args = types.SimpleNamespace(**{**vars(lr.args), "c": c})
            th.manual_seed(3)
            lr = type(lr)(dict(obs_shape=dict(agent=2, ubs=2, gt=4), n_actions=env.n_actions, n_agents=env.n_agents,
                               episode_limit=env.episode_limit), args)
            seed_comm_modules(lr, 77)
        return lr, env, rb, kw

    def fill(bufs, seed):
        gen = th.Generator(device="cuda").manual_seed(seed)
        for b in bufs:
            if b is not None:
                b.copy_(th.rand(b.shape, device="cuda", generator=gen)) if b.dtype != th.int64 else b.random_(0, 3, generator=gen)

    def env_rng(env):
        return env.map_rng if getattr(env, "map_rng", None) is not None else env.rng

    def updates(tag, lr, make, bufs):
        def call(gu):
            fill(bufs(gu), 9)
            gu()
        return record(tag, lr, make, lambda gu: [gu.out["LossQ"]], call)

    # ---- GraphedAct / GraphedSingleUbsAct
    lr, env, _, _ = multi("tarmac")
    n, M, rc = env.n_agents, env.n_gts, env.p.r_comm
    env.reset_from_map()
    o, h0 = env.observations(), lr.init_hidden(4)
    record("act-multi", lr, lambda: G.GraphedAct(lr, 4, n, M, rc), lambda ga: [ga.acts, ga.h_out],
           lambda ga: ga(o["gt"], o["ubs"], o["agent"], o["d_u2u"], h0, 0.3))
    for enc in ("gnn", "rnn"):
        l1, e1, _, _ = TE._exp1(enc)
        e1.reset()
        record(f"act-exp1-{enc}", l1, lambda: G.GraphedSingleUbsAct(l1, 4, e1.n_gts, enc), lambda ga: [ga.acts, ga.h_out],
               lambda ga: ga(e1.out["obs_gt"], e1.out["obs_agent"], l1.init_hidden(4), 0.3))
    # ---- GraphedUpdate / GraphedSingleUbsUpdate / GraphedCycle
    mbufs = lambda gu: [gu.obs.gt, gu.obs.ubs, gu.obs.agent, gu.obs.d_u2u, gu.h0, gu.h1, gu.acts, gu.rews, gu.dones]  # noqa: E731
    sbufs = lambda gu: [gu.gt, gu.agent, gu.h0, gu.h1, gu.acts, gu.rews, gu.dones]  # noqa: E731
    for c in ("tarmac", "disc"):
        lc = multi(c)[0]
        updates(f"update-{c}", lc, lambda: G.GraphedUpdate(lc, 4, 3, n, M, rc), mbufs)
    for enc in ("gnn", "rnn"):
        l1, e1, _, _ = TE._exp1(enc)
        updates(f"update-exp1-{enc}", l1, lambda: G.GraphedSingleUbsUpdate(l1, 8, 3, e1.n_gts, enc), sbufs)
    lr = multi("tarmac")[0]
    hold = G.GraphedUpdate(lr, 4, 3, n, M, rc, capture=False)
    fill(mbufs(hold), 9)
    g = env.graph(with_comm=True, static=True)

    def body():
        _, h1 = lr.act(g, h0, 0.3)
        lr.act(g, h1, 0.3)
        return lr.update(hold._batch())
    record("cycle", lr, lambda: G.GraphedCycle(lr, body), lambda cyc: [cyc.out["LossQ"]], lambda cyc: cyc())
    # ---- GraphedEpisode / GraphedEvaluation on the three setups
    for name, setup in TE.SETUPS.items():
        for train in (True, False):
            le, ee, rb, kw = setup()
            record(f"episode-{name}-{'train' if train else 'collect'}", le, lambda: G.GraphedEpisode(le, ee, rb, train=train, **kw),
                   lambda ge: [rb.state, rb.rng, rb.status, env_rng(ee), ge.t, ge.eps, ge.explore, ge.out["LossQ"] if train else None],
                   lambda ge: ge())
        for film in ((False, True) if name == "multi-tarmac" else (False,)):
            le, ee, rb, kw = setup()
            fl = Film(ee, 8) if film else None
            record(f"evaluation-{name}{'-film' if film else ''}", le, lambda: G.GraphedEvaluation(le, ee, 8, eps=0.3, seed=5, enc=kw["enc"], film=fl),
                   lambda ev: [ev.rng, ev.table, env_rng(ee)] + ([fl.buf, fl.status] if film else []), lambda ev: ev())
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)
    # ---- last, because the process group changes the capture mode of everything after it: GraphedUpdate cut at the all-reduce
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29533", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("nccl", device_id=th.device("cuda", 0))
    lc = multi("tarmac")[0]
    lc.grads.force_collective = True
    updates("update-tarmac-collective", lc, lambda: G.GraphedUpdate(lc, 4, 3, n, M, rc), mbufs)
    th.cuda.synchronize()
    dist.destroy_process_group()
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)


def compare(pa, pb):
    ra, rb = json.load(open(pa)), json.load(open(pb))
    bad = sorted(set(ra) ^ set(rb))
    for k in ra:
        same = ra[k] == rb.get(k)
        bad += [] if same else [k]
        print(f"{k:36s} {'identical' if same else 'DIFFERENT'}  " + " ".join(f"{x}={v}" for x, v in ra[k].items()))
        if not same:
            print(f"{'':36s} other arm:  " + " ".join(f"{x}={v}" for x, v in rb.get(k, {}).items()))
    print("RESULT:", "all identical" if not bad else f"differences in {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
