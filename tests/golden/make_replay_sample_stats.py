#!/usr/bin/env python
"""Generates tests/golden/replay_sample_stats.npz from the REFERENCE's own modules (algos/madrqn/buffer.py loaded unchanged from its
file, the exploration schedule evaluated from the text of algos/madrqn/run.py).  Runs only where the reference is present; data only:

  incl_a / incl_b   per-slot inclusion counts [40] of the first / second 10 000 of N = 20 000 seeded ``ReplayBuffer.sample(8)`` calls
                    (``random.sample`` over a deque) on a buffer holding 40 sequences
  pair_a / pair_b   co-inclusion counts [780] of the slot pairs i < j over the same two halves
  size, batch, n_draws
  eps_decay [2], eps_t [2, 7], eps_val [2, 7] (float64)
                    run.py:60-61's ``eps_thres(t)`` at t in {0, 1, decay / 2, decay - 1, decay, decay + 10, 3e6} for the decay_steps of
                    algos/madrqn/config.py and algos/drqn/config.py
"""
import importlib.util
import os
import random
import re
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("UAVGNN_REFERENCE", "/root/reference")
sys.path[:0] = [ROOT]

SIZE, BATCH, N_DRAWS, SEED = 40, 8, 20000, 20241


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def sample_stats():
    from tests.replay_sampler_ref import inclusion_counts
    buffer = _load(os.path.join(REF, "algos", "madrqn", "buffer.py"), "ref_madrqn_buffer")
    rb = buffer.ReplayBuffer(SIZE, 1, scheme=("obs",))
    for s in range(SIZE):
        rb.push(dict(obs=s, next_obs=s))
    assert len(rb) == SIZE
    random.seed(SEED)
    draws = np.array([[seq["obs"][0] for seq in rb.sample(BATCH)] for _ in range(N_DRAWS)], dtype=np.int64)
    half = N_DRAWS // 2
    ia, pa = inclusion_counts(draws[:half], SIZE)
    ib, pb = inclusion_counts(draws[half:], SIZE)
    return dict(incl_a=ia, incl_b=ib, pair_a=pa, pair_b=pb, size=SIZE, batch=BATCH, n_draws=N_DRAWS)


def eps_values():
    src = open(os.path.join(REF, "algos", "madrqn", "run.py")).read().splitlines()
    env = {}
    exec(src[59].strip(), env)                     # run.py:60  eps_start, eps_end = 1, 0.05
    line = src[60].strip()                         # run.py:61  eps_thres = lambda t: max(eps_end, ...)
    assert re.match(r"eps_thres = lambda t: ", line), line
    decays, ts, vals = [], [], []
    for cfg in ("madrqn", "drqn"):
        decay = _load(os.path.join(REF, "algos", cfg, "config.py"), f"ref_{cfg}_config").DEFAULT_CONFIG["decay_steps"]
        scope = dict(env, args=types.SimpleNamespace(decay_steps=decay))
        exec(line, scope)
        t = [0, 1, decay // 2, decay - 1, decay, decay + 10, 3 * 10 ** 6]
        decays.append(decay), ts.append(t), vals.append([float(scope["eps_thres"](v)) for v in t])
    return dict(eps_decay=np.array(decays, dtype=np.int64), eps_t=np.array(ts, dtype=np.int64),
                eps_val=np.array(vals, dtype=np.float64), eps_start=np.float64(env["eps_start"]), eps_end=np.float64(env["eps_end"]))


if __name__ == "__main__":
    if not os.path.isdir(REF):
        print(f"{REF} is absent: nothing generated")
        sys.exit(0)
    out = dict(sample_stats(), **eps_values())
    path = os.path.join(HERE, "replay_sample_stats.npz")
    np.savez_compressed(path, **out)
    print(f"replay_sample_stats.npz -> {os.path.getsize(path)} B")
