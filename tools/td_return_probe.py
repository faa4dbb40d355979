#!/usr/bin/env python
"""What the TD tail behind the Q head costs, and what the multi-step kernels (csrc/td_return.hip) save.

    python tools/td_return_probe.py [--rounds 5] [--window-ms 200] [--skip-episode] [--out profiles/td_return_probe.txt]

  tail      forward + backward to d_agent_out of the TD tail alone, on random Q tensors (A = 9, double-Q, importance weights, per-agent
            rewards): 32 sequences x 8 agents x T = 10 and 4096 x 8 x T = 50; targets n = 3 and lambda = 0.8.  Three arms:
              one-step torch   today's chain of ``learner._td_loss`` (gather, argmax, gather, the one-step target, ``_weighted_mse``) - what
                               the default path pays, a different (cheaper) target
              torch            the select in torch ops + ``ops.td_targets_torch`` + the weighted loss, autograd backward
              kernels          ``ops.td_select`` + ``ops.td_return_loss``, autograd backward through their two backward routines
  episode   one ``GraphedEpisode`` replay of map '8ubs' (8 x 50, episode limit 50 = T), TarMAC, H = 256, 32 environments, batch 32, with the
            option off and with returns = ('lambda', 0.8)

The arms alternate inside one process after a warm-up of all.  Every figure is a window of --window-ms of back-to-back iterations
between two device events, divided by the iterations; --rounds windows per arm, reported as median [min .. max] - the spread to hold a
difference against.  The tail arms run eagerly, so at the small size they measure launch and autograd overhead of the host as much as
the device.  Measurements, not thresholds."""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from replay_prio_probe import _alternate, _stat  # noqa: E402

E, BATCH, A, GAMMA = 32, 32, 9, 0.99
SETTINGS = (("nstep", 3), ("lambda", 0.8))


def tail_rows(B, C, T, rounds, window_ms):
    import torch as th

    from uav_bs_ctrl_amd import ops
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    gen = th.Generator(device="cuda").manual_seed(B + T)
    N = B * C
    agent_out = th.randn(T + 1, N, A, device="cuda", generator=gen).requires_grad_(True)
    target_out = th.randn(T, N, A, device="cuda", generator=gen)
    batch = dict(acts=th.randint(A, (T, N, 1), device="cuda", generator=gen), rews=th.rand(T, B, C, device="cuda", generator=gen),
                 dones=(th.rand(T, B, 1, device="cuda", generator=gen) < 0.05).float(), weights=th.rand(B, device="cuda", generator=gen) + 0.1)
    me = types.SimpleNamespace(returns=None, double_q=True, n_agents=C, mixer=None, gamma=GAMMA)
    workspace = {}

    def backward(loss):
        agent_out.grad = None
        loss.backward()

    def one_step():
        backward(MultiAgentQLearner._td_loss(me, batch, T, agent_out, target_out)[0])

    def torch_arm(returns):
        def run():
            qvals = agent_out[:-1].gather(2, batch["acts"]).view(T, B, C)
            next_vals = target_out.gather(2, agent_out[1:].detach().argmax(2, keepdim=True)).view(T, B, C)
            d = qvals - ops.td_targets_torch(next_vals, batch["rews"], batch["dones"], GAMMA, returns)
            backward((d.square() * batch["weights"].view(1, B, 1)).sum() / d.numel())
        return run

    def kernel_arm(returns):
        def run():
            qvals, next_vals = ops.td_select(agent_out, target_out, batch["acts"], True)
            backward(ops.td_return_loss(qvals.view(T, B, C), next_vals.view(T, B, C), batch["rews"], batch["dones"], batch["weights"], GAMMA,
                                        returns, workspace=workspace)[0])
        return run
    out = []
    for returns in SETTINGS:
        arms = {"one-step torch": one_step, "torch": torch_arm(returns), "kernels": kernel_arm(returns)}
        ms, iters = _alternate(arms, rounds, window_ms)
        rows = [dict(what="TD tail, forward + backward", sequences=B, agents=C, T=T, returns=list(returns), arm=name,
                     iters_per_window=iters[name], windows=rounds, **_stat(ms[name])) for name in ms]
        rows.append(dict(what="TD tail, forward + backward", sequences=B, agents=C, T=T, returns=list(returns), arm="kernels / torch",
                         ratio_of_medians=round(rows[2]["median_ms"] / rows[1]["median_ms"], 4),
                         kernels_max_over_torch_min=round(rows[2]["max_ms"] / rows[1]["min_ms"], 4)))
        for r in rows:
            print(json.dumps(r), flush=True)
        out += rows
    return out


def episode_rows(rounds, window_ms):
    import torch as th

    from uav_bs_ctrl_amd.graphs import GraphedEpisode
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    from uav_bs_ctrl_amd.replay import SequenceReplay
    from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv
    runs = {}
    for name, returns in (("off", None), ("on", ("lambda", 0.8))):
        th.manual_seed(0)
        env = BatchedUbsCoverageEnv.from_map("8ubs", E, seed=0)
        args = types.SimpleNamespace(device="cuda", hidden_size=256, c="tarmac", n_heads=4, n_layers=2, msg_size=64, key_size=16, n_rounds=1,
                                     dueling=False, mixer=False, share_reward=False, double_q=True, lr=5e-4, gamma=0.99, polyak=0.999,
                                     max_seq_len=None, batch_size=BATCH, seed=0)
        info = dict(obs_shape=dict(agent=2, ubs=2, gt=4), n_actions=env.n_actions, n_agents=env.n_agents, episode_limit=env.episode_limit)
        rb = SequenceReplay(8 * E, env.episode_limit, env.n_agents, env.n_gts, 256, n_envs=E, state_dim=0, r_comm=env.p.r_comm,
                            device_state=True, seed=0)
        runs[name] = (GraphedEpisode(MultiAgentQLearner(info, args, returns=returns), env, rb, BATCH, eps=(1.0, 0.05, 5e4)), rb, env)
    ms, iters = _alternate({k: v[0] for k, v in runs.items()}, rounds, window_ms, floor=2)
    out = []
    for name, (ge, rb, env) in runs.items():
        rb.check()
        out.append(dict(what="GraphedEpisode replay, '8ubs', TarMAC, H = 256", returns=name, envs=E, batch=BATCH,
                        episode_limit=env.episode_limit, iters_per_window=iters[name], windows=rounds,
                        loss_finite=bool(th.isfinite(ge.out["LossQ"])), **_stat(ms[name])))
        print(json.dumps(out[-1]), flush=True)
    out.append(dict(what="GraphedEpisode replay", arm="on / off", ratio_of_medians=round(out[1]["median_ms"] / out[0]["median_ms"], 4)))
    print(json.dumps(out[-1]), flush=True)
    return out


def main():   # noqa: D103
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--skip-episode", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for B, C, T in ((32, 8, 10), (4096, 8, 50)):
        rows += tail_rows(B, C, T, a.rounds, a.window_ms)
        _write(a, rows)
    if not a.skip_episode:
        rows += episode_rows(a.rounds, a.window_ms)
    _write(a, rows)


def _write(a, rows):
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"# td_return_probe: windows of {a.window_ms:.0f} ms between device events, {a.rounds} per arm, arms alternating; "
                    f"median [min .. max]\n")
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
