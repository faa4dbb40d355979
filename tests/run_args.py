"""Complete arguments at test sizes for ``uav_bs_ctrl_amd.run`` (tests/test_run_host.py, tests/test_run_gpu.py): the package holds no
defaults, so the tests carry their own."""


def small_args(exp, **over):
    """Complete arguments at test sizes (the package holds no defaults)."""
    a = dict(device="cuda", hidden_size=32, n_layers=2, n_heads=4, lr=1e-3, gamma=0.99, polyak=0.9, batch_size=4, replay_size=8,
             decay_steps=200.0, steps_per_epoch=80, epochs=3, update_after=40, num_test_episodes=4, save_freq=2, anneal_lr=True)
    if exp == "exp1":
        a.update(agent="rnn", max_seq_len=5)
    else:
        a.update(o="gnn" if exp == "exp3" else "mlp", c="tarmac", share_reward=False, msg_size=8, key_size=4, n_rounds=1, double_q=True,
                 dueling=False, mixer=False, max_seq_len=None)
    a.update(over)
    return a
