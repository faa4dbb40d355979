"""Builders of ``config.json`` texts for the tests of ``uav_bs_ctrl_amd.series`` (tests/test_series_host.py, tests/test_series_gpu.py)."""
import types


def reference_text(env_fn, env_kwargs, args, seed=20, exp_name="made_up"):
    """A ``config.json`` as the reference's logger writes it (utils/logx.py:126-134): no ``uav_bs_ctrl_amd`` key."""
    from uav_bs_ctrl_amd.run import config_text
    return config_text(dict(env_fn=type(env_fn, (), {}), env_kwargs=env_kwargs, seed=seed, args=types.SimpleNamespace(**args)), exp_name)


def run_text(exp, env, args, seed, exp_name="ours"):
    """The ``config.json`` of ``Run.create`` (run.py), without building a run."""
    from uav_bs_ctrl_amd import run as R
    ns = R.check_args(exp, args)
    ours = dict(exp=exp, env=R._env_to_config(exp, env), n_envs=4, n_test_envs=2, updates_per_segment=1, graphed=True, save_replay=True,
                seeds=R.derive_seeds(seed), world=1, force_collective=False)
    env_fn, env_kwargs = R._reference_env(exp, env)
    return R.config_text(dict(env_fn=env_fn, env_kwargs=env_kwargs, seed=int(seed), args=ns, uav_bs_ctrl_amd=ours), exp_name)
