"""Batched, device-resident counterpart of the reference simulator ``MultiUbsCoverageEnv``
(/root/reference/envs/mubs_cov/mubs_cov.py:10-345; maps: envs/mubs_cov/maps.py) - SURVEY 8f row f3.

B independent environments advance with ONE kernel launch per step (csrc/env_sim.hip, one wavefront per environment);
the padded observations it emits are exactly what the device-side graph builder (``graph.from_padded_obs``) and the
tensor-native replay consume, so a rollout never leaves the GPU: simulator -> graph -> agent -> actions -> simulator.

    env = BatchedUbsCoverageEnv(MapParams(n_ubs=8, n_gts=50, n_rbs=5, ...), B=4096)
    obs = env.reset(pos_ubs, pos_gts, prior)           # or env.reset() with the built-in uniform placement
    obs, reward, done, info = env.step(actions)        # actions [B, n] int64 on the device
    g = env.graph()                                    # HeteroBatch of the current observations (f1)
    info = env.get_env_info("gnn")                     # obs_shape, state_shape, n_actions, n_agents, episode_limit: the learner's env_info

Initial positions and the initial GT priority permutation are INPUTS of ``reset`` (the reference draws them from Python's /
NumPy's global generators in ``Map.set_positions`` and ``reset``); ``reset()`` without arguments places UBSs and GTs uniformly.

The reference's own maps and placements: ``MAPS`` holds its eight registered maps (maps.py:138-151) as ``MapSpec``s, and

    env = BatchedUbsCoverageEnv.from_map("8ubs", B=4096, seed=0)
    obs = env.reset_from_map()                         # placements drawn on the device: ONE launch (csrc/map_sample.hip)

draws what ``Map.set_positions`` + ``np.random.permutation`` draw - UBSs on distinct lattice points, GTs in a shuffled hotspot
- from a counter-based generator keyed by a device ``{seed, resets}`` pair, so the reset is reproducible and graph-capturable.

Experiment 1's single-UBS environment (envs/subs_cov/subs_cov.py) has its own pair at the end of this module: ``SingleUbsParams`` and
``BatchedSingleUbsCoverageEnv`` (csrc/subs_env.hip).
"""
from __future__ import annotations

import ctypes
import dataclasses
import math
from typing import Dict, Optional, Tuple, Union

import numpy as np
import torch as th

from . import _lib as L
from .graph import from_padded_obs, from_single_ubs_obs


@dataclasses.dataclass
class MapParams:
    """Attributes a reference ``Map`` splats onto the env (maps.py:7-30) + the env's class constants (mubs_cov.py:13-20)."""
    n_ubs: int
    n_gts: int
    n_rbs: int = 1
    range_pos: float = 500.0
    episode_limit: int = 20
    dt: float = 10.0
    r_cov: float = 100.0
    r_sns: float = math.inf
    r_comm: float = math.inf
    vels: tuple = (10.0,)
    n_dirs: int = 4
    reward_scale_rate: float = 1.0
    fair_service: bool = True
    avoid_collision: bool = True
    h_ubs: float = 100.0
    p_tx: float = 1e-3 * 10 ** (10 / 10)
    n0: float = 1e-3 * 10 ** (-170 / 10)
    bw: float = 180e3
    fc: float = 2.4e9
    scene: str = "dense-urban"
    safe_dist: float = 10.0
    penalty: float = 5.0

    CHAN = {"suburban": (4.88, 0.43, 0.1, 21), "urban": (9.61, 0.16, 1, 20), "dense-urban": (12.08, 0.11, 1.6, 23),
            "high-rise-urban": (27.23, 0.08, 2.3, 34)}                                          # envs/common.py:34-39

    def chan(self):
        return self.CHAN[self.scene]

    def chan_gain(self, d_level: float) -> float:
        """envs/common.py:49-59 in float64 (used once, for max_rate: mubs_cov.py:39-41)."""
        a, b, eta_los, eta_nlos = self.chan()
        p_los = 1 / (1 + a * math.exp(-b * (math.atan(self.h_ubs / (d_level + 1e-5)) - a)))
        d = math.sqrt(d_level ** 2 + self.h_ubs ** 2)
        fspl = (4 * math.pi * self.fc * d / 3e8) ** 2
        pl = p_los * fspl * 10 ** (eta_los / 20) + (1 - p_los) * fspl * 10 ** (eta_nlos / 20)
        return 1 / pl

    @property
    def max_rate(self) -> float:
        snr_max = self.p_tx * self.chan_gain(0.0) / (self.n0 * self.bw)
        return self.bw * math.log2(1 + snr_max) * 1e-6

    def avail_moves(self) -> np.ndarray:
        """mubs_cov.py:60-64: hover + |vels| x n_dirs displacement vectors."""
        amounts = self.dt * np.array(self.vels, dtype=np.float64).reshape(-1, 1)
        ang = 2 * np.pi * np.arange(self.n_dirs) / self.n_dirs
        dirs = np.stack([np.cos(ang), np.sin(ang)]).T
        return np.ascontiguousarray(np.concatenate((np.zeros((1, 2)), np.kron(amounts, dirs))))


KINDS = ("uniform_lattice", "fixed", "hotspot", "dense_hotspot", "dense_hotspot_v2")


@dataclasses.dataclass
class MapSpec:
    """A reference map: the parameters it splats onto the env + how ``set_positions`` places UBSs and GTs.

    kind             reference                    integers
    uniform_lattice  Map.set_positions :31-35     - (UBSs and GTs on distinct points of the 1 m lattice)
    fixed            Debug :47-50                 fixed_ubs [n,2], fixed_gts [M,2]
    hotspot          HotSpot :64-75               min_dist (lattice pitch, m)
    dense_hotspot    DenseHotSpot :97-113         min_dist, n_grps, gts_per_grp
    dense_hotspot_v2 DenseHotSpotV2 :125-132      ubs_pitch (UBS lattice pitch, m), radius_spot (half the hotspot's side, m)
    """
    params: MapParams
    kind: str
    min_dist: int = 200
    n_grps: int = 0
    gts_per_grp: int = 0
    ubs_pitch: int = 100
    radius_spot: int = 400
    fixed_ubs: Optional[tuple] = None
    fixed_gts: Optional[tuple] = None

    def sampler_consts(self) -> Tuple[list, list]:
        """(int_consts, f64_consts) of uavgnn_map_sample (layout: csrc/map_sample.hip), by the reference's own integer arithmetic."""
        p, kind = self.params, KINDS.index(self.kind)
        n, M, rng_pos = p.n_ubs, p.n_gts, p.range_pos
        L_u, L_s, r, n_picks, gpg, origin = int(rng_pos), 1, 1, 0, 1, 0
        pitch_u, pitch_s, pitch_c, spread = 1.0, 0.0, 0.0, 0.0
        if self.kind in ("hotspot", "dense_hotspot"):
            n_picks, gpg = (M, 1) if self.kind == "hotspot" else (self.n_grps, self.gts_per_grp)
            if n_picks * gpg != M:
                raise ValueError(f"{self.kind}: n_grps x gts_per_grp = {n_picks} x {gpg} is not n_gts = {M}")
            r = 1
            while r * r < n_picks:                                                   # maps.py:68-69 / :101-102
                r += 1
            L_u = int(rng_pos // self.min_dist)
            L_s = int(rng_pos // self.min_dist // r)
            pitch_u, pitch_s, pitch_c = float(self.min_dist), float(self.min_dist * r), float(self.min_dist)
            spread = 0.0 if self.kind == "hotspot" else float(p.r_cov)
        elif self.kind == "dense_hotspot_v2":
            L_u, pitch_u = int(rng_pos // self.ubs_pitch), float(self.ubs_pitch)
            L_s, origin, pitch_s = int(rng_pos // self.radius_spot) - 1, 1, float(self.radius_spot)  # arange(1, range_pos // 400)
            spread = float(2 * self.radius_spot)
        return [kind, n, M, L_u, L_s, r, n_picks, gpg, origin], [float(rng_pos), pitch_u, pitch_s, pitch_c, spread]


def _hotspot(**kw) -> MapSpec:                                                           # maps.py:59-62
    p = dict(range_pos=2000.0, episode_limit=40, dt=20.0, n_ubs=4, n_gts=4, r_cov=100.0, n_rbs=1, r_sns=200.0, r_comm=math.inf,
             vels=(5.0, 10.0), n_dirs=4, reward_scale_rate=10.0)
    p.update(kw)
    return MapSpec(MapParams(**p), "hotspot")


def _dense_hotspot(n_grps=10, gts_per_grp=5, **kw) -> MapSpec:                            # maps.py:88-95
    p = dict(range_pos=6000.0, episode_limit=50, dt=40.0, n_ubs=4, n_gts=n_grps * gts_per_grp, r_cov=100.0, n_rbs=5, r_sns=400.0,
             r_comm=math.inf, vels=(5.0, 10.0), n_dirs=4, reward_scale_rate=10.0)
    p.update(kw)
    return MapSpec(MapParams(**p), "dense_hotspot", n_grps=n_grps, gts_per_grp=gts_per_grp)


def dense_hotspot_v2(**overrides) -> MapSpec:
    """The reference's unregistered hard mode ``DenseHotSpotV2`` (maps.py:117-132); overrides: ``MapParams`` fields."""
    p = dict(range_pos=6000.0, episode_limit=100, dt=10.0, n_ubs=4, n_gts=100, r_cov=100.0, n_rbs=10, r_sns=400.0, r_comm=math.inf,
             vels=(5.0, 10.0), n_dirs=4, reward_scale_rate=10.0)
    p.update(overrides)
    return MapSpec(MapParams(**p), "dense_hotspot_v2")


# the reference's registry (maps.py:138-151)
MAPS: Dict[str, MapSpec] = {
    "test": MapSpec(MapParams(n_ubs=1, n_gts=1), "uniform_lattice"),                                              # Map()
    "debug": MapSpec(MapParams(n_ubs=3, n_gts=4, range_pos=1000.0, episode_limit=10, r_sns=300.0), "fixed",       # Debug()
                     fixed_ubs=((300.0, 300.0), (800.0, 200.0), (800.0, 900.0)),
                     fixed_gts=((300.0, 400.0), (400.0, 200.0), (300.0, 100.0), (600.0, 900.0))),
    "inf": _hotspot(), "r400": _hotspot(r_comm=400.0), "r800": _hotspot(r_comm=800.0),                            # experiment 2
    "4ubs": _dense_hotspot(n_ubs=4), "6ubs": _dense_hotspot(n_ubs=6), "8ubs": _dense_hotspot(n_ubs=8),            # experiment 3
}


class BatchedUbsCoverageEnv:
    def __init__(self, p: MapParams, B: int, device="cuda", max_rate: Optional[float] = None):
        self.p, self.B, self.device = p, B, th.device(device)
        n, M = p.n_ubs, p.n_gts
        self.n_agents, self.n_gts = n, M
        moves = p.avail_moves()
        self.n_actions = moves.shape[0]
        self.episode_limit = p.episode_limit
        a, b, eta_los, eta_nlos = p.chan()
        self.max_rate = p.max_rate if max_rate is None else float(max_rate)
        # int_consts / f64_consts of uavgnn_env_step: layout in include/uavgnn.h
        self._ic = (ctypes.c_int32 * 7)(n, M, p.n_rbs, self.n_actions, p.episode_limit, int(p.fair_service),
                                        int(p.avoid_collision))
        self._fc = (ctypes.c_double * 18)(p.range_pos, p.r_cov, min(p.r_sns, 1e300), min(p.r_comm, 1e300), p.dt, p.h_ubs,
                                          p.p_tx, p.n0, p.bw, p.fc, a, b, eta_los, eta_nlos, p.safe_dist, p.penalty,
                                          p.reward_scale_rate, self.max_rate)
        self.state_dim = L.lib().uavgnn_env_state_dim(n, M, int(p.fair_service))
        dev = self.device
        f32, f64, i32 = (dict(dtype=d, device=dev) for d in (th.float32, th.float64, th.int32))
        self.moves = th.as_tensor(moves, **f64).contiguous()
        self.pos_ubs, self.pos_gts = th.zeros(B, n, 2, **f64), th.zeros(B, M, 2, **f32)
        self.prior, self.avg_rate, self.t = th.zeros(B, M, **i32), th.zeros(B, M, **f32), th.zeros(B, **i32)
        self.run_f32, self.n_colls = th.zeros(B, 4, **f32), th.zeros(B, **f64)
        Sg = 5 if p.fair_service else 4
        self.out = dict(d_u2g=th.zeros(B, n, M, **f32), d_u2u=th.zeros(B, n, n, **f32), gt_ubs=th.zeros(B, M, **i32),
                        gt_rb=th.zeros(B, M, **i32), rate_per_gt=th.zeros(B, M, **f32), rate_per_ubs=th.zeros(B, n, **f64),
                        mask_collision=th.zeros(B, n, **i32), reward=th.zeros(B, n, **f64), done=th.zeros(B, **f32),
                        obs_gt=th.zeros(B, n, M, Sg, **f32), obs_ubs=th.zeros(B, n, max(n - 1, 0), 3, **f32),
                        obs_agent=th.zeros(B, n, 2, **f32), state=th.zeros(B, self.state_dim, **f32))
        self.ep_ret = th.zeros(B, **f64)
        self.spec: Optional[MapSpec] = None                  # set by from_map: the placement sampler's map
        self.map_rng: Optional[th.Tensor] = None             # device int64 {seed, resets} of the placement sampler

    @classmethod
    def from_map(cls, map_id_or_spec: Union[str, MapSpec], B: int, device="cuda", seed: Optional[int] = None):
        """Environment of a registered map (``MAPS``) or of a ``MapSpec``, with the map's placement sampler attached
        (``reset_from_map`` / ``sample_positions``).  seed: the sampler's key (None: drawn from torch's default generator, so
        ``torch.manual_seed`` reproduces a run)."""
        spec = MAPS[map_id_or_spec] if isinstance(map_id_or_spec, str) else map_id_or_spec
        if spec.kind not in KINDS:
            raise ValueError(f"unknown placement kind {spec.kind!r}: one of {KINDS}")
        env = cls(spec.params, B, device)
        ic, fc = spec.sampler_consts()
        env.spec = spec
        env._map_ic, env._map_fc = (ctypes.c_int32 * len(ic))(*ic), (ctypes.c_double * len(fc))(*fc)
        env._map_fixed = (None, None)
        if spec.kind == "fixed":
            env._map_fixed = (th.as_tensor(spec.fixed_ubs, dtype=th.float64, device=env.device).reshape(-1, 2).contiguous(),
                              th.as_tensor(spec.fixed_gts, dtype=th.float32, device=env.device).reshape(-1, 2).contiguous())
            if env._map_fixed[0].shape[0] != env.n_agents or env._map_fixed[1].shape[0] != env.n_gts:
                raise ValueError("fixed placement: fixed_ubs / fixed_gts must hold n_ubs / n_gts points")
        if seed is None:
            seed = int(th.randint(0, 2 ** 62, (1,)).item())
        env.map_rng = th.tensor([int(seed), 0], dtype=th.int64, device=env.device)
        return env

    @property
    def reset_rng(self) -> Optional[th.Tensor]:
        """The reset counter under the name both simulators share: ``map_rng``."""
        return self.map_rng

    # ---- the two kernels ---------------------------------------------------------------------------------------------
    def _launch(self, actions: Optional[th.Tensor]):
        L.require_gpu(self.pos_ubs, actions)
        o = self.out
        if actions is not None:
            actions = actions.to(th.int64).contiguous()
        L.check(L.lib().uavgnn_env_step(self._ic, self._fc, self.B, L.ptr(actions), self.moves.data_ptr(),
                                        self.pos_ubs.data_ptr(), self.pos_gts.data_ptr(), self.prior.data_ptr(),
                                        self.avg_rate.data_ptr(), self.t.data_ptr(), self.run_f32.data_ptr(),
                                        self.n_colls.data_ptr(), o["d_u2g"].data_ptr(), o["d_u2u"].data_ptr(),
                                        o["gt_ubs"].data_ptr(), o["gt_rb"].data_ptr(), o["rate_per_gt"].data_ptr(),
                                        o["rate_per_ubs"].data_ptr(), o["mask_collision"].data_ptr(),
                                        o["reward"].data_ptr(), o["done"].data_ptr(), o["obs_gt"].data_ptr(),
                                        o["obs_ubs"].data_ptr(), o["obs_agent"].data_ptr(), o["state"].data_ptr(),
                                        L.stream()), "uavgnn_env_step")

    def observations(self) -> Dict[str, th.Tensor]:
        """Padded observation tensors of the current state (mubs_cov.py:215-242) + what the wrapper's comm graph reads."""
        o = self.out
        return dict(gt=o["obs_gt"], ubs=o["obs_ubs"], agent=o["obs_agent"], d_u2u=o["d_u2u"], state=o["state"])

    def replay_state(self) -> Dict[str, th.Tensor]:
        """What ``observations()`` is a pure function of, beside the map's constants: pos_ubs [B,n,2] f64, rate [B,M] (this step's
        ``rate_per_gt``), avg [B,M] (``avg_rate`` after this step's update), pos_gts [B,M,2] (constant within an episode) - the step
        fields of ``replay.CompactSequenceReplay``.  VIEWS of the simulator's own buffers: no copy, no launch; the next step overwrites
        them in place."""
        return dict(pos_ubs=self.pos_ubs, rate=self.out["rate_per_gt"], avg=self.avg_rate, pos_gts=self.pos_gts)

    def graph(self, with_comm: bool = True, static: bool = False):
        """HeteroBatch of the current observations, built on the device (f1)."""
        o = self.out
        return from_padded_obs(o["obs_gt"], o["obs_ubs"], o["obs_agent"], o["d_u2u"] if with_comm else None,
                               r_comm=self.p.r_comm, static=static)

    def reset(self, pos_ubs=None, pos_gts=None, prior=None, generator: Optional[th.Generator] = None):
        """mubs_cov.py:86-102.  pos_ubs [B,n,2], pos_gts [B,M,2], prior [B,M] (a permutation of the GTs per env); missing
        ones are drawn uniformly over the square / as random permutations on the device."""
        B, n, M, dev = self.B, self.n_agents, self.n_gts, self.device
        if pos_ubs is None:
            pos_ubs = th.rand(B, n, 2, device=dev, generator=generator, dtype=th.float64) * self.p.range_pos
        if pos_gts is None:
            pos_gts = th.rand(B, M, 2, device=dev, generator=generator) * self.p.range_pos
        if prior is None:
            prior = th.argsort(th.rand(B, M, device=dev, generator=generator), dim=1)
        self.pos_ubs.copy_(th.as_tensor(pos_ubs, dtype=th.float64))
        self.pos_gts.copy_(th.as_tensor(pos_gts).to(th.float32))
        self.prior.copy_(th.as_tensor(prior).to(th.int32))
        for t_ in (self.avg_rate, self.t, self.run_f32, self.n_colls, self.ep_ret):
            t_.zero_()
        self._launch(None)                                     # UBSs serve the GTs at the initial positions (:98)
        return self.observations()

    def _sample_into(self, pos_ubs: th.Tensor, pos_gts: th.Tensor, prior: th.Tensor):
        """One uavgnn_map_sample launch at the current {seed, resets}; then resets += 1 on the device (capturable)."""
        if self.spec is None:
            raise L.UavGnnError("this environment has no map: build it with BatchedUbsCoverageEnv.from_map(...)")
        L.require_gpu(pos_ubs, pos_gts, prior, self.map_rng)
        fu, fg = self._map_fixed
        L.check(L.lib().uavgnn_map_sample(self._map_ic, self._map_fc, self.B, self.map_rng.data_ptr(), L.ptr(fu), L.ptr(fg),
                                          pos_ubs.data_ptr(), pos_gts.data_ptr(), prior.data_ptr(), L.stream()),
                "uavgnn_map_sample")
        self.map_rng[1:].add_(1)

    def sample_positions(self):
        """(pos_ubs [B,n,2] f64, pos_gts [B,M,2] f32, prior [B,M] i32) as the map's ``set_positions`` + the reset's
        ``np.random.permutation`` draw them (maps.py, mubs_cov.py:94-96), in fresh tensors; advances the reset counter."""
        B, n, M, dev = self.B, self.n_agents, self.n_gts, self.device
        out = (th.empty(B, n, 2, dtype=th.float64, device=dev), th.empty(B, M, 2, dtype=th.float32, device=dev),
               th.empty(B, M, dtype=th.int32, device=dev))
        self._sample_into(*out)
        return out

    def reset_from_map(self):
        """mubs_cov.py:86-102 with the map's own placements: the sampler launch (into the state buffers), the running state zeroed as
        ``reset`` zeroes it, the reset-time transmission launch.  No host synchronisation, fixed addresses: capturable."""
        self._sample_into(self.pos_ubs, self.pos_gts, self.prior)
        for t_ in (self.avg_rate, self.t, self.run_f32, self.n_colls, self.ep_ret):
            t_.zero_()
        self._launch(None)
        return self.observations()

    def step(self, actions: th.Tensor):
        """mubs_cov.py:104-129.  actions [B, n] (or [B*n]) int64 on the device.  Returns (observations, reward [B,n] f64,
        done [B] f32, info dict of device tensors) - nothing is synchronised with the host."""
        self._launch(actions.view(self.B, self.n_agents))
        o = self.out
        self.ep_ret += o["reward"].mean(1)
        info = dict(EpRet=self.ep_ret, EpLen=self.t, AvgGlobalUtility=self.run_f32[:, 1], FairIdx=self.run_f32[:, 2],
                    TotalThroughput=self.run_f32[:, 0], ProbCollision=self.n_colls / self.t.clamp(min=1),
                    BadMask=o["done"])                       # the only termination is the episode limit (:343-345)
        return self.observations(), o["reward"], o["done"], info

    def get_env_info(self, enc: str = "gnn") -> dict:
        """The wrapper's ``get_env_info`` (madrqn/utils/env_wrappers.py:114-117): enc 'gnn' -> the feature sizes of the observation
        graph's node types (:62-63: the visibility flags of ``ubs`` / ``gt`` rows become edges, not features), 'mlp' -> the width
        of the flattened observation (:48-49; ``graph.from_padded_obs_flat``'s row: agent, gt, ubs)."""
        if enc not in ("gnn", "mlp"):
            raise ValueError(f"enc must be 'gnn' or 'mlp', got {enc!r}")
        n, M, Sg = self.n_agents, self.n_gts, self.out["obs_gt"].shape[-1]
        obs_shape = 2 + Sg * M + 3 * max(n - 1, 0) if enc == "mlp" else dict(agent=2, ubs=2, gt=Sg - 1)
        return dict(obs_shape=obs_shape, state_shape=self.state_dim, n_actions=self.n_actions, n_agents=n,
                    episode_limit=self.episode_limit)


# ---------------------------------------------------------------------------------------------------------------------
# Experiment 1: the single-UBS environment (envs/subs_cov/subs_cov.py), csrc/subs_env.hip
@dataclasses.dataclass
class SingleUbsParams:
    """Arguments of ``SingleUbsCoverageEnv.__init__`` (subs_cov.py:22-23) + its class constants (:13-20)."""
    range_pos: float = 1000.0
    episode_limit: int = 200
    n_grps: int = 2
    gts_per_grp: int = 1
    r_cov: float = 100.0
    n_rbs: int = 10
    vels: Union[float, tuple] = 10.0
    n_dirs: int = 4
    unit: float = 100.0
    h_ubs: float = 100.0
    p_tx: float = 1e-3 * 10 ** (10 / 10)
    n0: float = 1e-3 * 10 ** (-170 / 10)
    bw: float = 180e3
    fc: float = 2.4e9
    dt: float = 10.0
    scene: str = "urban"

    @property
    def n_gts(self) -> int:
        return self.n_grps * self.gts_per_grp

    @property
    def reward_scale_rate(self) -> float:
        return float(self.n_grps)                                                               # subs_cov.py:67

    def chan(self):
        return MapParams.CHAN[self.scene]

    @property
    def max_rate(self) -> float:
        """subs_cov.py:35-38: the rate of the link straight below the UBS, in float64."""
        a, b, eta_los, eta_nlos = self.chan()
        p_los = 1 / (1 + a * math.exp(-b * (math.atan(self.h_ubs / (0.0 + 1e-5)) - a)))
        d = math.sqrt(0.0 ** 2 + self.h_ubs ** 2)
        fspl = (4 * math.pi * self.fc * d / 3e8) ** 2
        pl = p_los * fspl * 10 ** (eta_los / 20) + (1 - p_los) * fspl * 10 ** (eta_nlos / 20)
        snr_max = self.p_tx * (1 / pl) / (self.n0 * self.bw)
        return self.bw * math.log2(1 + snr_max) * 1e-6

    def avail_moves(self) -> np.ndarray:
        """subs_cov.py:56-59: hover + |vels| x n_dirs displacement vectors."""
        amounts = self.dt * np.array(self.vels, dtype=np.float64).reshape(-1, 1)
        ang = 2 * np.pi * np.arange(self.n_dirs) / self.n_dirs
        dirs = np.stack([np.cos(ang), np.sin(ang)]).T
        return np.ascontiguousarray(np.concatenate((np.zeros((1, 2)), np.kron(amounts, dirs))))


class BatchedSingleUbsCoverageEnv:
    """B independent ``SingleUbsCoverageEnv``s on the device, one launch per step (csrc/subs_env.hip); the interface of
    ``BatchedUbsCoverageEnv``.

        env = BatchedSingleUbsCoverageEnv(SingleUbsParams(n_grps=2, gts_per_grp=5), B=4096, seed=0)
        obs = env.reset()                                  # placements drawn on the device: one sampler launch + one step launch
        obs, reward, done, info = env.step(actions)        # actions [B] int64 on the device
        g = env.graph()                                    # the `seen-by` HeteroBatch of the current observations (no launch)
    """

    def __init__(self, p: SingleUbsParams, B: int, device="cuda", seed: Optional[int] = None):
        self.p, self.B, self.device = p, B, th.device(device)
        M = p.n_gts
        self.n_gts = M
        moves = p.avail_moves()
        self.n_actions = moves.shape[0]
        self.episode_limit = p.episode_limit
        self.max_rate = p.max_rate
        a, b, eta_los, eta_nlos = p.chan()
        self._ic = (ctypes.c_int32 * 5)(M, p.n_rbs, self.n_actions, p.episode_limit, p.n_grps)
        self._fc = (ctypes.c_double * 14)(p.range_pos, p.r_cov, p.dt, p.h_ubs, p.p_tx, p.n0, p.bw, p.fc, a, b, eta_los, eta_nlos,
                                          p.reward_scale_rate, self.max_rate)
        self._sample_ic = (ctypes.c_int32 * 2)(p.n_grps, p.gts_per_grp)
        self._sample_fc = (ctypes.c_double * 2)(p.range_pos, p.r_cov)
        dev = self.device
        f32, f64, i32 = (dict(dtype=d, device=dev) for d in (th.float32, th.float64, th.int32))
        self.moves = th.as_tensor(moves, **f64).contiguous()
        self.pos_ubs, self.pos_gts = th.zeros(B, 2, **f64), th.zeros(B, M, 2, **f32)
        self.prior, self.avg_rate, self.t = th.zeros(B, M, **i32), th.zeros(B, M, **f32), th.zeros(B, **i32)
        self.run_f64 = th.zeros(B, 4, **f64)
        self.out = dict(d_u2g=th.zeros(B, M, **f32), sched=th.zeros(B, M, **i32), rate_per_gt=th.zeros(B, M, **f32),
                        reward=th.zeros(B, **f64), done=th.zeros(B, **f32), obs_gt=th.zeros(B, M, 4, **f32),
                        obs_agent=th.zeros(B, 2, **f32), obs_flat=th.zeros(B, 2 + 4 * M, **f32))
        self.ep_ret = th.zeros(B, **f64)
        if seed is None:                                     # from torch's default generator: torch.manual_seed reproduces a run
            seed = int(th.randint(0, 2 ** 62, (1,)).item())
        self.rng = th.tensor([int(seed), 0], dtype=th.int64, device=dev)     # device {seed, resets} of the placement sampler

    @property
    def reset_rng(self) -> th.Tensor:
        """The reset counter under the name both simulators share: ``rng``."""
        return self.rng

    # ---- the two kernels ---------------------------------------------------------------------------------------------
    def _launch(self, actions: Optional[th.Tensor]):
        L.require_gpu(self.pos_ubs, actions)
        o = self.out
        if actions is not None:
            actions = actions.to(th.int64).contiguous()
            if actions.numel() != self.B:
                raise ValueError(f"actions must hold one action per environment ({self.B}), got {tuple(actions.shape)}")
        L.check(L.lib().uavgnn_subs_env_step(self._ic, self._fc, self.B, L.ptr(actions), self.moves.data_ptr(),
                                             self.pos_ubs.data_ptr(), self.pos_gts.data_ptr(), self.prior.data_ptr(),
                                             self.avg_rate.data_ptr(), self.t.data_ptr(), self.run_f64.data_ptr(),
                                             o["d_u2g"].data_ptr(), o["sched"].data_ptr(), o["rate_per_gt"].data_ptr(),
                                             o["reward"].data_ptr(), o["done"].data_ptr(), o["obs_gt"].data_ptr(),
                                             o["obs_agent"].data_ptr(), o["obs_flat"].data_ptr(), L.stream()),
                "uavgnn_subs_env_step")

    def _sample_into(self, pos_ubs: th.Tensor, pos_gts: th.Tensor, prior: th.Tensor):
        """One uavgnn_subs_env_sample launch at the current {seed, resets}; then resets += 1 on the device (capturable)."""
        L.require_gpu(pos_ubs, pos_gts, prior, self.rng)
        L.check(L.lib().uavgnn_subs_env_sample(self._sample_ic, self._sample_fc, self.B, self.rng.data_ptr(), pos_ubs.data_ptr(),
                                               pos_gts.data_ptr(), prior.data_ptr(), L.stream()), "uavgnn_subs_env_sample")
        self.rng[1:].add_(1)

    def sample_positions(self):
        """(pos_ubs [B,2] f64, pos_gts [B,M,2] f32, prior [B,M] i32) as ``_set_position`` + the reset's ``np.random.permutation``
        draw them (subs_cov.py:92-111, :84), in fresh tensors; advances the reset counter."""
        B, M, dev = self.B, self.n_gts, self.device
        out = (th.empty(B, 2, dtype=th.float64, device=dev), th.empty(B, M, 2, dtype=th.float32, device=dev),
               th.empty(B, M, dtype=th.int32, device=dev))
        self._sample_into(*out)
        return out

    def observations(self) -> Dict[str, th.Tensor]:
        """The observation of the current state in both forms of the reference's wrapper: the Dict fields ``gt`` [B,M,4] and
        ``agent`` [B,2] (subs_cov.py:159-171) and ``flat`` [B, 2+4M], their gym ``flatten`` (env_wrappers.py:51-53)."""
        o = self.out
        return dict(gt=o["obs_gt"], agent=o["obs_agent"], flat=o["obs_flat"])

    def graph(self):
        """`seen-by` HeteroBatch of the current observations (drqn/utils/env_wrappers.py:63-77 for B environments): views, no launch."""
        return from_single_ubs_obs(self.out["obs_gt"], self.out["obs_agent"])

    def reset(self, pos_ubs=None, pos_gts=None, prior=None):
        """subs_cov.py:75-90.  An explicit state - pos_ubs [B,2], pos_gts [B,M,2], prior [B,M] (a permutation of the GTs per
        environment) - or, when all three are None, the placements of the device sampler.  Then the running state is zeroed and the
        reset-time transmission runs (:85).  No host synchronisation, fixed addresses."""
        given = [x is not None for x in (pos_ubs, pos_gts, prior)]
        if not any(given):
            self._sample_into(self.pos_ubs, self.pos_gts, self.prior)
        elif all(given):
            self.pos_ubs.copy_(th.as_tensor(pos_ubs, dtype=th.float64).reshape(self.B, 2))
            self.pos_gts.copy_(th.as_tensor(pos_gts).to(th.float32))
            self.prior.copy_(th.as_tensor(prior).to(th.int32))
        else:
            raise ValueError("reset: give pos_ubs, pos_gts and prior together, or none of them (the sampler draws all three)")
        for t_ in (self.avg_rate, self.t, self.run_f64, self.ep_ret):
            t_.zero_()
        self._launch(None)
        return self.observations()

    def step(self, actions: th.Tensor):
        """subs_cov.py:113-133.  actions [B] int64 on the device.  Returns (observations, reward [B] f64, done [B] f32, info
        dict of device tensors with the reference's keys) - nothing is synchronised with the host."""
        self._launch(actions.reshape(self.B))
        o = self.out
        self.ep_ret += o["reward"]
        info = dict(EpRet=self.ep_ret, EpLen=self.t, AvgGlobalUtility=self.run_f64[:, 1], FairIdx=self.run_f64[:, 2],
                    TotalThroughput=self.run_f64[:, 0], BadMask=o["done"])     # the only termination is the episode limit (:126)
        return self.observations(), o["reward"], o["done"], info

    def get_env_info(self, agent: str = "gnn") -> dict:
        """The wrapper's ``get_env_info`` (drqn/utils/env_wrappers.py:21-25): agent 'gnn' -> the graph observation's feature
        sizes, 'rnn' -> the flattened width."""
        if agent not in ("gnn", "rnn"):
            raise ValueError(f"agent must be 'gnn' or 'rnn', got {agent!r}")
        obs_shape = 2 + 4 * self.n_gts if agent == "rnn" else dict(agent=2, gt=4)
        return dict(obs_shape=obs_shape, n_actions=self.n_actions, episode_limit=self.episode_limit)
