"""Epoch statistics on the device (csrc/eval_stats.hip): what the reference's logger keeps per key between two ``dump_tabular`` calls
(utils/logx.py:302-307 through ``mpi_statistics_scalar``, utils/mpi_tools.py:78-98: mean, population std, min, max), accumulated by
one launch per push and read with ONE device-to-host copy when the row is printed.

    st = EpochStats(["EpRet", "EpLen", "LossQ", "TestEpRet"], "cuda")
    st.push(EpRet=info["EpRet"], EpLen=info["EpLen"])         # any subset of the keys, equal element counts; no host synchronisation
    row = st.summary()                                        # {AverageEpRet, StdEpRet, MaxEpRet, MinEpRet, NEpRet, NonFiniteEpRet, ...}
    row = st.summary(group)                                   # data-parallel: of ALL ranks' values (one all-gather + ``merge_acc``)
    st.reset()

``push`` copies every tensor into its row of a fixed float64 staging buffer (``copy_`` casts int32 / float32 and reads strided views such
as ``run_f32[:, 1]``) and issues uavgnn_stats_push for every run of keys that are adjacent in ``keys``: fixed addresses, so a push
captures into a hipGraph (``graphs.Episode(stats=...)``, ``graphs.Evaluation(stats=...)``).  The staging buffer grows outside captures
only (earlier buffers stay alive: a graph captured before the growth keeps pushing through the one it was captured with)."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import torch as th

from . import _lib as L

MAX_KEYS_PER_LAUNCH = 16
EMPTY = (0.0, 0.0, 0.0, math.inf, -math.inf, 0.0)       # {count, mean, M2, min, max, non-finite count}


def merge_acc(accs) -> List[List[float]]:
    """The accumulator of all values a list of accumulators saw: ``accs`` holds [K, 6] tables {count, mean, M2, min, max, non-finite count}
    (nested lists, arrays or tensors) and the result is their merge IN LIST ORDER by the pairwise update of uavgnn_stats_push (Chan et
    al.), as nested lists of Python floats - float64 on the host, no launch.  Counts and non-finite counts add, min and max combine; an
    empty accumulator (count 0) is the identity, so the merge of one table is that table, bit for bit."""
    tables = [a.tolist() if hasattr(a, "tolist") else [list(r) for r in a] for a in accs]
    if not tables:
        raise ValueError("merge_acc: an empty list of accumulators")
    if any(len(t) != len(tables[0]) or any(len(r) != 6 for r in t) for t in tables):
        raise ValueError("merge_acc: accumulators of shape [K, 6] with equal K expected")
    out = []
    for rows in zip(*tables):
        count, mean, m2, lo, hi, bad = (float(v) for v in EMPTY)
        for n_b, mean_b, m2_b, lo_b, hi_b, bad_b in rows:
            bad += float(bad_b)
            if not n_b > 0:
                continue
            if count > 0:
                d, n2 = float(mean_b) - mean, count + float(n_b)
                mean, m2 = mean + d * float(n_b) / n2, m2 + (float(m2_b) + d * d * count * float(n_b) / n2)
                count, lo, hi = n2, min(lo, float(lo_b)), max(hi, float(hi_b))
            else:
                count, mean, m2, lo, hi = float(n_b), float(mean_b), float(m2_b), float(lo_b), float(hi_b)
        out.append([count, mean, m2, lo, hi, bad])
    return out


class EpochStats:
    def __init__(self, keys: Sequence[str], device="cuda", cap: int = 64):
        self.keys: List[str] = list(keys)
        if not self.keys or len(set(self.keys)) != len(self.keys):
            raise ValueError("keys: a non-empty list of distinct names expected")
        if cap < 1:
            raise ValueError("cap must be positive")
        self.device = th.device(device)
        self.index = {k: i for i, k in enumerate(self.keys)}
        self.cap = int(cap)
        self._empty = th.tensor([EMPTY] * len(self.keys), dtype=th.float64, device=self.device)
        self.acc = self._empty.clone()
        self.staging = th.zeros(len(self.keys), self.cap, dtype=th.float64, device=self.device)
        self._retired: List[th.Tensor] = []

    def _grow(self, n: int) -> None:
        if th.cuda.is_available() and th.cuda.is_current_stream_capturing():
            raise RuntimeError(f"EpochStats: a push of {n} values per key inside a graph capture exceeds the staging buffer (cap = "
                               f"{self.cap}); push that many once before the capture, or pass cap=")
        self._retired.append(self.staging)       # a graph captured earlier still pushes through it
        self.cap = max(n, 2 * self.cap)
        self.staging = th.zeros(len(self.keys), self.cap, dtype=th.float64, device=self.device)

    def push(self, **tensors: th.Tensor) -> None:
        unknown = [k for k in tensors if k not in self.index]
        if unknown:
            raise ValueError(f"unknown keys {unknown}: this EpochStats holds {self.keys}")
        if not tensors:
            return
        counts = {k: int(t.numel()) for k, t in tensors.items()}
        n = next(iter(counts.values()))
        if any(c != n for c in counts.values()):
            raise ValueError(f"the tensors of one push must hold equal element counts, got {counts}")
        if n == 0:
            return
        L.require_gpu(self.acc, *tensors.values())
        if n > self.cap:
            self._grow(n)
        rows = sorted(self.index[k] for k in tensors)
        for k, t in tensors.items():
            self.staging[self.index[k], :n].copy_(t.detach().reshape(-1), non_blocking=True)
        lib, first = L.lib(), 0
        while first < len(rows):                 # one launch per run of adjacent keys
            last = first
            while last + 1 < len(rows) and rows[last + 1] == rows[last] + 1 and last + 1 - first < MAX_KEYS_PER_LAUNCH:
                last += 1
            k0 = rows[first]
            L.check(lib.uavgnn_stats_push(self.staging.data_ptr() + 8 * k0 * self.cap, self.cap, n, last - first + 1,
                                          self.acc.data_ptr() + 8 * 6 * k0, L.stream()), "uavgnn_stats_push")
            first = last + 1

    def reset(self) -> None:
        self.acc.copy_(self._empty)

    def state_tensors(self) -> List[th.Tensor]:
        """What a graph capture snapshots before its warm-up and restores after the capture."""
        return [self.acc]

    def summary(self, group=None) -> Dict[str, float]:
        """group: a ``torch.distributed`` process group - the accumulators of all its ranks are all-gathered (ONE collective of
        K x 6 doubles) and every rank returns the summary of their merge in rank order (``merge_acc``).  None: this process's alone."""
        if group is None:
            acc = self.acc.cpu().tolist()        # the one device-to-host copy
        else:
            import torch.distributed as dist
            parts = [th.empty_like(self.acc) for _ in range(dist.get_world_size(group))]
            dist.all_gather(parts, self.acc, group=group)
            acc = merge_acc(th.stack(parts).cpu().tolist())
        out: Dict[str, float] = {}
        for k, (count, mean, m2, lo, hi, bad) in zip(self.keys, acc):
            out["Average" + k] = mean if count > 0 else math.nan
            out["Std" + k] = math.sqrt(m2 / count) if count > 0 else math.nan
            out["Max" + k], out["Min" + k] = hi, lo
            out["N" + k], out["NonFinite" + k] = int(count), int(bad)
        return out
