"""`-m gpu`: the f16x2 kernels reproduce, bit for bit, what they computed before the split helper of csrc/f16x2.h moved to mixed-precision
FMAs and the three files to a build without packed fp32: uavgnn_gemm_nt_h2 (plain, ReLU, accumulate, accumulate + ReLU; two sources),
uavgnn_gemm_nt_h2_rm2 with its row maxima, uavgnn_gemm_nt_h2_n64, uavgnn_gemm_tn_h2 (64 and 256 rows in two chunks, accumulating) and
uavgnn_gru_cell_fwd_h2 (no-grad and training with every saved set) on the seeded operands of tools/record_f16x2_golden.py, whose
magnitudes reach 2^-30 of their row / column bound (lo terms and f16 subnormals in the in-loop staging).  The fixtures under
tests/golden/f16x2_mix/ were written by that tool on the earlier build; per output they hold the SHA-256 of the whole int32 image and
the image itself (whole up to 64 KB, every fourth row and the last two beyond).
A recording pins bits, right or wrong.  That the ragged shapes pinned here are RIGHT - the clamped row of M = 257, the partial column
block of N = 192, the second source's first slice at K1 = 32 of K = 64, the n64 kernel at M = 129, the cell at N = 129 with a two-piece
input - is checked against float64, entry by entry, in tests/test_f16x2_nt_edges_gpu.py and tests/test_gru_cell_h2_edges_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch as th

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_f16x2_golden as rec  # noqa: E402

NAMES = ["nt_plain", "nt_relu", "nt_acc", "nt_acc_relu", "nt_rm2", "nt_rm2_rowmax2", "nt_n64", "tn_64", "tn_256", "tn_256_acc",
         "gru_nograd_h", "gru_train_h", "gru_train_pre"]


@pytest.fixture(scope="module")
def computed():
    return {k: rec.image(v) for k, v in rec.compute().items()}


def test_every_recorded_output_has_a_case(computed):
    assert sorted(computed) == sorted(NAMES)
    assert sorted(f[:-4] for f in os.listdir(rec.GOLDEN) if f.endswith(".npz")) == sorted(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_bits_equal_the_recorded_build(computed, name):
    gold = np.load(os.path.join(rec.GOLDEN, name + ".npz"))
    bits = computed[name]
    assert tuple(gold["shape"]) == bits.shape
    rows = gold["rows"].astype(np.int64)
    got, want = th.from_numpy(np.ascontiguousarray(bits[rows])), th.from_numpy(gold["bits"])
    if not th.equal(got, want):
        bad = (got != want).nonzero()
        r, c = int(bad[0, 0]), int(bad[0, 1])
        pytest.fail(f"{name}: {len(bad)} of {got.numel()} recorded elements differ, first at row {int(rows[r])} column {c}: "
                    f"{int(got[r, c]):#010x} against {int(want[r, c]):#010x}")
    assert rec.digest(bits) == gold["sha256"].tobytes().decode(), f"{name}: a row outside the recorded sample differs"


def test_no_grad_and_training_cells_agree(computed):
    assert np.array_equal(computed["gru_nograd_h"], computed["gru_train_h"])
