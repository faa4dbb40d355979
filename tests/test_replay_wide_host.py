"""No GPU: the host side of the many-workgroup replay sampler (csrc/replay_wide.hip) - its entries in the ctypes table, the workspace
size over the accepted capacities, the slot chunk of a workgroup, and that the CPU guard of ``device_state=True`` still comes first."""
import pytest

from uav_bs_ctrl_amd import _lib

NAMES = ("uavgnn_replay_sample_wide_workspace_bytes", "uavgnn_replay_sample_wide_slots_per_workgroup", "uavgnn_replay_sample_wide")


def test_the_new_entry_points_are_in_the_signature_table():
    for n in NAMES:
        assert n in _lib.SIGNATURES, n
    assert len(_lib.SIGNATURES["uavgnn_replay_sample_wide"][1]) == len(_lib.SIGNATURES["uavgnn_replay_sample"][1]) + 1, "+ workspace"


def test_workspace_bytes_over_the_accepted_capacities():
    ws = _lib.lib().uavgnn_replay_sample_wide_workspace_bytes
    sizes = [ws(c) for c in (65537, 1 << 20, 1 << 30)]
    assert sizes[0] > 0 and sizes == sorted(sizes), sizes
    assert ws(1) > 0 and ws(65536) > 0, "the wide call is not limited to capacities above the narrow kernel's"
    assert ws(0) <= 0 and ws(-5) <= 0 and ws((1 << 30) + 1) <= 0
    assert sizes[2] <= 16 << 20, "the workspace is O(workgroups), not O(slots)"


def test_slots_per_workgroup():
    assert _lib.lib().uavgnn_replay_sample_wide_slots_per_workgroup() >= 64


def test_argument_errors_are_codes_before_any_launch():
    f = _lib.lib().uavgnn_replay_sample_wide
    assert f(None, None, 70000, 4, None, None, None, None) == _lib.UAVGNN_EINVAL
    assert f(16, 16, 70000, -1, 16, 16, 16, None) == _lib.UAVGNN_EINVAL
    assert f(16, 16, 0, 4, 16, 16, 16, None) == _lib.UAVGNN_EINVAL
    assert f(16, 16, 70000, 4, None, 16, 16, None) == _lib.UAVGNN_EINVAL, "B > 0 with a null idx"
    assert f(16, 16, 70000, 4, 16, 16, None, None) == _lib.UAVGNN_EINVAL, "a null workspace"
    assert f(16, 16, 70000, 4, 16, 16, 24, None) == _lib.UAVGNN_EINVAL, "a workspace that is not 16-byte aligned"
    assert f(16, 16, (1 << 30) + 1, 4, 16, 16, 16, None) == _lib.UAVGNN_EUNSUPPORTED


@pytest.mark.parametrize("single", [False, True], ids=["SequenceReplay", "SingleUbsSequenceReplay"])
def test_the_cpu_guard_of_device_state_comes_before_the_capacity_limit(single, monkeypatch):
    """... and before the ring is allocated: a ring of 2^30 + 1 sequences is hundreds of GB of host memory, so an allocation of that
    size fails the test at once instead of being made."""
    from uav_bs_ctrl_amd import replay
    from uav_bs_ctrl_amd.replay import SequenceReplay, SingleUbsSequenceReplay
    cap = (1 << 30) + 1
    zeros = replay.th.zeros

    def small_zeros(*shape, **kw):
        lead = shape[0][0] if isinstance(shape[0], (tuple, list)) else shape[0]
        assert lead < (1 << 20), f"the ring was allocated ({shape}) before device_state=True was checked against the device"
        return zeros(*shape, **kw)
    monkeypatch.setattr(replay.th, "zeros", small_zeros)
    with pytest.raises(ValueError, match="device_state=True: the ring counters and the sampler live on the GPU"):
        if single:
            SingleUbsSequenceReplay(cap, 2, 3, 8, n_envs=2, device="cpu", device_state=True)
        else:
            SequenceReplay(cap, 2, 3, 5, 8, n_envs=3, state_dim=3, device="cpu", device_state=True)
