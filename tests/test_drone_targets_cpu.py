"""dronesim_amd.drone_targets on the CPU: the argument handling DepthCamera and RangeScanner share (no device: the sensors
themselves are tests/test_gpu_camera_drones.py and tests/test_gpu_scan.py)."""
import numpy as np
import pytest
import torch

from dronesim_amd.drone_targets import check_drone_args, offsets_tensor, require_targets
from dronesim_amd.fleet import StorageOrder


def test_drone_args_are_refused_without_drones_and_out_of_range():
    assert check_drone_args(False, None, None) is None and check_drone_args(True, None, None) is None
    assert check_drone_args(True, 5.0, None) is None
    box = check_drone_args(True, None, [-1, -2, 3, np.float32(4)])
    assert box == (-1.0, -2.0, 3.0, 4.0) and all(type(v) is float for v in box)
    assert check_drone_args(True, 1e-3, (0, 0, 0, 0)) == (0.0, 0.0, 0.0, 0.0)             # a degenerate box is a box
    for kw in (dict(drone_range=5.0, drone_box=None), dict(drone_range=None, drone_box=(0, 0, 1, 1))):
        with pytest.raises(ValueError, match="without drones=True"):
            check_drone_args(False, **kw)
    for r in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="drone_range must be positive"):
            check_drone_args(True, r, None)
    for b in ((0, 0, 1), (0, 0, 1, 1, 1), (0, 0, float("inf"), 1), (0, float("nan"), 1, 1), (2, 0, 1, 1), (0, 2, 1, 1)):
        with pytest.raises(ValueError, match=r"drone_box must be \(xmin, ymin, xmax, ymax\)"):
            check_drone_args(True, None, b)


@pytest.mark.parametrize("noun", ["camera", "scanner"])
def test_a_sensor_without_drones_is_named_in_the_refusal(noun):
    t = object()
    assert require_targets(t, "drones_outside", noun) is t
    for method in ("refresh_drone_box", "drones_outside"):
        with pytest.raises(ValueError) as e:
            require_targets(None, method, noun)
        assert str(e.value) == f"{method}() needs a {noun} made with drones=True"


def test_offsets_tensor_is_soa_in_storage_order_and_zero_in_the_padding():
    n, n_pad = 7, 64
    off = np.arange(3 * n, dtype=np.float64).reshape(n, 3) + 0.25
    assert offsets_tensor(None, n, n_pad, None, "cpu") is None
    t = offsets_tensor(off, n, n_pad, None, "cpu")
    assert t.shape == (3, n_pad) and t.dtype == torch.float32 and t.is_contiguous()
    np.testing.assert_array_equal(t.numpy()[:, :n], off.T.astype(np.float32))
    assert not t[:, n:].any()
    # a type-major fleet: slot s holds the offset of drone order.drone_np[s]
    order = StorageOrder(np.array([1, 0, 1, 0, 0, 2, 1], dtype=np.uint8), "cpu")
    assert not np.array_equal(order.drone_np, np.arange(n))
    s = offsets_tensor(off.tolist(), n, n_pad, order, "cpu")                              # (any array-like)
    np.testing.assert_array_equal(s.numpy()[:, :n], off[order.drone_np].T.astype(np.float32))
    np.testing.assert_array_equal(s.numpy()[:, order.slot_np], off.T.astype(np.float32))
    assert not s[:, n:].any()
    for bad in (off[:-1], off[:, :2], off.T, off.ravel()):
        with pytest.raises(ValueError, match=rf"offsets must be \[{n}, 3\]"):
            offsets_tensor(bad, n, n_pad, order, "cpu")
