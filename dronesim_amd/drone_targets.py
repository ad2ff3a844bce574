"""The other drones as targets of a ray sensor: what :class:`DepthCamera` and :class:`RangeScanner` build alike with ``drones=True``
(the record dsim_camera_drones of include/dronesim_amd.h and what it points to), and the argument handling the two share."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _native as nat


def check_drone_args(drones, drone_range, drone_box):
    """ValueError for ``drone_range`` / ``drone_box`` without ``drones``, a range that is not positive or a box that is not four
    finite numbers (xmin, ymin, xmax, ymax); returns the box as a tuple of floats, or None."""
    if not drones and (drone_range is not None or drone_box is not None):
        raise ValueError("drone_range / drone_box without drones=True")
    if drone_range is not None and not float(drone_range) > 0.0:
        raise ValueError("drone_range must be positive")
    if drone_box is not None:
        drone_box = tuple(float(v) for v in drone_box)
        if len(drone_box) != 4 or not all(np.isfinite(drone_box)) or not (drone_box[0] <= drone_box[2] and drone_box[1] <= drone_box[3]):
            raise ValueError("drone_box must be (xmin, ymin, xmax, ymax)")
    return drone_box


def require_targets(targets, method, noun):
    """The sensor's :class:`DroneTargets`, or ValueError where the ``noun`` ("camera", "scanner") was made without ``drones=True``."""
    if targets is None:
        raise ValueError(f"{method}() needs a {noun} made with drones=True")
    return targets


def offsets_tensor(offsets, n, n_pad, order, dev):
    """``offsets`` [n, 3] in the caller's numbering as the kernels read them: float32 SoA [3, n_pad] in storage order (``order``: the
    fleet's type-major order, or None), zero beyond n; None for None."""
    if offsets is None:
        return None
    off = np.asarray(offsets, dtype=np.float64)
    if off.shape != (n, 3):
        raise ValueError(f"offsets must be [{n}, 3]")
    if order is not None:
        off = order.to_storage_np(off)
    t = torch.zeros((3, n_pad), dtype=torch.float32)
    t[:, :n] = torch.from_numpy(np.ascontiguousarray(off.T)).float()
    return t.to(dev)


class DroneTargets:
    """The fleet as bounding spheres up to ``reach`` metres along a ray.  It is binned per call on an xy grid over its bounding
    box, re-measured every 256 calls like the contact watch's, or over ``box`` = (xmin, ymin, xmax, ymax); ``dr`` is the record a
    call passes, valid once :meth:`grid_args` has run for it."""

    def __init__(self, ctx, state, type_id, order, reach, box=None):
        from .downwash import Downwash
        self.grid = Downwash(ctx, state, type_id, None)      # the helper the contact watch bins with
        self.box = box
        # storage slot -> the caller's number (a type-major fleet): what a hit names a drone by
        self.label = torch.from_numpy(order.drone_np.astype(np.int32)).to(ctx.device) if order is not None else None
        self.outside_count = torch.zeros((1,), dtype=torch.int64, device=ctx.device)
        self.args = None
        self.dr = nat.CameraDrones()
        self.dr.radius_all = None
        self.dr.label = self.label.data_ptr() if self.label is not None else None
        self.dr.range = float(reach)
        self.dr.outside_out = self.outside_count.data_ptr()

    def grid_args(self):
        """The grid of the next call, planned and pointed to by ``dr`` (kept in ``args``: the struct outlives the call)."""
        self.args = self.grid.sphere_grid(self.box)
        self.dr.grid = ctypes.addressof(self.args)
        return self.args

    def refresh_box(self) -> None:
        """Has the next eager call re-measure the grid's box (no-op with ``box``)."""
        self.grid._box = None

    def outside(self) -> int:
        """Drones x calls so far that were binned outside the grid's box (synchronises the stream)."""
        return int(self.outside_count.item())

    def keepalive(self):
        """What a captured call holds the addresses of, beyond the sensor's own tensors."""
        return [self.grid._ws, self.label, self.outside_count]
