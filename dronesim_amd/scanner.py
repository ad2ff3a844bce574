"""Range scanner: a fan of range beams per drone, for every drone (dsim_range_scan).

A watch says how close the nearest thing is, not where; the depth camera says where at thousands of rays per drone, for a few
carriers.  The scanner is the sensor real vehicles carry — a ToF ring, a downward altimeter, a small lidar fan: B <= 64 beams fixed
in the BODY frame, cast from the drone's centre against the obstacle set (or the placements of the drone's scene), the plane
z = 0 and the other drones as their bounding spheres.  The ray and its hits are specified in include/dronesim_amd.h.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _native as nat
from .camera import camera_reach
from .drone_targets import DroneTargets, check_drone_args, offsets_tensor, require_targets
from .obstacles import DeviceObstacles, DeviceScenes, ObstacleScenes, ObstacleSet, scene_ids_tensor

MAX_BEAMS = 64


def unit_beams(beams) -> np.ndarray:
    """[B, 3] float32 unit vectors of ``beams``: normalised in fp64, rounded once.  ValueError for a shape other than [1 .. 64, 3]
    and for a zero or non-finite row."""
    b = np.asarray(beams, dtype=np.float64)
    if b.ndim != 2 or b.shape[1] != 3 or not (1 <= b.shape[0] <= MAX_BEAMS):
        raise ValueError(f"beams must be [B, 3] with 1 <= B <= {MAX_BEAMS}, got shape {b.shape}")
    if not np.isfinite(b).all():
        raise ValueError("beams must be finite")
    with np.errstate(over="ignore"):
        b = b / np.abs(b).max(axis=1, keepdims=True).clip(min=np.finfo(np.float64).tiny)      # (no overflow in the squares)
        norm = np.linalg.norm(b, axis=1, keepdims=True)
    if not (norm > 0.0).all():
        raise ValueError("a beam is zero")
    return (b / norm).astype(np.float32)


class RangeScanner:
    """``world``: an :class:`ObstacleSet` or :class:`ObstacleScenes` (a device set is made for it), a :class:`DeviceObstacles` or
    :class:`DeviceScenes` to share, or None with ``drones`` or ``ground``.  ``beams`` [B, 3], B <= 64, in the body frame (normalised
    here: ranges are metres).  A beam reports the nearest hit with ``t_min`` <= t <= ``t_max``; a miss reads +inf, or ``t_max``
    with ``clamp``.  ``ground``: the plane z = 0 of the task frame.  ``offsets`` [N, 3] and ``scene_id`` [N] are in the CALLER's
    numbering (the world lies in the frame p_i - offset_i; scene_id is required with scenes, an id outside [0, K) meaning no
    obstacles); ``type_id``: uint8 device tensor [n_pad] in storage order, required with several types and ``drones``.

    ``drones=True``: the other drones are targets, as their bounding spheres about their stored positions, up to ``drone_range``
    metres (None: ``t_max``); the fleet is binned per scan on the grid :class:`DepthCamera` uses (``drone_box``, :meth:`refresh_drone_box`,
    :meth:`drones_outside` as there).  Unlike the camera the scanner serves scenes and drones together.

    The scanner owns its outputs, fixed-address tensors [B, n_pad] in STORAGE order that a graph can hold: ``range_out`` float32
    and ``hit_out`` int32 (body index — instance-major g n_bodies + body on scenes —, -1 nothing, -2 the plane, -3 - k drone k of
    the caller's numbering: :meth:`hit_drone`).  :attr:`ranges` and :attr:`hits` give [B, N] in the caller's numbering."""

    def __init__(self, ctx, state, world, beams, t_min=0.0, t_max=10.0, ground=False, clamp=False, offsets=None, type_id=None,
                 scene_id=None, drones=False, drone_range=None, drone_box=None):
        b32 = unit_beams(beams)
        check_range(t_min, t_max)
        drone_box = check_drone_args(drones, drone_range, drone_box)
        if world is None and not (drones or ground):
            raise ValueError("no world at all: world=None needs drones=True or ground=True")
        if world is not None and not isinstance(world, (ObstacleSet, DeviceObstacles, ObstacleScenes, DeviceScenes)):
            raise TypeError("world takes an ObstacleSet, a DeviceObstacles, an ObstacleScenes, a DeviceScenes or None")
        self.placed = isinstance(world, (ObstacleScenes, DeviceScenes))
        if self.placed and scene_id is None:
            raise ValueError("scene_id is required with obstacle scenes")
        if not self.placed and scene_id is not None:
            raise ValueError("scene_id without obstacle scenes")
        if drones and len(ctx.types) > 1 and type_id is None:
            raise ValueError("type_id is required with several drone types and drones=True")
        self.ctx, self.state = ctx, state
        self._owns_set = isinstance(world, (ObstacleSet, ObstacleScenes))
        if self._owns_set:
            world = world.to_device(ctx, camera_reach(ctx.types))
        self.set = world.enable_rays() if world is not None else None
        order = getattr(state, "order", None) or getattr(ctx, "order", None)
        self._order = order
        n, dev = state.n, ctx.device
        self.n_beams = int(b32.shape[0])
        self.beams = b32
        self._beams = torch.from_numpy(b32).to(dev)
        self._scene_id = scene_ids_tensor(scene_id, n, state.n_pad, dev, order) if self.placed else None
        self._off = offsets_tensor(offsets, n, state.n_pad, order, dev)
        self._type_id = type_id
        self._slot = torch.from_numpy(order.slot_np.astype(np.int64)).to(dev) if order is not None else None
        self.range_out = torch.full((self.n_beams, state.n_pad), float("inf"), dtype=torch.float32, device=dev)
        self.hit_out = torch.full((self.n_beams, state.n_pad), -1, dtype=torch.int32, device=dev)
        self.drones = bool(drones)
        self._dr = None
        self._targets = DroneTargets(ctx, state, type_id, order, t_max if drone_range is None else drone_range, drone_box) if drones else None
        if drones:                                 # (kept under the names the tests reach for)
            self._grid, self._outside, self._dr = self._targets.grid, self._targets.outside_count, self._targets.dr
        a = self.args = nat.ScanArgs()
        a.beams, a.n_beams, a.t_min, a.t_max = self._beams.data_ptr(), self.n_beams, float(t_min), float(t_max)
        a.flags = (nat.SCAN_GROUND if ground else 0) | (nat.SCAN_CLAMP if clamp else 0)
        a.offset = self._off.data_ptr() if self._off is not None else None
        a.type_id = type_id.data_ptr() if type_id is not None else None
        a.scenes = self.set.handle if self.placed else None
        a.scene_id = self._scene_id.data_ptr() if self.placed else None
        a.drones = ctypes.addressof(self._dr) if self.drones else None
        a.range_out = self.range_out.data_ptr()

    @staticmethod
    def fan(n_ring, elevations=(0.0,), up=False, down=False) -> np.ndarray:
        """The usual tables, [B, 3] float32 unit beams in the body frame: per elevation (radians above the body's xy plane) a ring
        of ``n_ring`` beams at azimuths 2 pi k / n_ring from the nose (+x) towards +y, ring after ring, then +z with ``up`` and -z
        with ``down``.  ``n_ring`` may be 0 for an altimeter alone."""
        n_ring = int(n_ring)
        if n_ring < 0:
            raise ValueError("n_ring must not be negative")
        rows = []
        for el in elevations:
            el = float(el)
            if not abs(el) < np.pi / 2:
                raise ValueError("an elevation must lie inside (-pi / 2, pi / 2): up / down are the poles")
            az = 2.0 * np.pi * np.arange(n_ring) / max(n_ring, 1)
            rows.append(np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.full(n_ring, np.sin(el))], 1))
        if up:
            rows.append(np.array([[0.0, 0.0, 1.0]]))
        if down:
            rows.append(np.array([[0.0, 0.0, -1.0]]))
        b = np.concatenate(rows) if rows else np.zeros((0, 3))
        if not (1 <= b.shape[0] <= MAX_BEAMS):
            raise ValueError(f"a fan has 1 .. {MAX_BEAMS} beams, got {b.shape[0]}")
        # (cos and sin of the multiples of pi / 2 leave 1e-17s where zeros belong: an axis beam is exactly an axis)
        b[np.abs(b) < 1e-15] = 0.0
        return unit_beams(b)

    def scan(self, hits: bool = True):
        """Enqueues one dsim_range_scan on the current stream (it may be captured into a graph) and returns (range_out, hit_out):
        the scanner's own tensors [B, n_pad] in storage order, overwritten by the next scan.  ``hits=False`` leaves hit_out unwritten
        (None is returned for it)."""
        a = self.args
        a.hit_out = self.hit_out.data_ptr() if hits else None
        if self.drones:
            self._grid_args = self._targets.grid_args()
        nat.check(self.ctx.lib.dsim_range_scan(
            self.ctx.handle, self.ctx.stream_ptr(), self.state.n, self.state.view(),
            self.set.handle if (self.set is not None and not self.placed) else None, ctypes.byref(a)))
        return self.range_out, (self.hit_out if hits else None)

    def _caller(self, t):
        n = self.state.n
        return t[:, :n] if self._slot is None else t.index_select(1, self._slot)

    @property
    def ranges(self):
        """[B, N] float32 in the caller's numbering: a view of range_out where the fleet is stored in the caller's order, else a gather."""
        return self._caller(self.range_out)

    @property
    def hits(self):
        """[B, N] int32 in the caller's numbering (see :attr:`ranges`)."""
        return self._caller(self.hit_out)

    @staticmethod
    def hit_drone(hit):
        """The drone number where a beam hit a drone (hit <= -3: DSIM_SEG_DRONE), -1 elsewhere; a tensor or an array of hit's kind."""
        from .camera import DepthCamera
        return DepthCamera.seg_drone(hit)

    def refresh_drone_box(self) -> None:
        """Has the next eager scan re-measure the box of the drones' grid (no-op with ``drone_box``): for a caller that is about to
        capture a graph, whose scans keep the box and the workspace of the last eager one."""
        require_targets(self._targets, "refresh_drone_box", "scanner").refresh_box()

    def graph_keepalive(self):
        """What a captured scan() holds the addresses of, for the owner of the graph to keep alive."""
        keep = [self.range_out, self.hit_out, self._beams, self._off, self._type_id, self._scene_id]
        if self.drones:
            keep += self._targets.keepalive()
        return tuple(keep)

    def drones_outside(self) -> int:
        """Drones x scans so far that were binned outside the grid's box (synchronises the stream): targets all the same, but
        tested by every beam — a count that grows says the box is stale."""
        return require_targets(self._targets, "drones_outside", "scanner").outside()

    def close(self) -> None:
        if self._owns_set:
            self.set.close()


def check_range(t_min, t_max) -> None:
    """0 <= t_min < t_max, both finite (ValueError otherwise): what dsim_range_scan accepts, in float32 as it sees them."""
    lo, hi = np.float32(t_min), np.float32(t_max)
    if not (np.isfinite(lo) and np.isfinite(hi) and lo >= 0.0 and hi > lo):
        raise ValueError(f"need 0 <= t_min < t_max, both finite, got ({t_min!r}, {t_max!r})")
