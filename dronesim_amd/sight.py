"""Line of sight: which of a drone's neighbours its obstacles hide, per slot (dsim_line_of_sight).

The nearest-neighbour observation tells a drone who its neighbours are and how they move — through walls; the watches, the scanner
and the camera know the walls, not the neighbours behind them.  :class:`LineOfSight` casts the segment from every drone to each of
the points a ``rel`` record names (a knn record's ``rel_pos``, or any target: ``rel = goal - p``) against the obstacle set (or the
placements of the drone's scene) and the plane z = 0, and says per slot whether it is clear, what hides it first and where.  The
segment and its hits are specified in include/dronesim_amd.h.  The other drones hide nobody unless asked: with ``drones=True``
every other drone hides too, as its bounding sphere (dsim_line_of_sight_drones) — in a column of three the middle one hides the far one.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import torch

from . import _native as nat
from .camera import camera_reach
from .drone_targets import DroneTargets, check_drone_args, offsets_tensor, require_targets
from .obstacles import DeviceObstacles, DeviceScenes, ObstacleScenes, ObstacleSet, scene_ids_tensor

MAX_K = nat.SIGHT_MAX_K


class Sight(NamedTuple):
    """What :meth:`LineOfSight.query` saw: slot t of drone i.  A member that was not asked for is None."""

    visible: torch.Tensor              # [k, n] int32: 1 = cast and nothing on the segment; 0 = blocked, or not cast
    blocker: Optional[torch.Tensor]    # [k, n] int32: body of the first hit (instance-major g n_bodies + body on scenes), -2 the plane, -1 none,
                                       # -3 - j drone j of the caller's numbering (drones=True: LineOfSight.seg_drone)
    frac: Optional[torch.Tensor]       # [k, n] float32: where on the segment (0 at the drone, 1 at the target), +inf none

    def mask(self) -> torch.Tensor:
        """[n] int32: bit t set where slot t is visible (with 32 slots bit 31 is the sign)."""
        k = self.visible.shape[0]
        sh = torch.arange(k, dtype=torch.int64, device=self.visible.device)[:, None]
        return ((self.visible != 0).to(torch.int64) << sh).sum(0).to(torch.int32)


class LineOfSight:
    """``world``: an :class:`ObstacleSet` or :class:`ObstacleScenes` (a device set is made for it), a :class:`DeviceObstacles` or
    :class:`DeviceScenes` to share, or None with ``ground`` or ``drones``.  ``k`` (1 .. 32): the slots of every query.  ``ground``: the plane
    z = 0 of the task frame hides too.  ``offsets`` [N, 3] and ``scene_id`` [N] are in the CALLER's numbering (the world lies in the
    frame p_i - offset_i; scene_id is required with scenes, an id outside [0, K) meaning no obstacles).  The segment of slot t of
    drone i lies in drone i's task frame: with offsets, i may see j where j does not see i.

    ``drones=True``: the other drones hide too, as solid balls of their type's collision_sphere about their STORED positions, met
    from the stored p_i (the offsets move the triangles' frame, not the spheres).  Drone i never blocks, nor does the slot's own
    target ``index[t, i]``; with ``index=None`` only i is left out.  A drone that stands inside another's ball has every slot
    blocked at frac 0.  ``blocker`` names drone j of the caller's numbering as -3 - j (:meth:`seg_drone`).  The fleet is binned per
    query on the grid :class:`DepthCamera` uses (``drone_box``, :meth:`refresh_drone_box`, :meth:`drones_outside` as there);
    ``type_id``: uint8 device tensor [n_pad] in storage order, required with several types.  ``targets``: a :class:`DroneTargets`
    of reach 1 to share (the env's on-demand queries bin through the per-launch object's).

    The object owns its outputs, fixed-address tensors [k, n_pad] in STORAGE order that a graph can hold: ``visible_out`` and
    ``blocker_out`` int32, ``frac_out`` float32."""

    def __init__(self, ctx, state, world, k, ground=False, offsets=None, scene_id=None, drones=False, drone_box=None, type_id=None,
                 targets=None):
        if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= MAX_K:
            raise ValueError(f"k must be a whole number of slots in 1 .. {MAX_K}")
        drone_box = check_drone_args(drones, None, drone_box)
        if targets is not None and not drones:
            raise ValueError("targets without drones=True")
        if world is None and not (ground or drones):
            raise ValueError("no world at all: world=None needs ground=True or drones=True")
        if world is not None and not isinstance(world, (ObstacleSet, DeviceObstacles, ObstacleScenes, DeviceScenes)):
            raise TypeError("world takes an ObstacleSet, a DeviceObstacles, an ObstacleScenes, a DeviceScenes or None")
        self.placed = isinstance(world, (ObstacleScenes, DeviceScenes))
        if self.placed and scene_id is None:
            raise ValueError("scene_id is required with obstacle scenes")
        if not self.placed and scene_id is not None:
            raise ValueError("scene_id without obstacle scenes")
        if drones and len(ctx.types) > 1 and type_id is None:
            raise ValueError("type_id is required with several drone types and drones=True")
        self.ctx, self.state, self.k = ctx, state, int(k)
        self._owns_set = isinstance(world, (ObstacleSet, ObstacleScenes))
        if self._owns_set:
            world = world.to_device(ctx, camera_reach(ctx.types))
        self.set = world.enable_rays() if world is not None else None
        order = getattr(state, "order", None) or getattr(ctx, "order", None)
        n, n_pad, dev = state.n, state.n_pad, ctx.device
        self._scene_id = scene_ids_tensor(scene_id, n, n_pad, dev, order) if self.placed else None
        self._off = offsets_tensor(offsets, n, n_pad, order, dev)
        self.visible_out = torch.zeros((self.k, n_pad), dtype=torch.int32, device=dev)
        self.blocker_out = torch.full((self.k, n_pad), -1, dtype=torch.int32, device=dev)
        self.frac_out = torch.full((self.k, n_pad), float("inf"), dtype=torch.float32, device=dev)
        a = self.args = nat.SightArgs()
        a.k, a.flags = self.k, (nat.SIGHT_GROUND if ground else 0)
        a.offset = self._off.data_ptr() if self._off is not None else None
        a.scenes = self.set.handle if self.placed else None
        a.scene_id = self._scene_id.data_ptr() if self.placed else None
        a.visible_out = self.visible_out.data_ptr()
        # drones->range bounds s: 1, the whole segment
        self.drones = bool(drones)
        self._type_id = type_id
        self._targets = (targets if targets is not None else DroneTargets(ctx, state, type_id, order, 1.0, drone_box)) if drones else None

    def _padded(self, t, name, dtype, mid):
        """``t`` as the library reads it: [k, *mid, n_pad] contiguous, or its first n drones cut from such a tensor (what
        Downwash.nearest returns).  ValueError otherwise."""
        n, n_pad = self.state.n, self.state.n_pad
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != self.visible_out.device:
            raise ValueError(f"{name} must be a {dtype} tensor on the fleet's device")
        full, cut = (self.k, *mid, n_pad), (self.k, *mid, n)
        strides = tuple(torch.empty(full, device="meta").stride())
        if not ((tuple(t.shape) == full or tuple(t.shape) == cut) and tuple(t.stride()) == strides):
            raise ValueError(f"{name} must be a contiguous {list(full)} in storage order, or its first {n} drones")
        return t

    def query(self, rel, index=None, blocker: bool = True, frac: bool = True) -> Sight:
        """Enqueues one dsim_line_of_sight (``drones=True``: dsim_line_of_sight_drones) on the current stream (it may be captured into a graph).  ``rel`` float32
        [k, 3, n_pad] in storage order (or its first n drones, cut from such a tensor: a knn record's ``rel_pos``): slot t of drone
        i looks from p_i - offset_i along rel[t, :, i], to its end.  ``index`` int32 [k, n_pad] (likewise) or None: a slot whose
        index is negative is not cast.  Returns ``Sight(visible, blocker, frac)``: views [k, n] of the object's own tensors, in
        storage order, overwritten by the next query; ``blocker=False`` / ``frac=False`` leave that output unwritten (None is
        returned for it).  A slot that is not cast — a negative index, a zero or non-finite rel, a non-finite position — reads
        0 / -1 / +inf."""
        rel = self._padded(rel, "rel", torch.float32, (3,))
        if index is not None:
            index = self._padded(index, "index", torch.int32, ())
        a = self.args
        a.rel, a.index = rel.data_ptr(), (index.data_ptr() if index is not None else None)
        a.blocker_out = self.blocker_out.data_ptr() if blocker else None
        a.frac_out = self.frac_out.data_ptr() if frac else None
        self._inputs = (rel, index)                # (the kernel reads these asynchronously on the stream)
        world = self.set.handle if (self.set is not None and not self.placed) else None
        if self.drones:
            self._grid_args = self._targets.grid_args()
            nat.check(self.ctx.lib.dsim_line_of_sight_drones(
                self.ctx.handle, self.ctx.stream_ptr(), self.state.n, self.state.view(), world, ctypes.byref(a),
                self._type_id.data_ptr() if self._type_id is not None else None, ctypes.byref(self._targets.dr)))
        else:
            nat.check(self.ctx.lib.dsim_line_of_sight(
                self.ctx.handle, self.ctx.stream_ptr(), self.state.n, self.state.view(), world, ctypes.byref(a)))
        n = self.state.n
        return Sight(self.visible_out[:, :n], self.blocker_out[:, :n] if blocker else None, self.frac_out[:, :n] if frac else None)

    def query_neighbors(self, nb, blocker: bool = True, frac: bool = True) -> Sight:
        """:meth:`query` on a knn record in storage order (Downwash.nearest): its ``rel_pos`` and ``index``."""
        if nb.rel_pos is None:
            raise ValueError("the record has no rel_pos (Downwash.nearest(rel_pos=True))")
        return self.query(nb.rel_pos, nb.index, blocker=blocker, frac=frac)

    def graph_keepalive(self):
        """What a captured query() holds the addresses of, for the owner of the graph to keep alive."""
        keep = (self.visible_out, self.blocker_out, self.frac_out, self._off, self._scene_id) + tuple(getattr(self, "_inputs", ()))
        if self.drones:
            keep += (self._type_id,) + tuple(self._targets.keepalive())
        return keep

    @staticmethod
    def seg_drone(blocker):
        """The drone number where a drone hides the slot (blocker <= -3: DSIM_SEG_DRONE), -1 elsewhere; a tensor or an array of
        blocker's kind."""
        from .camera import DepthCamera
        return DepthCamera.seg_drone(blocker)

    def refresh_drone_box(self) -> None:
        """Has the next eager query re-measure the box of the drones' grid (no-op with ``drone_box``): for a caller that is about
        to capture a graph, whose queries keep the box and the workspace of the last eager one."""
        require_targets(self._targets, "refresh_drone_box", "line of sight").refresh_box()

    def drones_outside(self) -> int:
        """Drones x queries so far that were binned outside the grid's box (synchronises the stream): they hide all the same,
        but are tested by every segment — a count that grows says the box is stale."""
        return require_targets(self._targets, "drones_outside", "line of sight").outside()

    def close(self) -> None:
        if self._owns_set:
            self.set.close()
