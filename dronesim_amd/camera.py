"""Depth camera: per-drone depth and segmentation images of a static obstacle set (dsim_depth_image).

The reference's envs keep, with ``vision_attributes=True``, an image triple per drone from ``p.getCameraImage``
(BaseAviary._getDroneImages, BaseAviary.py:794-853).  Depth and segmentation of the static world are geometry: one ray per pixel
against the set's triangles gives them exactly.  Two deviations from Bullet's renderer: the other drones are not drawn, and there
is no RGB (shading is not reproducible).  The camera model is in include/dronesim_amd.h.

``drones=True`` (dsim_depth_image_drones) draws the other drones as well, with two deviations of its own: a drone is drawn as its
bounding sphere (DroneType.collision_sphere about its stored position), not as its mesh, and the camera's own drone is never
drawn (its eye sits ``arm`` above its own centre, usually inside its own sphere).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _native as nat
from .drone_targets import DroneTargets, check_drone_args, offsets_tensor, require_targets
from .obstacles import DeviceObstacles, DeviceScenes, ObstacleScenes, ObstacleSet, scene_ids_tensor


def camera_reach(types) -> float:
    """The reach a device set made for the camera alone is given (the watch grid still has to be planned): that of a watch
    with margin 1 m."""
    from .obstacles import watch_reach
    return watch_reach(types, 1.0)


class DepthCamera:
    """``cameras``: the drones that carry a camera, in the CALLER's numbering and in the order of the output images (None:
    every drone); ``offsets`` [N, 3] (the caller's numbering): the set lies in the frame p_i - offset_i of each drone's task;
    ``type_id``: uint8 device tensor [n_pad] in storage order, required with several types.  ``obstacle_set``: an
    :class:`ObstacleSet` (a device set is made for it) or a :class:`DeviceObstacles` to share.  The camera owns its outputs:
    ``dep`` float32 [n_cam, H, W] (row 0 at the top, as PyBullet returns it; the depth-buffer value, or metres with
    ``metric=True``) and ``seg`` int32 (body index, -1 nothing, -2 the ground plane).

    ``drones=True``: the other drones of the fleet are drawn as their bounding spheres, up to ``drone_range`` metres of
    eye-space depth (None: ``far``); ``seg`` reports drone k of the CALLER's numbering as -3 - k (:meth:`seg_drone` maps back).
    The fleet is binned per capture on an xy grid over its bounding box, re-measured every 256 captures like the contact
    watch's (one host sync; never under stream capture, where the box of the last eager capture stands), or over ``drone_box`` =
    (xmin, ymin, xmax, ymax); a drone outside the box is still drawn exactly, and :meth:`drones_outside` counts such drones.
    ``obstacle_set`` may then be None: a world of drones and, with ``ground``, the plane.

    Obstacle scenes: ``obstacle_set`` may be an :class:`ObstacleScenes` (device scenes are made for it) or a
    :class:`DeviceScenes` to share; the camera of drone i then sees the placements of scene ``scene_id[i]`` (dsim_depth_image_scenes;
    ``scene_id`` [n] ints in the numbering ``offsets`` uses, required, an id outside [0, K) meaning no obstacles), and ``seg``
    names a hit by the instance-major body index g n_bodies + body.  ``drones=True`` with scenes is not implemented."""

    def __init__(self, ctx, state, obstacle_set, res=(64, 48), fov=60.0, aspect=1.0, far=1000.0, ground=False, metric=False,
                 cameras=None, offsets=None, type_id=None, drones=False, drone_range=None, drone_box=None, scene_id=None):
        w, h = (int(v) for v in res)
        if not (1 <= w <= 1024 and 1 <= h <= 1024):
            raise ValueError(f"res must be (width, height) with 1 <= each <= 1024, got {res!r}")
        if not (0.0 < float(fov) < 180.0):
            raise ValueError("fov must lie in (0, 180) degrees")
        if not (float(aspect) > 0.0 and np.isfinite(aspect)):
            raise ValueError("aspect must be positive")
        if not (float(far) > 0.0 and np.isfinite(far)):
            raise ValueError("far must be positive and finite")
        if any(not float(t.arm) > 0.0 for t in ctx.types):
            raise ValueError("every drone type needs arm > 0: it is the camera's height above the drone and its near plane")
        if len(ctx.types) > 1 and type_id is None:
            raise ValueError("type_id is required with several drone types")
        drone_box = check_drone_args(drones, drone_range, drone_box)
        if obstacle_set is None and not drones:
            raise TypeError("obstacle_set takes an ObstacleSet or a DeviceObstacles (None only with drones=True)")
        self.ctx, self.state = ctx, state
        self.placed = isinstance(obstacle_set, (ObstacleScenes, DeviceScenes))
        if self.placed and drones:
            raise NotImplementedError("drones=True with obstacle scenes: there is no placed dsim_depth_image_drones (the other "
                                      "drones in placed images are a follow-up)")
        if self.placed and scene_id is None:
            raise ValueError("scene_id is required with obstacle scenes")
        if not self.placed and scene_id is not None:
            raise ValueError("scene_id without obstacle scenes")
        self._owns_set = isinstance(obstacle_set, (ObstacleSet, ObstacleScenes))
        if self._owns_set:
            obstacle_set = obstacle_set.to_device(ctx, camera_reach(ctx.types))
        if obstacle_set is not None and not isinstance(obstacle_set, (DeviceObstacles, DeviceScenes)):
            raise TypeError("obstacle_set takes an ObstacleSet, a DeviceObstacles, an ObstacleScenes or a DeviceScenes")
        self.set = obstacle_set.enable_rays() if obstacle_set is not None else None
        order = getattr(state, "order", None) or getattr(ctx, "order", None)
        n, dev = state.n, ctx.device
        self._scene_id = scene_ids_tensor(scene_id, n, state.n_pad, dev, order) if self.placed else None
        self._index = None
        if cameras is None:
            n_cam = n
            if order is not None:                  # image k belongs to drone k of the caller: its storage slot
                self._index = torch.from_numpy(order.slot_np.astype(np.int32)).to(dev)
        else:
            cams = np.asarray(cameras, dtype=np.int64).ravel()
            if cams.size < 1 or cams.min() < 0 or cams.max() >= n:
                raise ValueError(f"cameras must name drones in [0, {n})")
            n_cam = int(cams.size)
            self._index = torch.from_numpy((order.slot_np[cams] if order is not None else cams).astype(np.int32)).to(dev)
        self.n_cam = n_cam
        self._off = offsets_tensor(offsets, n, state.n_pad, order, dev)
        self._type_id = type_id
        self.params = nat.CameraParams(w, h, float(fov), float(aspect), float(far),
                                       (nat.CAM_GROUND if ground else 0) | (nat.CAM_METRIC if metric else 0))
        self.dep = torch.empty((n_cam, h, w), dtype=torch.float32, device=dev)
        self.seg = torch.empty((n_cam, h, w), dtype=torch.int32, device=dev)
        self.drones = bool(drones)
        self._targets = DroneTargets(ctx, state, type_id, order, far if drone_range is None else drone_range, drone_box) if drones else None
        if drones:                                 # (kept under the names the tests reach for)
            self._grid, self._outside, self._dr = self._targets.grid, self._targets.outside_count, self._targets.dr

    def capture(self, seg: bool = True):
        """Enqueues one dsim_depth_image (``drones=True``: dsim_depth_image_drones; scenes: dsim_depth_image_scenes) on the current stream (it may be captured into
        a graph) and returns (dep, seg): the camera's own tensors, overwritten by the next capture.  ``seg=False`` leaves the
        segmentation image unwritten."""
        common = (self._index.data_ptr() if self._index is not None else None, self._off.data_ptr() if self._off is not None else None,
                  self._type_id.data_ptr() if self._type_id is not None else None)
        if self.drones:
            self._grid_args = self._targets.grid_args()
            nat.check(self.ctx.lib.dsim_depth_image_drones(
                self.ctx.handle, self.ctx.stream_ptr(), self.state.view(), self.set.handle if self.set is not None else None,
                ctypes.byref(self.params), self.n_cam, *common, ctypes.byref(self._dr), self.dep.data_ptr(),
                self.seg.data_ptr() if seg else None))
            return self.dep, (self.seg if seg else None)
        if self.placed:
            nat.check(self.ctx.lib.dsim_depth_image_scenes(
                self.ctx.handle, self.ctx.stream_ptr(), self.state.view(), self.set.handle, self._scene_id.data_ptr(),
                ctypes.byref(self.params), self.n_cam, *common, self.dep.data_ptr(), self.seg.data_ptr() if seg else None))
            return self.dep, (self.seg if seg else None)
        nat.check(self.ctx.lib.dsim_depth_image(
            self.ctx.handle, self.ctx.stream_ptr(), self.state.view(), self.set.handle, ctypes.byref(self.params), self.n_cam,
            *common, self.dep.data_ptr(), self.seg.data_ptr() if seg else None))
        return self.dep, (self.seg if seg else None)

    @staticmethod
    def seg_drone(seg):
        """The drone number where a segmentation image shows a drone (seg <= -3: DSIM_SEG_DRONE), -1 elsewhere; a tensor or an
        array of seg's kind."""
        if isinstance(seg, torch.Tensor):
            return torch.where(seg <= -3, -3 - seg, torch.full_like(seg, -1))
        seg = np.asarray(seg)
        return np.where(seg <= -3, -3 - seg, -1)

    def refresh_drone_box(self) -> None:
        """Has the next eager capture re-measure the box of the drones' grid (no-op with ``drone_box``): for a caller that is about
        to capture a graph, whose captures keep the box and the workspace of the last eager one."""
        require_targets(self._targets, "refresh_drone_box", "camera").refresh_box()

    def graph_keepalive(self):
        """What a captured capture() holds the addresses of, for the owner of the graph to keep alive: an eager capture that later
        re-measures the box and outgrows the drones' workspace makes a new one, and the old must outlive the graph."""
        keep = [self.dep, self.seg, self._index, self._off, self._type_id, self._scene_id]
        if self.drones:
            keep += self._targets.keepalive()
        return tuple(keep)

    def drones_outside(self) -> int:
        """Drones x captures so far that were binned outside the grid's box (synchronises the stream): drawn all the same, but
        tested by every ray — a count that grows says the box (``drone_box``, or the one a graph was captured with) is stale."""
        return require_targets(self._targets, "drones_outside", "camera").outside()

    def close(self) -> None:
        if self._owns_set:
            self.set.close()
