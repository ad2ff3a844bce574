"""Static obstacles of the world as triangle soups: the input of the static-obstacle watch (dsim_obstacle_clearance).

The reference flies in a Bullet world into which static bodies are loaded (``p.loadURDF`` of a gate:
examples/fly_INDI_TrajectoryTrack.py:216-221); a body marked ``concave="yes"`` collides against its triangles.  An
:class:`ObstacleSet` holds such bodies as fp32 triangles, each with the index of the body it belongs to; nothing here needs a
device until :meth:`ObstacleSet.to_device`.
"""
from __future__ import annotations

import ctypes
import os
import typing
import xml.etree.ElementTree as etxml

import numpy as np

from . import _native as nat


def _rot(rpy) -> np.ndarray:
    """URDF / Bullet fixed-axis roll-pitch-yaw: R = Rz(yaw) Ry(pitch) Rx(roll)."""
    r, p, y = (float(v) for v in rpy)
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                     [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                     [-sp, cp * sr, cp * cr]])


def _vec(text, n=3) -> np.ndarray:
    v = np.array([float(s) for s in str(text).split()], dtype=np.float64)
    if v.size != n:
        raise ValueError(f"expected {n} numbers, got {text!r}")
    return v


def read_obj(path: str):
    """The ``v`` and ``f`` lines of a Wavefront file: (vertices [V, 3] float64, faces [F, 3] int64, 0-based).  ``f`` entries
    of the forms i, i/j, i//k and i/j/k; negative indices count from the end; polygons are fanned from their first vertex."""
    verts, faces = [], []
    with open(path) as fh:
        for ln in fh:
            tok = ln.split()
            if not tok:
                continue
            if tok[0] == "v":
                verts.append([float(x) for x in tok[1:4]])
            elif tok[0] == "f":
                idx = [int(t.split("/")[0]) for t in tok[1:]]
                idx = [i - 1 if i > 0 else len(verts) + i for i in idx]
                if len(idx) < 3:
                    raise ValueError(f"{path}: face with {len(idx)} vertices")
                faces.extend([idx[0], idx[k], idx[k + 1]] for k in range(1, len(idx) - 1))
    v, f = np.array(verts, dtype=np.float64).reshape(-1, 3), np.array(faces, dtype=np.int64).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError(f"{path}: face index out of range")
    return v, f


_BOX_FACES = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4],
                       [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6], [1, 3, 5], [3, 7, 5]], dtype=np.int64)


class DeviceObstacles:
    """The library's device copy of a set (dsim_obstacles_create): records, grid and cell lists for one ``reach``."""

    def __init__(self, ctx, tri: np.ndarray, body: np.ndarray, reach: float):
        self.ctx, self.reach, self.n_tri = ctx, float(np.float32(reach)), int(tri.shape[0])
        self._tri = np.ascontiguousarray(tri, dtype=np.float32).reshape(-1, 9)
        self._body = np.ascontiguousarray(body, dtype=np.int32)
        self._h = ctypes.c_void_p()
        nat.check(ctx.lib.dsim_obstacles_create(ctx.handle, self._tri.ctypes.data, self._body.ctypes.data, self.n_tri,
                                                self.reach, ctypes.byref(self._h)))

    @property
    def handle(self):
        return self._h

    def enable_rays(self) -> "DeviceObstacles":
        """The set's ray grid for the depth camera (dsim_obstacles_enable_rays: host work, an upload and a synchronisation, not
        inside a graph capture; nothing happens when the set already has it)."""
        nat.check(self.ctx.lib.dsim_obstacles_enable_rays(self.ctx.handle, self._h))
        return self

    def close(self) -> None:
        if self._h:
            self.ctx.lib.dsim_obstacles_destroy(None, self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ObstacleSet:
    """Triangles [T, 3, 3] (float32, world frame of the drone's task) and the body index [T] of each."""

    def __init__(self, triangles, body):
        self.triangles = np.ascontiguousarray(np.asarray(triangles, dtype=np.float32).reshape(-1, 3, 3))
        self.body = np.ascontiguousarray(np.broadcast_to(np.asarray(body, dtype=np.int32), (self.triangles.shape[0],)))
        if self.triangles.shape[0] == 0:
            raise ValueError("an obstacle set needs at least one triangle")
        if not np.isfinite(self.triangles).all():
            raise ValueError("non-finite vertex coordinate")
        if self.body.min() < 0:
            raise ValueError("body indices are >= 0")
        t = self.triangles.astype(np.float64)
        area = 0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1)
        if area.min() < 1e-12:
            raise ValueError(f"triangle {int(area.argmin())} has area {area.min():.3e} m^2 (below 1e-12)")

    # ---- constructors ---------------------------------------------------------------------------------------------------
    @classmethod
    def from_triangles(cls, vertices, faces, body=0) -> "ObstacleSet":
        v, f = np.asarray(vertices, dtype=np.float64).reshape(-1, 3), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
        if f.size and (f.min() < 0 or f.max() >= len(v)):
            raise ValueError("face index out of range")
        return cls(v[f], body)

    @classmethod
    def box(cls, centre, size, rpy=(0, 0, 0)) -> "ObstacleSet":
        """A box of full edge lengths ``size`` about ``centre``: 12 triangles."""
        h = 0.5 * np.asarray(size, dtype=np.float64).reshape(3)
        corners = np.array([[sx, sy, sz] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)], dtype=np.float64) * h
        v = corners @ _rot(rpy).T + np.asarray(centre, dtype=np.float64)
        return cls.from_triangles(v, _BOX_FACES)

    @classmethod
    def from_obj(cls, path, scale=(1, 1, 1), position=(0, 0, 0), rpy=(0, 0, 0)) -> "ObstacleSet":
        v, f = read_obj(path)
        v = (v * np.asarray(scale, dtype=np.float64)) @ _rot(rpy).T + np.asarray(position, dtype=np.float64)
        return cls.from_triangles(v, f)

    @classmethod
    def from_urdf(cls, path, position=(0, 0, 0), rpy=(0, 0, 0)) -> "ObstacleSet":
        """Every ``<collision>`` of every link of a static body, placed at ``position`` / ``rpy`` (what p.loadURDF takes): one
        body.  A ``<mesh>`` only when its link or its collision says ``concave="yes"`` — without the flag Bullet collides
        against the mesh's convex hull, which the triangles are not; ``<box>``; any other shape is a ValueError.  So is a file
        with a ``<joint>`` or more than one ``<link>``: joint origins are not composed, and the links would be misplaced."""
        root = etxml.parse(path).getroot()
        n_links, n_joints = len(list(root.iter("link"))), len(list(root.iter("joint")))
        if n_links != 1 or n_joints:
            raise ValueError(f"{path}: {n_links} links and {n_joints} joints: only a static body of one link is supported")
        base_r, base_t = _rot(rpy), np.asarray(position, dtype=np.float64)
        tris = []
        for link in root.iter("link"):
            for col in link.findall("collision"):
                org = col.find("origin")
                o_t = _vec(org.attrib.get("xyz", "0 0 0")) if org is not None else np.zeros(3)
                o_r = _rot(_vec(org.attrib.get("rpy", "0 0 0"))) if org is not None else np.eye(3)
                geo = col.find("geometry")
                shape = geo[0] if geo is not None and len(geo) else None
                if shape is None:
                    raise ValueError(f"{path}: <collision> of link {link.attrib.get('name')!r} has no geometry")
                if shape.tag == "mesh":
                    if "yes" not in (link.attrib.get("concave", "no"), col.attrib.get("concave", "no")):
                        raise ValueError(f"{path}: the <mesh> of link {link.attrib.get('name')!r} is not concave=\"yes\": Bullet "
                                         "would collide against its convex hull, which its triangles are not")
                    v, f = read_obj(os.path.join(os.path.dirname(os.path.abspath(path)), shape.attrib["filename"]))
                    local = (v * _vec(shape.attrib.get("scale", "1 1 1")))[f]
                elif shape.tag == "box":
                    local = cls.box((0, 0, 0), _vec(shape.attrib["size"])).triangles.astype(np.float64)
                else:
                    raise ValueError(f"{path}: collision shape <{shape.tag}> is not supported (a concave <mesh> or a <box>)")
                tris.append((local @ o_r.T + o_t) @ base_r.T + base_t)
        if not tris:
            raise ValueError(f"{path}: no <collision>")
        return cls(np.concatenate(tris), 0)

    # ---- the set ----------------------------------------------------------------------------------------------------------
    def __add__(self, other: "ObstacleSet") -> "ObstacleSet":
        """Both sets' triangles; the bodies of ``other`` are numbered behind this set's."""
        if not isinstance(other, ObstacleSet):
            return NotImplemented
        return ObstacleSet(np.concatenate([self.triangles, other.triangles]),
                           np.concatenate([self.body, other.body + self.n_bodies]))

    @property
    def n_tri(self) -> int:
        return int(self.triangles.shape[0])

    @property
    def n_bodies(self) -> int:
        return int(self.body.max()) + 1

    @property
    def aabb(self):
        """(lo [3], hi [3]) of the vertices, float32."""
        v = self.triangles.reshape(-1, 3)
        return v.min(0), v.max(0)

    def grid(self, reach: float):
        """The host-side grid of this set for ``reach`` (dsim_obstacle_grid_plan / _build; needs no device):
        (nat.ObstacleGrid, cell_start int32 [cells + 1], cell_tri int32 [list_len])."""
        lib = nat.load()
        tri = np.ascontiguousarray(self.triangles.reshape(-1, 9))
        g = nat.ObstacleGrid()
        nat.check(lib.dsim_obstacle_grid_plan(tri.ctypes.data, self.n_tri, float(reach), ctypes.byref(g)))
        start = np.zeros(g.nx * g.ny * g.nz + 1, dtype=np.int32)
        lst = np.zeros(max(int(g.list_len), 1), dtype=np.int32)
        nat.check(lib.dsim_obstacle_grid_build(tri.ctypes.data, self.n_tri, ctypes.byref(g), start.ctypes.data, lst.ctypes.data))
        return g, start, lst[: int(g.list_len)]

    def ray_grid(self):
        """The host-side RAY grid of this set (dsim_obstacle_ray_grid_plan / _build; needs no device): a triangle is listed in
        the cells its own bounding box touches.  (nat.ObstacleGrid, cell_start int32 [cells + 1], cell_tri int32 [list_len])."""
        lib = nat.load()
        tri = np.ascontiguousarray(self.triangles.reshape(-1, 9))
        g = nat.ObstacleGrid()
        nat.check(lib.dsim_obstacle_ray_grid_plan(tri.ctypes.data, self.n_tri, ctypes.byref(g)))
        start = np.zeros(g.nx * g.ny * g.nz + 1, dtype=np.int32)
        lst = np.zeros(max(int(g.list_len), 1), dtype=np.int32)
        nat.check(lib.dsim_obstacle_ray_grid_build(tri.ctypes.data, self.n_tri, ctypes.byref(g), start.ctypes.data, lst.ctypes.data))
        return g, start, lst[: int(g.list_len)]

    def to_device(self, ctx, reach: float) -> DeviceObstacles:
        """The library's device set for queries with R_max + margin <= ``reach`` (allocates, uploads, synchronises: not
        inside a graph capture)."""
        return DeviceObstacles(ctx, self.triangles, self.body, reach)


def watch_reach(types, margin: float) -> float:
    """The least ``reach`` a query of ``margin`` over these drone types accepts: fp32(R_max) + fp32(margin), a thousandth more so
    that no rounding of the sum undercuts it."""
    r_max = max(float(np.float32(t.collision_sphere)) for t in types)
    return float(np.float32((r_max + float(np.float32(margin))) * (1.0 + 2.0 ** -10)))


def query(ctx, state, dev: DeviceObstacles, margin: float, clearance, nearest, offset=None, type_id=None, contacts_out=None) -> None:
    """dsim_obstacle_clearance on the current stream into the given tensors ([n_pad] float32 / int32)."""
    nat.check(ctx.lib.dsim_obstacle_clearance(
        ctx.handle, ctx.stream_ptr(), state.n, state.view(), dev.handle, offset.data_ptr() if offset is not None else None,
        type_id.data_ptr() if type_id is not None else None, float(margin), clearance.data_ptr(),
        nearest.data_ptr() if nearest is not None else None, contacts_out.data_ptr() if contacts_out is not None else None))


# ---- obstacle scenes: per-drone placements of one set (dsim_scenes_create) --------------------------------------------------------
SCENES_MAX_G, SCENES_MAX_SLOTS = 32, 1 << 22


class DeviceScenes:
    """The library's device copy of an :class:`ObstacleScenes` (dsim_scenes_create): the placement table, and the prototype's
    device set, which it makes for ``reach`` and owns unless ``prototype_dev`` hands it one to share."""

    def __init__(self, ctx, scenes: "ObstacleScenes", reach: float = None, prototype_dev: DeviceObstacles = None):
        if prototype_dev is None and reach is None:
            raise ValueError("reach, or a device set of the prototype to share")
        self.ctx, self.scenes, self.K, self.G, self.n_bodies = ctx, scenes, scenes.K, scenes.G, scenes.n_bodies
        self._owns_set = prototype_dev is None
        self.set = scenes.prototype.to_device(ctx, reach) if self._owns_set else prototype_dev
        self.reach = self.set.reach
        self._h = ctypes.c_void_p()
        self.motion = None                 # the SceneMotion attached (set_motion)
        self.twist = None                  # float32 [K, G, 8] on the device: the placements' twists (enable_twist)
        place, count = scenes.place, scenes.count
        nat.check(ctx.lib.dsim_scenes_create(ctx.handle, self.set.handle, place.ctypes.data, count.ctypes.data, self.K, self.G,
                                             ctypes.byref(self._h)))

    @property
    def handle(self):
        return self._h

    def enable_rays(self) -> "DeviceScenes":
        """The prototype's ray grid for the depth camera (DeviceObstacles.enable_rays)."""
        self.set.enable_rays()
        return self

    def set_motion(self, motion: "SceneMotion" = None) -> "DeviceScenes":
        """Attaches a :class:`SceneMotion` made for these scenes (dsim_scenes_motion_set: uploads, synchronises; not inside a graph
        capture); the table stands at its base until :meth:`move`.  None detaches it and restores the base table."""
        if motion is not None and (not isinstance(motion, SceneMotion) or motion.scenes is not self.scenes):
            raise ValueError("set_motion takes a SceneMotion made for the ObstacleScenes of this device object")
        rec = motion.records() if motion is not None else None
        nat.check(self.ctx.lib.dsim_scenes_motion_set(self.ctx.handle, self._h, rec.ctypes.data if rec is not None else None))
        self.motion = motion
        if self.twist is not None:             # (what the old motion moved and the new one leaves alone reads zero again)
            self.twist.zero_()
        return self

    def enable_twist(self) -> "DeviceScenes":
        """Allocates ``twist``, float32 [K, G, 8] of zeros on the context's device: from now on :meth:`move` also writes
        (t'.xyz, 0, w.xyz, 0) of every moving placement into it (dsim_scenes_move_twist); static and unused slots stay zero.
        :func:`witness_scenes_vel` reads it.  Not inside a graph capture."""
        if self.twist is None:
            import torch
            self.twist = torch.zeros((self.K, self.G, 8), dtype=torch.float32, device=self.ctx.device)
        return self

    def move(self, clock, dt: float, t_start: float = 0.0) -> None:
        """dsim_scenes_move on the current stream: the table to scene time t_start + dt * clock.  ``clock``: a device int64 tensor
        [1] read when the kernel runs (a captured call follows it), or None for 0.  Every query of these scenes on the same
        stream is ordered behind it.  After :meth:`enable_twist` it is dsim_scenes_move_twist: the same table, and ``twist``
        at the same scene time."""
        if self.motion is None:
            raise ValueError("move() needs a motion: set_motion(SceneMotion)")
        clk = clock.data_ptr() if clock is not None else None
        if self.twist is not None:
            nat.check(self.ctx.lib.dsim_scenes_move_twist(self.ctx.handle, self.ctx.stream_ptr(), self._h, clk, float(dt),
                                                          float(t_start), self.twist.data_ptr()))
        else:
            nat.check(self.ctx.lib.dsim_scenes_move(self.ctx.handle, self.ctx.stream_ptr(), self._h, clk, float(dt), float(t_start)))

    def read(self) -> np.ndarray:
        """float32 [K, G, 12]: the table as the device holds it now (dsim_scenes_read: waits for the current stream), R row-major
        then t, NaN in unused slots — the layout of ``ObstacleScenes.place``."""
        out = np.empty((self.K, self.G, 12), dtype=np.float32)
        nat.check(self.ctx.lib.dsim_scenes_read(self.ctx.handle, self.ctx.stream_ptr(), self._h, out.ctypes.data))
        return out

    def close(self) -> None:
        if self._h:
            self.ctx.lib.dsim_scenes_destroy(None, self._h)
            self._h = ctypes.c_void_p()
            if self._owns_set:
                self.set.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ObstacleScenes:
    """K scenes of up to G rigid placements of ONE prototype :class:`ObstacleSet`; a drone looks at the scene its ``scene_id``
    names.  ``position`` and ``rpy`` [K, G, 3]: placement g of scene k maps the prototype's frame into the task frame,
    x_task = R(rpy) x_proto + position with R = :func:`_rot` — the convention of ``ObstacleSet.from_urdf(path, position, rpy)``.
    ``count`` [K] ints in 0 .. G (default: G everywhere): the slots of a scene that are used; a scene may be empty, and the
    entries of the other slots are never looked at.  1 <= G <= 32, K G <= 2^22, finite entries in every used slot.

    Every output names a hit triangle by the instance-major body index g n_bodies + body: g the placement's slot in the scene.
    ``place`` is what the device is given: float32 [K, G, 12], R row-major, then the position."""

    def __init__(self, prototype: ObstacleSet, position, rpy, count=None):
        if not isinstance(prototype, ObstacleSet):
            raise TypeError("prototype takes an ObstacleSet")
        pos, rpy = np.asarray(position, dtype=np.float64), np.asarray(rpy, dtype=np.float64)
        if pos.ndim != 3 or pos.shape[2] != 3 or rpy.shape != pos.shape:
            raise ValueError("position and rpy must both be [K, G, 3]")
        K, G = int(pos.shape[0]), int(pos.shape[1])
        if K < 1 or not 1 <= G <= SCENES_MAX_G:
            raise ValueError(f"K >= 1 scenes of 1 <= G <= {SCENES_MAX_G} placements, got K = {K}, G = {G}")
        if K * G > SCENES_MAX_SLOTS:
            raise ValueError(f"K G = {K * G} placements exceed 2^22")
        if count is None:
            cnt = np.full(K, G, dtype=np.int32)
        else:
            cnt = np.asarray(count)
            if cnt.shape != (K,) or not np.issubdtype(cnt.dtype, np.integer) or cnt.min() < 0 or cnt.max() > G:
                raise ValueError(f"count must be [{K}] ints in 0 .. {G}")
            cnt = np.ascontiguousarray(cnt, dtype=np.int32)
        used = np.arange(G)[None, :] < cnt[:, None]
        if not (np.isfinite(pos[used]).all() and np.isfinite(rpy[used]).all()):
            raise ValueError("non-finite placement")
        self.prototype, self.position, self.rpy, self.count = prototype, pos, rpy, cnt
        place = np.full((K, G, 12), np.nan, dtype=np.float32)
        r, p, y = (rpy[used][:, k] for k in range(3))              # _rot for every used slot at once
        cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
        with np.errstate(over="ignore"):
            place[used] = np.stack([cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr,
                                    sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr,
                                    -sp, cp * sr, cp * cr, *pos[used].T], 1)
        if not np.isfinite(place[used]).all():
            raise ValueError("a placement is not finite in float32")
        self.place = np.ascontiguousarray(place)

    @classmethod
    def from_place(cls, prototype: ObstacleSet, place, count=None) -> "ObstacleScenes":
        """Scenes from a table as the device takes and hands back (``place``, ``DeviceScenes.read()``, ``SceneMotion.place``):
        float32 [K, G, 12], R row-major then t, taken verbatim.  ``position`` is t; ``rpy`` is NaN: the rotation is held as a
        matrix only."""
        place = np.ascontiguousarray(place, dtype=np.float32)
        if place.ndim != 3 or place.shape[2] != 12:
            raise ValueError("place must be [K, G, 12]")
        K, G = place.shape[:2]
        proxy = cls(prototype, np.zeros((K, G, 3)), np.zeros((K, G, 3)), count)        # (the checks of K, G and count)
        if not np.isfinite(place[np.arange(G)[None, :] < proxy.count[:, None]]).all():
            raise ValueError("non-finite placement")
        proxy.place = place
        proxy.position, proxy.rpy = place[..., 9:].astype(np.float64), np.full((K, G, 3), np.nan)
        return proxy

    @property
    def K(self) -> int:
        return int(self.place.shape[0])

    @property
    def G(self) -> int:
        return int(self.place.shape[1])

    @property
    def n_bodies(self) -> int:
        return self.prototype.n_bodies

    def flatten(self, k: int) -> ObstacleSet:
        """Scene k's placed triangles as one plain set, body g n_bodies + body (placed with the float32 R and t the device holds).
        An empty scene has no triangles and is a ValueError."""
        k = int(k)
        if not 0 <= k < self.K:
            raise ValueError(f"scene {k} outside [0, {self.K})")
        if self.count[k] == 0:
            raise ValueError(f"scene {k} is empty")
        tri, body = [], []
        proto = self.prototype.triangles.astype(np.float64)
        for g in range(int(self.count[k])):
            R, t = self.place[k, g, :9].astype(np.float64).reshape(3, 3), self.place[k, g, 9:].astype(np.float64)
            tri.append(proto @ R.T + t)
            body.append(self.prototype.body + g * self.n_bodies)
        return ObstacleSet(np.concatenate(tri), np.concatenate(body))

    def to_device(self, ctx, reach: float = None, prototype_dev: DeviceObstacles = None) -> DeviceScenes:
        """The library's device scenes for queries with R_max + margin <= ``reach`` (allocates, uploads, synchronises: not inside
        a graph capture); ``prototype_dev``: a device set of the prototype to share instead of making one."""
        return DeviceScenes(ctx, self, reach, prototype_dev)


class SceneMotion:
    """Per-placement motion of an :class:`ObstacleScenes` (dsim_scene_motion; include/dronesim_amd.h states the law).  With
    (R0, t0) the base pose of placement (k, g) — the float32 ``scenes.place`` — at scene time tau:

        s = sin(omega tau + phase),  t = t0 + velocity tau + amplitude s,  theta = rate tau + swing s,  R = Rot(axis, theta) R0

    a rotation about the placement's own origin.  Every argument broadcasts to [K, G] (``velocity``, ``amplitude``, ``axis``: to
    [K, G, 3]) and is kept as the float32 the library is given; ``axis`` is a unit vector of the task frame (to 1e-5), or zero
    with ``rate == swing == 0``.  A placement whose record is all zeros is static: it equals ``scenes.place`` at every tau, bit
    for bit, and the device never rewrites it.  Entries of unused slots are not looked at.

    Nothing here needs a device: :meth:`pose` and :meth:`place` are the fp64 restatement of what ``DeviceScenes.move`` writes,
    :meth:`twist` and :meth:`point_velocity` of its derivative (``DeviceScenes.enable_twist``)."""

    def __init__(self, scenes: ObstacleScenes, velocity=None, amplitude=None, omega=0.0, phase=0.0, axis=None, rate=0.0, swing=0.0):
        if not isinstance(scenes, ObstacleScenes):
            raise TypeError("SceneMotion takes the ObstacleScenes it moves")
        K, G = scenes.K, scenes.G

        def cast(x, shape, what):
            try:
                return np.ascontiguousarray(np.broadcast_to(np.asarray(0.0 if x is None else x, dtype=np.float32), shape))
            except ValueError:
                raise ValueError(f"{what} does not broadcast to {list(shape)}") from None

        self.scenes = scenes
        self.velocity, self.amplitude = cast(velocity, (K, G, 3), "velocity"), cast(amplitude, (K, G, 3), "amplitude")
        self.axis = cast(axis, (K, G, 3), "axis")
        self.omega, self.phase = cast(omega, (K, G), "omega"), cast(phase, (K, G), "phase")
        self.rate, self.swing = cast(rate, (K, G), "rate"), cast(swing, (K, G), "swing")
        used = self.used = np.arange(G)[None, :] < scenes.count[:, None]
        rec = self.records()
        if not np.isfinite(rec[used]).all():
            raise ValueError("non-finite motion entry in a used slot")
        norm = np.sqrt((self.axis.astype(np.float64) ** 2).sum(-1))
        turning = (self.rate != 0.0) | (self.swing != 0.0)
        bad = used & np.where(norm == 0.0, turning, ~(np.abs(norm - 1.0) <= 1e-5))
        if bad.any():
            raise ValueError("axis must be a unit vector (to 1e-5), or zero with rate == swing == 0")
        # the slots the device rewrites: used, and any entry of the record non-zero
        self.moving = used & (rec != 0.0).any(-1)

    def records(self) -> np.ndarray:
        """float32 [K, G, 16]: the dsim_scene_motion records as dsim_scenes_motion_set takes them (13 floats and the padding)."""
        rec = np.zeros(self.omega.shape + (16,), dtype=np.float32)
        rec[..., 0:3], rec[..., 3:6], rec[..., 6], rec[..., 7] = self.velocity, self.amplitude, self.omega, self.phase
        rec[..., 8:11], rec[..., 11], rec[..., 12] = self.axis, self.rate, self.swing
        return rec

    def pose(self, tau: float):
        """fp64 (R [K, G, 3, 3], t [K, G, 3]) at scene time ``tau``; NaN in unused slots.  For a static slot the base pose."""
        tau = float(tau)
        d = lambda x: x.astype(np.float64)
        place = d(self.scenes.place)
        R0, t0 = place[..., :9].reshape(place.shape[:2] + (3, 3)), place[..., 9:]
        with np.errstate(invalid="ignore", over="ignore"):
            s = np.sin(d(self.omega) * tau + d(self.phase))
            t = t0 + d(self.velocity) * tau + d(self.amplitude) * s[..., None]
            th = d(self.rate) * tau + d(self.swing) * s
            ct, st = np.cos(th)[..., None, None], np.sin(th)[..., None, None]
            k = d(self.axis)[..., :, None]                             # against every column v of R0
            kxv = np.cross(np.broadcast_to(k, R0.shape), R0, axis=-2)
            kv = (k * R0).sum(-2, keepdims=True)
            R = R0 * ct + kxv * st + k * (kv * (1.0 - ct))
        R, t = np.where(self.moving[..., None, None], R, R0), np.where(self.moving[..., None], t, t0)
        return R, t

    def twist(self, tau: float):
        """fp64 (v [K, G, 3], w [K, G, 3]) at scene time ``tau``, the derivative of the law: v = velocity + amplitude omega
        cos(omega tau + phase), w = (rate + swing omega cos(omega tau + phase)) axis — the axis is fixed in the task frame, so w
        is the placement's angular velocity in task axes.  Exact zeros in static slots, NaN in unused ones."""
        tau = float(tau)
        d = lambda x: x.astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            oc = d(self.omega) * np.cos(d(self.omega) * tau + d(self.phase))
            v = d(self.velocity) + d(self.amplitude) * oc[..., None]
            w = (d(self.rate) + d(self.swing) * oc)[..., None] * d(self.axis)
        out = []
        for x in (v, w):
            x = np.where(self.moving[..., None], x, 0.0)
            x[~self.used] = np.nan
            out.append(x)
        return out[0], out[1]

    def point_velocity(self, tau: float, x) -> np.ndarray:
        """fp64 [K, G, 3]: the velocity at scene time ``tau`` of the material point of each placement that stands at the
        task-frame position ``x`` ([K, G, 3], or what broadcasts to it): t' + w x (x - t(tau)).  NaN in unused slots."""
        v, w = self.twist(tau)
        _, t = self.pose(tau)
        r = np.broadcast_to(np.asarray(x, dtype=np.float64), t.shape) - t
        return v + np.cross(w, r)

    def place(self, tau: float) -> np.ndarray:
        """float32 [K, G, 12] at scene time ``tau``, R row-major then t: what ``DeviceScenes.read()`` returns after a move to
        ``tau`` (to the rounding of one float), NaN in unused slots.  Static slots are ``scenes.place``'s, bit for bit."""
        R, t = self.pose(tau)
        with np.errstate(over="ignore"):
            out = np.concatenate([R.reshape(R.shape[:2] + (9,)), t], -1).astype(np.float32)
        return np.ascontiguousarray(np.where(self.moving[..., None], out, self.scenes.place))

    def snapshot(self, tau: float) -> ObstacleScenes:
        """A plain static :class:`ObstacleScenes` whose ``place`` is :meth:`place` at ``tau`` (same prototype and counts; its
        ``position`` is t(tau), its ``rpy`` NaN: the rotation is held as a matrix only)."""
        return ObstacleScenes.from_place(self.scenes.prototype, self.place(tau), self.scenes.count)


def query_scenes(ctx, state, dev_scenes: DeviceScenes, scene_id, margin: float, clearance, nearest, offset=None, type_id=None,
                 contacts_out=None) -> None:
    """dsim_obstacle_clearance_scenes on the current stream into the given tensors ([n_pad] float32 / int32); ``scene_id``: int32
    device tensor [n_pad] in storage order, an id outside [0, K) meaning no obstacles."""
    if scene_id is None:
        raise ValueError("scene_id is required")
    nat.check(ctx.lib.dsim_obstacle_clearance_scenes(
        ctx.handle, ctx.stream_ptr(), state.n, state.view(), dev_scenes.handle, scene_id.data_ptr(),
        offset.data_ptr() if offset is not None else None, type_id.data_ptr() if type_id is not None else None, float(margin),
        clearance.data_ptr(), nearest.data_ptr() if nearest is not None else None,
        contacts_out.data_ptr() if contacts_out is not None else None))


# ---- the obstacle witness (dsim_obstacle_witness) -----------------------------------------------------------------------------------
def _witness_args(margin, clearance, nearest, rel, triangle, offset, type_id, contacts_out, body_frame) -> "nat.WitnessArgs":
    if rel is None:
        raise ValueError("rel ([3, n_pad] float32) is required")
    ptr = lambda t: t.data_ptr() if t is not None else None
    return nat.WitnessArgs(ptr(offset), ptr(type_id), float(margin), nat.WITNESS_BODY_FRAME if body_frame else 0, clearance.data_ptr(),
                           ptr(nearest), rel.data_ptr(), ptr(triangle), ptr(contacts_out))


def witness(ctx, state, dev: DeviceObstacles, margin: float, clearance, nearest, rel, triangle=None, offset=None, type_id=None,
            contacts_out=None, body_frame: bool = False) -> None:
    """dsim_obstacle_witness on the current stream: what :func:`query` writes into ``clearance`` / ``nearest`` ([n_pad] float32 /
    int32) and, into ``rel`` ([3, n_pad] float32), the vector from every drone's query point to the closest point of the set —
    world axes, or the drone's body axes with ``body_frame`` — and into ``triangle`` ([n_pad] int32, may be None) the triangle
    that holds it.  Zeros and -1 where ``nearest`` is -1.  The unit direction is rel / (clearance + R_i): not normalised here."""
    a = _witness_args(margin, clearance, nearest, rel, triangle, offset, type_id, contacts_out, body_frame)
    nat.check(ctx.lib.dsim_obstacle_witness(ctx.handle, ctx.stream_ptr(), state.n, state.view(), dev.handle, ctypes.byref(a)))


def witness_scenes(ctx, state, dev_scenes: DeviceScenes, scene_id, margin: float, clearance, nearest, rel, triangle=None, offset=None,
                   type_id=None, contacts_out=None, body_frame: bool = False) -> None:
    """dsim_obstacle_witness_scenes on the current stream: :func:`witness` against the placements of each drone's scene
    (``scene_id`` as in :func:`query_scenes`); ``triangle`` is instance-major, g n_tri + t, as ``nearest`` is g n_bodies + body."""
    if scene_id is None:
        raise ValueError("scene_id is required")
    a = _witness_args(margin, clearance, nearest, rel, triangle, offset, type_id, contacts_out, body_frame)
    nat.check(ctx.lib.dsim_obstacle_witness_scenes(ctx.handle, ctx.stream_ptr(), state.n, state.view(), dev_scenes.handle,
                                                   scene_id.data_ptr(), ctypes.byref(a)))


def witness_scenes_vel(ctx, state, dev_scenes: DeviceScenes, scene_id, margin: float, clearance, nearest, rel, vel, triangle=None,
                       offset=None, type_id=None, contacts_out=None, body_frame: bool = False) -> None:
    """dsim_obstacle_witness_scenes_vel on the current stream: what :func:`witness_scenes` writes, bit for bit, and into ``vel``
    ([3, n_pad] float32) the velocity of every drone's closest obstacle point as a material point of the placement that holds
    it, t' + w x r from ``dev_scenes.twist`` as the last :meth:`DeviceScenes.move` left it — world axes, or the drone's body axes
    with ``body_frame``; the obstacle's own velocity, not the relative one.  Zeros where ``nearest`` is -1 and on a static
    placement."""
    if scene_id is None:
        raise ValueError("scene_id is required")
    if vel is None:
        raise ValueError("vel ([3, n_pad] float32) is required")
    if dev_scenes.twist is None:
        raise ValueError("witness_scenes_vel needs the scenes' twist table: DeviceScenes.enable_twist()")
    a = _witness_args(margin, clearance, nearest, rel, triangle, offset, type_id, contacts_out, body_frame)
    nat.check(ctx.lib.dsim_obstacle_witness_scenes_vel(ctx.handle, ctx.stream_ptr(), state.n, state.view(), dev_scenes.handle,
                                                       scene_id.data_ptr(), ctypes.byref(a), dev_scenes.twist.data_ptr(),
                                                       vel.data_ptr()))


class ObstacleWitnesses(typing.NamedTuple):
    """What :func:`witnesses` / :func:`witnesses_scenes` answer, slot-major: ``clearance`` and ``body`` [m, N], ``rel`` [m, 3, N],
    ``vel`` [m, 3, N] or None, ``count`` [N] — the slots filled, min(bodies within the margin, m): ``count == m`` may hide
    further bodies."""
    clearance: object
    body: object
    rel: object
    vel: object
    count: object


def _witnesses_args(m, margin, clearance, body, rel, triangle, count, offset, type_id, contacts_out, body_frame, twist=None,
                    vel=None) -> "nat.WitnessesArgs":
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 1 <= int(m) <= nat.WITNESSES_MAX:
        raise ValueError(f"m must be an int in 1..{nat.WITNESSES_MAX}, got {m!r}")
    if clearance is None or body is None or rel is None:
        raise ValueError("clearance, body ([m, n_pad]) and rel ([m, 3, n_pad] float32) are required")
    ptr = lambda t: t.data_ptr() if t is not None else None
    return nat.WitnessesArgs(ptr(offset), ptr(type_id), float(margin), int(m), nat.WITNESS_BODY_FRAME if body_frame else 0,
                             clearance.data_ptr(), body.data_ptr(), rel.data_ptr(), ptr(triangle), ptr(count), ptr(contacts_out),
                             ptr(twist), ptr(vel))


def witnesses(ctx, state, dev: DeviceObstacles, margin: float, m: int, clearance, body, rel, triangle=None, count=None, offset=None,
              type_id=None, contacts_out=None, body_frame: bool = False) -> None:
    """dsim_obstacle_witnesses on the current stream: per drone the ``m`` (1..8) closest BODIES of the set within the margin,
    ascending in distance, slot-major: ``clearance`` [m, n_pad] float32 (``margin`` in an unfilled slot), ``body`` [m, n_pad]
    int32 (-1), ``rel`` [m, 3, n_pad] float32, the vector from the query point to the closest point of that body — world axes, or
    the drone's body axes with ``body_frame`` — exact zeros unfilled; ``triangle`` [m, n_pad] int32 and ``count`` [n_pad] int32
    may be None.  Slot 0 is :func:`witness`, bit for bit; ties keep what the walk met first."""
    a = _witnesses_args(m, margin, clearance, body, rel, triangle, count, offset, type_id, contacts_out, body_frame)
    nat.check(ctx.lib.dsim_obstacle_witnesses(ctx.handle, ctx.stream_ptr(), state.n, state.view(), dev.handle, ctypes.byref(a)))


def witnesses_scenes(ctx, state, dev_scenes: DeviceScenes, scene_id, margin: float, m: int, clearance, body, rel, triangle=None,
                     count=None, offset=None, type_id=None, contacts_out=None, body_frame: bool = False, vel=None) -> None:
    """dsim_obstacle_witnesses_scenes on the current stream: :func:`witnesses` over the instance-major bodies g n_bodies + body of
    the placements of each drone's scene (``scene_id`` as in :func:`query_scenes`; ``triangle`` is g n_tri + t).  With ``vel``
    ([m, 3, n_pad] float32) the velocity of every witness as a material point of its own placement, from ``dev_scenes.twist`` as
    the last :meth:`DeviceScenes.move` left it: what :func:`witness_scenes_vel` gives for the one, zeros unfilled and static."""
    if scene_id is None:
        raise ValueError("scene_id is required")
    if vel is not None and dev_scenes.twist is None:
        raise ValueError("vel needs the scenes' twist table: DeviceScenes.enable_twist()")
    a = _witnesses_args(m, margin, clearance, body, rel, triangle, count, offset, type_id, contacts_out, body_frame,
                        dev_scenes.twist if vel is not None else None, vel)
    nat.check(ctx.lib.dsim_obstacle_witnesses_scenes(ctx.handle, ctx.stream_ptr(), state.n, state.view(), dev_scenes.handle,
                                                     scene_id.data_ptr(), ctypes.byref(a)))


def point_query(ctx, state, dev, scene_id, margin: float, clearance, nearest, rel=None, offset=None, type_id=None, contacts_out=None,
                body_frame: bool = False, vel=None, m=None, count=None) -> None:
    """The point query of a device world, whichever it is: :func:`query` on a :class:`DeviceObstacles`, :func:`query_scenes` on a
    :class:`DeviceScenes` (``scene_id`` is theirs and is not looked at otherwise); with ``rel`` the witness query in its place
    (:func:`witness` / :func:`witness_scenes`: the same answers and the vector beside them, no ``triangle``); with ``vel`` too,
    on scenes, :func:`witness_scenes_vel`.  With ``m`` the witnesses query in the witness's place (:func:`witnesses` /
    :func:`witnesses_scenes`): ``clearance`` / ``nearest`` [m, n_pad], ``rel`` / ``vel`` [m, 3, n_pad], ``count`` [n_pad]."""
    ids = (scene_id,) if isinstance(dev, DeviceScenes) else ()
    if m is not None:
        if rel is None or (vel is not None and not ids):
            raise ValueError("m needs rel, and vel a DeviceScenes")
        if ids:
            witnesses_scenes(ctx, state, dev, scene_id, margin, m, clearance, nearest, rel, None, count, offset, type_id, contacts_out,
                             body_frame=body_frame, vel=vel)
        else:
            witnesses(ctx, state, dev, margin, m, clearance, nearest, rel, None, count, offset, type_id, contacts_out,
                      body_frame=body_frame)
        return
    if vel is not None:
        if not ids or rel is None:
            raise ValueError("vel needs a DeviceScenes and rel")
        witness_scenes_vel(ctx, state, dev, scene_id, margin, clearance, nearest, rel, vel, None, offset, type_id, contacts_out,
                           body_frame=body_frame)
    elif rel is None:
        (query_scenes if ids else query)(ctx, state, dev, *ids, margin, clearance, nearest, offset, type_id, contacts_out)
    else:
        (witness_scenes if ids else witness)(ctx, state, dev, *ids, margin, clearance, nearest, rel, None, offset, type_id,
                                             contacts_out, body_frame=body_frame)


def scene_ids_tensor(scene_id, n: int, n_pad: int, device, order=None):
    """``scene_id`` [n] ints in the caller's numbering as the int32 device tensor [n_pad] in storage order the calls take (-1, no
    obstacles, behind n)."""
    ids = np.asarray(scene_id)
    if ids.shape != (n,) or not np.issubdtype(ids.dtype, np.integer):
        raise ValueError(f"scene ids must be [{n}] ints")
    ids = np.clip(ids.astype(np.int64), -1, 2 ** 31 - 1)
    if order is not None:
        ids = order.to_storage_np(ids)
    import torch
    t = torch.full((n_pad,), -1, dtype=torch.int32)
    t[:n] = torch.from_numpy(np.ascontiguousarray(ids.astype(np.int32)))
    return t.to(device)


# ---- the swept watch (dsim_obstacle_sweep) ------------------------------------------------------------------------------------------
def sweep_reach(types, margin: float, sag: float, travel: float) -> float:
    """The ``reach`` of a set for swept queries of ``margin`` and ``sag`` over these drone types whose chords are up to ``travel``
    metres long per lookup: fp32(R_max + sag + margin + travel / 2), a thousandth more as in :func:`watch_reach`.  A longer chord
    is cut into pieces of that length (up to 32 of them), so ``travel`` decides speed, never results; it must be positive: the
    library refuses a set whose reach leaves less than a 1024th of itself for the pieces."""
    r_max = max(float(np.float32(t.collision_sphere)) for t in types)
    s = r_max + float(np.float32(sag)) + float(np.float32(margin)) + 0.5 * float(travel)
    return float(np.float32(s * (1.0 + 2.0 ** -10)))


def corridor_reach(types, margin: float, sag: float, piece: float) -> float:
    """The ``reach`` of a set for corridor queries (dsim_corridor_clearance, corridor.Corridor) of ``margin`` and ``sag`` over these
    drone types whose segments are cut into pieces of ``piece`` metres: :func:`sweep_reach`, the same pieces under the name the
    query's callers look for.  A segment of up to 32 pieces is served, so ``piece`` decides speed and the longest segment."""
    return sweep_reach(types, margin, sag, piece)


def sweep_sag(a_max: float, T: float) -> float:
    """a_max T^2 / 8: how far a path whose acceleration never exceeds ``a_max`` [m/s^2] can leave the chord between its positions
    a time ``T`` [s] apart (x(t) minus the chord vanishes at both ends and has a second derivative bounded by a_max: the
    parabola a_max t (T - t) / 2 bounds it, with its maximum in the middle).  With ``sag`` at least this, every state between the
    two samples lies in the volume the swept query tests."""
    return float(a_max) * float(T) ** 2 / 8.0


def sweep(ctx, state, dev: DeviceObstacles, margin: float, sag: float, prev, clearance, nearest, offset=None, type_id=None,
          contacts_out=None, unswept_out=None, keep_prev: bool = False) -> None:
    """dsim_obstacle_sweep on the current stream: the chord from ``prev`` ([3, n_pad] float32, world frame, updated unless
    ``keep_prev``) to the current positions, into the given tensors ([n_pad] float32 / int32)."""
    ptr = lambda t: t.data_ptr() if t is not None else None
    a = nat.SweepArgs(ptr(offset), ptr(type_id), float(margin), float(sag), prev.data_ptr(),
                      nat.SWEEP_KEEP_PREV if keep_prev else 0, clearance.data_ptr(), ptr(nearest), ptr(contacts_out), ptr(unswept_out))
    nat.check(ctx.lib.dsim_obstacle_sweep(ctx.handle, ctx.stream_ptr(), state.n, state.view(), dev.handle, ctypes.byref(a)))


def prime(ctx, state, dev: DeviceObstacles, prev) -> None:
    """``prev`` := the current positions (DSIM_SWEEP_PRIME): the next :func:`sweep` starts its chords here."""
    a = nat.SweepArgs(None, None, 0.0, 0.0, prev.data_ptr(), nat.SWEEP_PRIME, None, None, None, None)
    nat.check(ctx.lib.dsim_obstacle_sweep(ctx.handle, ctx.stream_ptr(), state.n, state.view(), dev.handle, ctypes.byref(a)))


# ---- the gate passage watch (dsim_gate_passage) ----------------------------------------------------------------------------------------
class Aperture:
    """One planar opening in the frame of an :class:`ObstacleScenes`' prototype: what a gate is flown THROUGH.  ``center`` [3];
    ``normal`` [3], the forward direction, and ``u`` [3], an in-plane axis — both of unit length to 1e-5 and perpendicular to
    1e-5 (they are used as given, never normalised: v = normal x u); ``half`` (a, b) > 0, the half-extents along u and v;
    ``shape`` "rect" or "ellipse" (the ellipse inscribed in the rectangle); ``outer`` (a_out >= a, b_out >= b) or None: a
    rectangle around the opening — a forward crossing inside it but outside the aperture is a miss, the vehicle went over or
    round the opening."""

    SHAPES = {"rect": nat.APERTURE_RECT, "ellipse": nat.APERTURE_ELLIPSE}

    def __init__(self, center, normal, u, half, shape="rect", outer=None):
        vec = lambda x, k, what: self._vec(x, k, what)
        self.center, self.normal, self.u = vec(center, 3, "center"), vec(normal, 3, "normal"), vec(u, 3, "u")
        self.half = vec(half, 2, "half")
        self.outer = vec(outer, 2, "outer") if outer is not None else None
        if shape not in self.SHAPES:
            raise ValueError(f"shape must be 'rect' or 'ellipse', got {shape!r}")
        self.shape = shape
        n, uu = self.normal.astype(np.float64), self.u.astype(np.float64)
        if abs(np.linalg.norm(n) - 1.0) > 1e-5 or abs(np.linalg.norm(uu) - 1.0) > 1e-5:
            raise ValueError("normal and u must be of unit length (to 1e-5)")
        if abs(float(n @ uu)) > 1e-5:
            raise ValueError("u must be perpendicular to normal (to 1e-5)")
        if not (self.half > 0).all():
            raise ValueError("half-extents must be positive")
        if self.outer is not None and not (self.outer >= self.half).all():
            raise ValueError("the outer rectangle must not be smaller than the aperture")

    @staticmethod
    def _vec(x, k, what):
        v = np.asarray(x, dtype=np.float32).reshape(-1)
        if v.shape != (k,) or not np.isfinite(v).all():
            raise ValueError(f"{what} must be {k} finite numbers")
        return v

    @property
    def v(self) -> np.ndarray:
        """normal x u, fp64 on the float32 numbers the device is given."""
        return np.cross(self.normal.astype(np.float64), self.u.astype(np.float64))

    def to_c(self) -> "nat.ApertureC":
        c = nat.ApertureC()
        c.center[:], c.normal[:], c.u[:], c.half[:] = self.center.tolist(), self.normal.tolist(), self.u.tolist(), self.half.tolist()
        c.outer[:] = self.outer.tolist() if self.outer is not None else [0.0, 0.0]
        c.shape = self.SHAPES[self.shape]
        return c


def gate_passage(ctx, state, dev_scenes: DeviceScenes, scene_id, aperture: Aperture, travel: float, prev, due, laps=None, clock=None,
                 pass_time=None, fwd=None, back=None, miss=None, offset=None, passes_out=None, wrong_way_out=None,
                 out_of_order_out=None, misses_out=None, unswept_out=None, wrap: bool = False, keep_prev: bool = False) -> None:
    """dsim_gate_passage on the current stream: the chord from ``prev`` ([3, n_pad] float32, world frame, updated unless
    ``keep_prev``) to the current positions against the aperture at every placement of each drone's scene.  ``due`` ([n_pad]
    int32) and, with ``wrap``, ``laps`` ([n_pad] int32) are the course state, in-out; ``pass_time`` ([G, n_pad] float64) receives
    ``clock`` (int64 [1] device counter, the caller advances it) + tau for every gate passed; ``fwd`` / ``back`` / ``miss``
    ([n_pad] int32, one bit per slot) the events of this query; the ``*_out`` are int64 [1] device counters.  All but ``prev``
    and ``due`` may be None."""
    if not isinstance(aperture, Aperture):
        raise TypeError("aperture takes an obstacles.Aperture")
    if scene_id is None:
        raise ValueError("scene_id is required")
    ptr = lambda t: t.data_ptr() if t is not None else None
    flags = (nat.SWEEP_KEEP_PREV if keep_prev else 0) | (nat.GATE_WRAP if wrap else 0)
    a = nat.GateArgs(aperture.to_c(), float(travel), flags, ptr(offset), prev.data_ptr(), due.data_ptr(), ptr(laps), ptr(clock),
                     ptr(pass_time), ptr(fwd), ptr(back), ptr(miss), ptr(passes_out), ptr(wrong_way_out), ptr(out_of_order_out),
                     ptr(misses_out), ptr(unswept_out))
    nat.check(ctx.lib.dsim_gate_passage(ctx.handle, ctx.stream_ptr(), state.n, state.view(), dev_scenes.handle, scene_id.data_ptr(),
                                        ctypes.byref(a)))


def gate_prime(ctx, state, prev) -> None:
    """``prev`` := the current positions (DSIM_SWEEP_PRIME): the next :func:`gate_passage` starts its chords here."""
    a = nat.GateArgs()
    a.prev, a.flags = prev.data_ptr(), nat.SWEEP_PRIME
    nat.check(ctx.lib.dsim_gate_passage(ctx.handle, ctx.stream_ptr(), state.n, state.view(), None, None, ctypes.byref(a)))
