"""The range scanner's reference (numpy only, so the CPU tests use it without a device): an fp64 brute-force caster over ALL
triangles and ALL spheres (camera_ref.cast, camera_drones_ref.cast_spheres; no grid, no cell walk), a float32 restatement of the
kernel's own arithmetic from which the tests' tolerance is derived, and the inputs the GPU cases and the CPU checks of their
conditions share.  tests/README_scan.md.

The ray (include/dronesim_amd.h): origin e = p_i - offset_i, direction d = R(quat_i) beam_b with R from the unnormalised quaternion
(s = 2 / |q|^2), not normalised; the drones' spheres are met from the stored position p_i with the same d."""
import functools

import numpy as np

from tests import camera_drones_ref as dr
from tests import camera_ref as cr
from tests import scenes_ref as sr

SEG_GROUND = -2


def R64(q):
    """R(q) in fp64 from the (unnormalised) quaternion xyzw."""
    x, y, z, w = (float(v) for v in q)
    s = 2.0 / (x * x + y * y + z * z + w * w)
    return np.array([[1.0 - s * (y * y + z * z), s * (x * y - w * z), s * (x * z + w * y)],
                     [s * (x * y + w * z), 1.0 - s * (x * x + z * z), s * (y * z - w * x)],
                     [s * (x * z - w * y), s * (y * z + w * x), 1.0 - s * (x * x + y * y)]])


def fan(*a, **k):
    from dronesim_amd.scanner import RangeScanner
    return RangeScanner.fan(*a, **k)


# ---- fp64 brute force ----------------------------------------------------------------------------------------------------------------
def scan_brute(stored, beams, t_min, t_max, tri=None, body=None, scenes=None, scene_id=None, ground=False, offsets=None,
               radius=None, drone_range=None, label=None):
    """What dsim_range_scan is specified to give, in fp64 on the float32 inputs, per drone: stored [n, 7] (pos + quat xyzw, the
    caller's numbering), beams [B, 3], tri / body an unplaced set or scenes / scene_id a placed one (neither: no triangles),
    offsets [n, 3] or None, radius [n] with drones as targets (None: none; label as camera_drones_ref).  Returns a dict of [B, n]
    arrays: t (inf: no hit), hit (body — instance-major on scenes —, -1, -2 the plane, -3 - label[j]), ambiguous (the triangle mask
    joined with the sphere mask), ndot, is_drone."""
    stored = np.asarray(stored, np.float32)
    beams64 = np.asarray(beams, np.float32).astype(np.float64)
    n, B = stored.shape[0], beams64.shape[0]
    near, far = float(np.float32(t_min)), float(np.float32(t_max))
    rng = far if drone_range is None else float(np.float32(drone_range))
    out = {"t": np.full((B, n), np.inf), "hit": np.full((B, n), -1, dtype=np.int64), "ambiguous": np.zeros((B, n), bool),
           "ndot": np.ones((B, n)), "is_drone": np.zeros((B, n), bool)}
    lab = None if radius is None else (np.arange(n) if label is None else np.asarray(label))
    if tri is not None:
        tri = np.asarray(tri, np.float32)
    placed = {}
    for i in range(n):
        p, q = stored[i, :3].astype(np.float64), stored[i, 3:].astype(np.float64)
        e = p - (0.0 if offsets is None else np.asarray(offsets[i], np.float32).astype(np.float64))
        if not (np.isfinite(p).all() and np.isfinite(e).all() and np.isfinite(q).all() and (q @ q) > 0.0):
            continue                                           # an undefined pose: every beam misses
        d = beams64 @ R64(q).T
        t_i, b_i = dr._NO_TRI, 0
        if tri is not None:
            t_i, b_i = tri, body
        elif scenes is not None:
            k = int(scene_id[i])
            if 0 <= k < scenes.K and scenes.count[k] > 0:
                if k not in placed:
                    placed[k] = sr.placed_triangles(scenes, k)
                t_i, b_i = placed[k]
        base = cr.cast(t_i, b_i, e, d, near, far, ground)
        t, hit, amb, ndot, isd = base["t"], base["seg"], base["ambiguous"], base["ndot"], np.zeros(B, bool)
        if radius is not None:
            sph = dr.cast_spheres(stored[:, :3], radius, p, d, near, min(far, rng), own=i)
            isd = sph["t"] < t
            t = np.where(isd, sph["t"], t)
            hit = np.where(isd, dr.seg_drone(lab[np.maximum(sph["idx"], 0)]), hit)
            amb = amb | dr.sphere_mask(sph, t, near, far, rng)
            ndot = np.where(isd, sph["ndot"], ndot)
        out["t"][:, i], out["hit"][:, i], out["ambiguous"][:, i], out["ndot"][:, i], out["is_drone"][:, i] = t, hit, amb, ndot, isd
    return out


# ---- the kernel's arithmetic in float32 ----------------------------------------------------------------------------------------------
def _rays32(stored, beams, offsets):
    """(e [n, 3], w [n, 3], d [n, B, 3]) in float32, operation by operation as the kernel forms them."""
    F = np.float32
    st = np.asarray(stored, F)
    w = st[:, :3]
    e = w if offsets is None else w - np.asarray(offsets, F)
    x, y, z, qw = (st[:, 3 + k] for k in range(4))
    with np.errstate(all="ignore"):
        s2 = F(2.0) / (x * x + y * y + z * z + qw * qw)
        xs, ys, zs = x * s2, y * s2, z * s2
        r = [[F(1.0) - (y * ys + z * zs), x * ys - qw * zs, x * zs + qw * ys],
             [x * ys + qw * zs, F(1.0) - (x * xs + z * zs), y * zs - qw * xs],
             [x * zs - qw * ys, y * zs + qw * xs, F(1.0) - (x * xs + y * ys)]]
        b = np.asarray(beams, F)
        d = np.stack([r[k][0][:, None] * b[None, :, 0] + r[k][1][:, None] * b[None, :, 1] + r[k][2][:, None] * b[None, :, 2]
                      for k in range(3)], -1)
    assert d.dtype == np.float32 and e.dtype == np.float32
    return e, w, d


def _tri32(rec, e, d, near, far):
    """Nearest Moeller-Trumbore t [n, B] of rays (e [n, 3], d [n, B, 3]) over the records, camera_ref.restated_image's test."""
    F = np.float32
    a, ab, ac = rec
    ax, ay, az = (a[:, k][None, None, :] for k in range(3))
    abx, aby, abz = (ab[:, k][None, None, :] for k in range(3))
    acx, acy, acz = (ac[:, k][None, None, :] for k in range(3))
    dx, dy, dz = (d[..., k][..., None] for k in range(3))
    ex, ey, ez = (e[:, k][:, None, None] for k in range(3))
    px, py, pz = dy * acz - dz * acy, dz * acx - dx * acz, dx * acy - dy * acx
    det = abx * px + aby * py + abz * pz
    tx, ty, tz = ex - ax, ey - ay, ez - az
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        idet = F(1.0) / det
        u = (tx * px + ty * py + tz * pz) * idet
        qx, qy, qz = ty * abz - tz * aby, tz * abx - tx * abz, tx * aby - ty * abx
        v = (dx * qx + dy * qy + dz * qz) * idet
        t = (acx * qx + acy * qy + acz * qz) * idet
        hit = (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= near) & (t <= far)
    assert t.dtype == np.float32
    return np.where(hit, t, F(np.inf)).min(-1)


def _records(tri):
    tri = np.asarray(tri, np.float32).reshape(-1, 3, 3)
    return (tri[:, 0], (tri[:, 1].astype(np.float64) - tri[:, 0]).astype(np.float32),
            (tri[:, 2].astype(np.float64) - tri[:, 0]).astype(np.float32))


def restated_scan(stored, beams, t_min, t_max, tri=None, scenes=None, scene_id=None, ground=False, offsets=None, radius=None,
                  drone_range=None, chunk=64):
    """t [B, n] (inf: no hit) as the kernel computes it, operation by operation in float32 (numpy rounds every product and sum
    where the device contracts some into fused multiply-adds and takes 1-ulp reciprocals and square roots), over all triangles
    and all spheres without a grid: the quaternion to R, d = R beam, the plane, the triangle test of camera_ref.restated_image
    (on scenes by the placed route of scenes_ref.restated_placed_image: subtract, rotate), the sphere form of
    camera_drones_ref.restated_spheres."""
    F = np.float32
    e, w, d = _rays32(stored, beams, offsets)
    n, B = d.shape[:2]
    near, far = F(t_min), F(t_max)
    best = np.full((n, B), np.inf, dtype=F)
    with np.errstate(all="ignore"):
        if ground:
            tg = -e[:, 2][:, None] / d[..., 2]
            best = np.where((tg >= near) & (tg <= far), tg, best)
        if tri is not None:
            rec = _records(tri)
            for k0 in range(0, n, chunk):
                best[k0:k0 + chunk] = np.minimum(best[k0:k0 + chunk], _tri32(rec, e[k0:k0 + chunk], d[k0:k0 + chunk], near, far))
        if scenes is not None:
            rec = _records(scenes.prototype.triangles)
            sid = np.asarray(scene_id, np.int64)
            for k in range(scenes.K):
                m = np.nonzero(sid == k)[0]
                for g in range(int(scenes.count[k])):
                    P = scenes.place[k, g]
                    c = [P[[j, 3 + j, 6 + j]] for j in range(3)]                # column j of R
                    for k0 in range(0, len(m), chunk):
                        mm = m[k0:k0 + chunk]
                        tx, ty, tz = e[mm, 0] - P[9], e[mm, 1] - P[10], e[mm, 2] - P[11]
                        le = np.stack([cj[0] * tx + cj[1] * ty + cj[2] * tz for cj in c], -1)
                        ld = np.stack([cj[0] * d[mm, :, 0] + cj[1] * d[mm, :, 1] + cj[2] * d[mm, :, 2] for cj in c], -1)
                        assert le.dtype == np.float32 and ld.dtype == np.float32
                        best[mm] = np.minimum(best[mm], _tri32(rec, le, ld, near, far))
        if radius is not None:
            R = np.asarray(radius, F)
            tmax = min(far, F(t_max if drone_range is None else drone_range))
            dx, dy, dz = (d[..., k][..., None] for k in range(3))
            inv_a = F(1.0) / (dx * dx + dy * dy + dz * dz)
            mx, my, mz = (w[None, None, :, k] - w[:, None, None, k] for k in range(3))          # [n, 1, n]: centre j - origin i
            tc = (mx * dx + my * dy + mz * dz) * inv_a
            qx, qy, qz = mx - tc * dx, my - tc * dy, mz - tc * dz
            disc = (R * R)[None, None, :] - (qx * qx + qy * qy + qz * qz)
            h = np.sqrt(np.maximum(disc, F(0.0)) * inv_a)
            t0, t1 = tc - h, tc + h
            t = np.where(t0 >= near, t0, t1)
            hit = (R > 0)[None, None, :] & (disc >= 0) & (t >= near) & (t <= tmax) & ~np.eye(n, dtype=bool)[:, None, :]
            assert t.dtype == np.float32
            best = np.minimum(best, np.where(hit, t, F(np.inf)).min(-1))
    return best.T.astype(np.float64)


def t_error(t, ref):
    """camera_ref.t_error on [B, n] arrays."""
    return cr.t_error(np.asarray(t, np.float64), ref)


# the float32 restatement's worst t_error against scan_brute over the inputs of the GPU cases (RESTATED_INPUTS): measured by
# tests/test_scan_cpu.py::test_restated_error_is_what_is_recorded; the kernel is granted 4 x this, the project's standing margin
# for FMA contraction and 1-ulp reciprocals
SCAN_RESTATED_WORST = 1.30e-6
SCAN_TOL = 4.0 * SCAN_RESTATED_WORST
MASK_CAP = 0.01


# ---- the inputs of the GPU cases -----------------------------------------------------------------------------------------------------
T_MIN, T_MAX = 0.05, 8.0


def draw_fleet(seed, n, lo=(-1.0, -2.5, 0.2), hi=(5.0, 2.5, 2.5), tilt=0.5):
    """stored [n, 7] float32: positions uniform in the box, on multiples of 2^-10 m (p + offset is then exact in float32 for
    offsets that are multiples of 1/4 m); rpy uniform in +-tilt, +-tilt, +-pi."""
    rng = np.random.default_rng(seed)
    pos = np.round(rng.uniform(lo, hi, (n, 3)) * 1024.0) / 1024.0
    rpy = rng.uniform([-tilt, -tilt, -np.pi], [tilt, tilt, np.pi], (n, 3))
    st = np.zeros((n, 7), dtype=np.float32)
    st[:, :3] = pos
    st[:, 3:] = np.stack([cr.quat_from_rpy(*e) for e in rpy])
    return st


def quarter_offsets(seed, n):
    """[n, 3] offsets, multiples of 1/4 m up to 8 m (camera_ref.fleet_offsets)."""
    return np.random.default_rng(seed).integers(-32, 33, (n, 3)).astype(np.float64) * 0.25


def with_offsets(st, off):
    """The fleet stored at p + offset: exact in float32, so that the stored value minus the offset is p again."""
    out = st.copy()
    out[:, :3] = (st[:, :3].astype(np.float64) + off).astype(np.float32)
    assert np.array_equal(out[:, :3] - off.astype(np.float32), st[:, :3])
    return out


@functools.lru_cache(maxsize=None)
def case_main(subdiv):
    """Cases 1 and 2: scene(0) with n = 500, scene(2) with n = 192; fan(16, up, down), B = 18.  -> dict(st, beams, sc, ref: (without
    ground, with ground))."""
    n = 500 if subdiv == 0 else 192
    st, beams, sc = draw_fleet(101 + subdiv, n), fan(16, up=True, down=True), cr.scene(subdiv)
    ref = tuple(scan_brute(st, beams, T_MIN, T_MAX, sc.triangles, sc.body, ground=g) for g in (False, True))
    return {"st": st, "beams": beams, "sc": sc, "ref": ref}


AXIS_BEAMS = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float32)
# the edge table: every eye of camera_ref.edge_eyes with the four axis quaternions of EDGE_QUATS and the six axis beams.  Left out
# BY NAME: combinations whose mask exceeds the cap (none is known; tests/test_scan_cpu.py asserts the cap for every one kept)
EDGE_LEFT_OUT = ()


@functools.lru_cache(maxsize=None)
def case_edges(subdiv=0):
    """Case 3: origins on cell planes, on the box's faces, outside a slab; components of d exactly 0.  -> dict(st [20, 7], names,
    beams, sc, ref (with ground off))."""
    sc = cr.scene(subdiv)
    eyes = dict(cr.edge_eyes(sc))
    # three more of the scanner's own, aimed at the rotated box (body 1, about (3.5, 0.6, 0.8)) so that axis beams along cell
    # planes also HIT: on the grid's low x face with y and z on the cell planes nearest the box's centre; on the grid's top above
    # it; half a metre beyond the high x face (outside the slab, looking back in)
    F = np.float32
    g = sc.ray_grid()[0]
    o, hi, cell = np.array(list(g.origin), F), np.array(list(g.hi), F), F(g.cell)
    face = lambda k, v: F(o[k] + F(int(round((v - float(o[k])) / float(cell)))) * cell)
    eyes["aim_x"] = np.array([o[0], face(1, 0.6), face(2, 0.8)], F)
    eyes["aim_z"] = np.array([face(0, 3.5), face(1, 0.6), hi[2]], F)
    eyes["aim_back"] = np.array([F(hi[0] + F(0.5)), face(1, 0.6), face(2, 0.8)], F)
    names = [(e, q[0]) for e in cr.EDGE_EYES + ("aim_x", "aim_z", "aim_back") for q in cr.EDGE_QUATS if (e, q[0]) not in EDGE_LEFT_OUT]
    quats = {q[0]: q[1] for q in cr.EDGE_QUATS}
    st = np.zeros((len(names), 7), dtype=np.float32)
    for k, (e, q) in enumerate(names):
        st[k, :3], st[k, 3:] = eyes[e], quats[q]
    ref = scan_brute(st, AXIS_BEAMS, 0.0, 1000.0, sc.triangles, sc.body)
    return {"st": st, "names": names, "beams": AXIS_BEAMS, "sc": sc, "ref": ref}


@functools.lru_cache(maxsize=None)
def case_scenes():
    """Case 6: the gate prototype, K = 6 with counts (0, 1, 2, 3, 3, 3), G = 3, n = 256, scene ids from -1 to K."""
    from dronesim_amd.obstacles import ObstacleScenes
    K, G, n = 6, 3, 256
    rng = np.random.default_rng(61)
    pos, rpy = sr.random_placements(rng, K, G)
    scenes = ObstacleScenes(sr.gate(), pos, rpy, [0, 1, 2, 3, 3, 3])
    sid = rng.integers(-1, K + 1, n)
    st = draw_fleet(62, n, lo=(-3.0, -3.0, 0.5), hi=(3.0, 3.0, 3.5))
    beams = fan(16, up=True, down=True)
    ref = tuple(scan_brute(st, beams, T_MIN, T_MAX, scenes=scenes, scene_id=sid, ground=g) for g in (False, True))
    return {"st": st, "beams": beams, "scenes": scenes, "sid": sid, "ref": ref}


@functools.lru_cache(maxsize=None)
def case_carry():
    """scenes_ref.camera_scenes(0), scene 2: drones in front of slot 2 looking along +x see a hit in the LAST slot in front of one
    in the first (the carry_pixels situation).  -> dict(..., carry: beams hit in slot 0 alone whose nearest hit lies in slot 2)."""
    scenes = sr.camera_scenes(0)
    st = draw_fleet(63, 64, lo=(0.0, -0.4, 0.6), hi=(1.0, 0.4, 1.4), tilt=0.1)
    st[:, 3:] = np.stack([cr.quat_from_rpy(0.0, 0.0, y) for y in np.random.default_rng(64).uniform(-0.2, 0.2, 64)])
    sid = np.full(64, 2)
    beams = fan(8, elevations=(0.0, 0.15))
    ref = scan_brute(st, beams, T_MIN, 20.0, scenes=scenes, scene_id=sid)
    proto = scenes.prototype.triangles.astype(np.float64)
    t = []
    for g in (0, 2):
        R, tr = sr.placement64(scenes, 2, g)
        t.append(scan_brute(st, beams, T_MIN, 20.0, (proto @ R.T + tr).astype(np.float32), scenes.prototype.body)["t"])
    return {"st": st, "beams": beams, "scenes": scenes, "sid": sid, "ref": ref, "carry": np.isfinite(t[0]) & (t[1] < t[0])}


LATTICE_RANGE = 6.0


def lattice(models=("tello",), seed=71):
    """Case 7: 256 drones on a 16 x 16 lattice of 0.75 m pitch, +-0.15 m jitter in xy, z = 1 +- 0.08, rpy +-0.2, +-0.2, +-pi.
    -> (stored [256, 7], models [256], radius [256]); drone i is models[i mod len(models)]."""
    rng = np.random.default_rng(seed)
    i = np.arange(256)
    pos = np.stack([(i % 16) * 0.75, (i // 16) * 0.75, np.ones(256)], 1) + rng.uniform([-0.15, -0.15, -0.08], [0.15, 0.15, 0.08], (256, 3))
    rpy = rng.uniform([-0.2, -0.2, -np.pi], [0.2, 0.2, np.pi], (256, 3))
    st = np.zeros((256, 7), dtype=np.float32)
    st[:, :3] = np.round(pos * 1024.0) / 1024.0
    st[:, 3:] = np.stack([cr.quat_from_rpy(*e) for e in rpy])
    ms = [models[k % len(models)] for k in range(256)]
    return st, ms, dr.type_radii(ms)


def lattice_scene(subdiv=0):
    """scene(subdiv) moved into the lattice (it stands about (2 .. 3.75, 0, 1) in its own frame): + (3, 5, 0)."""
    from dronesim_amd.obstacles import ObstacleSet
    sc = cr.scene(subdiv)
    return ObstacleSet((sc.triangles.astype(np.float64) + np.array([3.0, 5.0, 0.0])).astype(np.float32), sc.body)


@functools.lru_cache(maxsize=None)
def lattice_scenes(subdiv=0):
    """Two scenes of one placement each of scene(subdiv) in the lattice, for scenes AND drones."""
    from dronesim_amd.obstacles import ObstacleScenes
    pos = np.array([[[3.0, 5.0, 0.0]], [[1.0, 8.0, 0.25]]])
    rpy = np.array([[[0.0, 0.0, 0.0]], [[0.1, -0.1, 1.0]]])
    return ObstacleScenes(cr.scene(subdiv), pos, rpy)


LATTICE_SCENE_ID = (np.arange(256) % 4) - 1          # -1 (no obstacles), 0, 1, 2 (= K: no obstacles)


@functools.lru_cache(maxsize=None)
def case_lattice(world, mixed=False):
    """world: None (drones alone), "set" / "set2" (scene(0) / scene(2) standing in the lattice) or "scenes" / "scenes2"
    (lattice_scenes of scene(0) / scene(2), scene ids LATTICE_SCENE_ID).  mixed: every other drone a hexa_6DOF_simple."""
    st, ms, rad = lattice(("tello", "hexa_6DOF_simple") if mixed else ("tello",))
    beams = fan(16, up=True, down=True)
    kw = {}
    if world in ("set", "set2"):
        sc = lattice_scene(0 if world == "set" else 2)
        kw = dict(tri=sc.triangles, body=sc.body)
    elif world in ("scenes", "scenes2"):
        kw = dict(scenes=lattice_scenes(0 if world == "scenes" else 2), scene_id=LATTICE_SCENE_ID)
    ref = scan_brute(st, beams, T_MIN, T_MAX, radius=rad, drone_range=LATTICE_RANGE, **kw)
    return {"st": st, "models": ms, "rad": rad, "beams": beams, "ref": ref, **kw}


LATTICE_WORLDS = ((None, False), ("set", False), ("set2", False), ("scenes", False), ("scenes2", False), (None, True))


def restated_inputs():
    """(name, restated t, reference) for every GPU case's inputs: what SCAN_RESTATED_WORST is measured over."""
    c1, c2, c3, c6, cc = case_main(0), case_main(2), case_edges(), case_scenes(), case_carry()
    for name, c in (("case 1", c1), ("case 2", c2)):
        for g in (False, True):
            yield f"{name}, ground {g}", restated_scan(c["st"], c["beams"], T_MIN, T_MAX, c["sc"].triangles, ground=g), c["ref"][g]
    yield "case 3", restated_scan(c3["st"], c3["beams"], 0.0, 1000.0, c3["sc"].triangles), c3["ref"]
    for g in (False, True):
        yield f"case 6, ground {g}", restated_scan(c6["st"], c6["beams"], T_MIN, T_MAX, scenes=c6["scenes"], scene_id=c6["sid"], ground=g), c6["ref"][g]
    yield "case 6, carry", restated_scan(cc["st"], cc["beams"], T_MIN, 20.0, scenes=cc["scenes"], scene_id=cc["sid"]), cc["ref"]
    for world, mixed in LATTICE_WORLDS:
        c = case_lattice(world, mixed)
        kw = {k: c[k] for k in ("scenes", "scene_id") if k in c}
        yield (f"case 7, {world}, mixed {mixed}",
               restated_scan(c["st"], c["beams"], T_MIN, T_MAX, c.get("tri"), radius=c["rad"], drone_range=LATTICE_RANGE, **kw), c["ref"])


def all_references():
    """(name, reference) of every GPU case: what the 1 % cap is asserted on."""
    for name, _, ref in restated_inputs():
        yield name, ref
