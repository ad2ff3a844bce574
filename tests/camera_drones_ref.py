"""The reference of the drones in the camera's images (dsim_depth_image_drones): a numpy fp64 brute-force caster over ALL spheres
(no grid, no cell walk) merged with camera_ref.cast, the sphere ambiguity mask, |n^ . d^| of the winning sphere, a float32
restatement of the kernel's sphere arithmetic from which the tests' tolerance is derived, and the scenes the tests share.

Semantics (include/dronesim_amd.h): drone j with R_j > 0 is the sphere of radius R_j about its STORED position; the sphere ray
starts at the eye in the world frame, e_w = p_i + (0, 0, L), the triangles and the plane keep e_w - offset_i; d is the same
unnormalised pixel ray.  The hit is the smallest root t of |e_w + t d - p_j| = R_j with near <= t <= min(far, range), the second
root when the first lies in front of near; the camera's own drone is never drawn.
"""
import numpy as np

from tests import camera_ref as cr

AMBIG_REL = 1e-3         # the sphere mask's one constant: relative closeness of rho to R, and of a root to near / far / range
FAR = 1000.0


def seg_drone(k):
    return -3 - k


# ---- the fp64 caster ----------------------------------------------------------------------------------------------------------------
def cast_spheres(centre, radius, eye, d, near, tmax, own=-1):
    """Nearest sphere hit of every ray over every sphere, fp64 on the fp32 inputs.  Every (ray, sphere) pair is looked at: a first
    pass keeps the pairs whose ray passes within 1.01 R of the centre (rho^2 = |m|^2 - (m.d)^2 / d.d, good to 1e-11 m here), the
    hit and the mask are then worked out for those pairs alone with the cancellation-free form.  Returns [H, W] arrays t (inf:
    none), idx (-1), ndot (|n^ . d^| at the hit, 1 where none) and the pairs for sphere_mask."""
    centre = np.asarray(centre, np.float32).astype(np.float64).reshape(-1, 3)
    radius = np.asarray(radius, np.float32).astype(np.float64).ravel()
    shp = d.shape[:-1]
    D = d.reshape(-1, 3)
    P = D.shape[0]
    a = (D * D).sum(1)
    drawn = (radius > 0.0) & np.isfinite(centre).all(1)
    if own >= 0:
        drawn[own] = False
    sel = np.nonzero(drawn)[0]
    m_all = centre[sel] - eye[None, :]
    b = D[:, 0:1] * m_all[None, :, 0] + D[:, 1:2] * m_all[None, :, 1] + D[:, 2:3] * m_all[None, :, 2]    # [P, S] (a matmul with an
    #                                                                      inner size of 3 is ten times slower at 65 536 spheres)
    rho2 = (m_all * m_all).sum(1)[None, :] - b * b / a[:, None]
    pi, sj = np.nonzero(rho2 <= (1.01 * radius[sel])[None, :] ** 2)
    si = sel[sj]
    m, Dp, ap, R = m_all[sj], D[pi], a[pi], radius[si]
    tc = (m * Dp).sum(1) / ap
    q = m - tc[:, None] * Dp
    rho = np.sqrt((q * q).sum(1))
    disc = R * R - rho * rho
    h = np.sqrt(np.maximum(disc, 0.0) / ap)
    t0, t1 = tc - h, tc + h
    t = np.where(t0 >= near, t0, t1)
    hit = (disc >= 0.0) & (t >= near) & (t <= tmax)
    best, idx, ndot = np.full(P, np.inf), np.full(P, -1, dtype=np.int64), np.ones(P)
    hp, hs, ht = pi[hit], si[hit], t[hit]
    order = np.lexsort((ht, hp))
    hp, hs, ht = hp[order], hs[order], ht[order]
    first = np.ones(hp.size, dtype=bool)
    first[1:] = hp[1:] != hp[:-1]
    hp, hs, ht = hp[first], hs[first], ht[first]
    best[hp], idx[hp] = ht, hs
    n = (eye[None, :] + ht[:, None] * D[hp] - centre[hs]) / radius[hs][:, None]
    ndot[hp] = np.abs((n * D[hp]).sum(1)) / np.sqrt(a[hp])
    return {"t": best.reshape(shp), "idx": idx.reshape(shp), "ndot": ndot.reshape(shp), "_pairs": (pi, rho, R, tc, t0, t1, disc >= 0.0),
            "_shape": shp}


def sphere_mask(sph, win, near, far, rng):
    """The sphere ambiguity mask, in the spirit of the triangle mask: a sphere at t <= (1 + 1e-3) winner (t: its first root, or the
    ray's closest point to it where it has none) whose ray distance rho satisfies |rho - R| <= 1e-3 R, or one of whose roots lies
    within 1e-3 relative of near, far or the range.  win [H, W]: the merged winner's t (inf where nothing is hit)."""
    pi, rho, R, tc, t0, t1, real = sph["_pairs"]
    w = (np.where(np.isfinite(win), win, min(far, rng)).reshape(-1) * (1.0 + AMBIG_REL))[pi]
    graze = (np.abs(rho - R) <= AMBIG_REL * R) & (tc <= w) & (tc > 0.0)
    clip = np.zeros(pi.size, dtype=bool)
    for plane in (near, far, rng):
        if np.isfinite(plane):
            clip |= (np.abs(t0 - plane) <= AMBIG_REL * plane) | (np.abs(t1 - plane) <= AMBIG_REL * plane)
    amb = np.zeros(win.size, dtype=bool)
    amb[pi[graze | (clip & real & (t0 <= w))]] = True
    return amb.reshape(sph["_shape"])


_NO_TRI = (np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], dtype=np.float32) + np.float32(1.0e6))      # beyond any far plane


def reference_image(tri, body, stored, radius, cam, quat, L, W, H, far=FAR, rng=None, ground=False, offset=None, label=None):
    """What dsim_depth_image_drones is specified to give for the camera on drone `cam` (an index into stored [N, 3], the fleet's
    stored positions; radius [N]): a dict of [H, W] arrays t, seg (body, -1, -2, -3 - label[j]), ambiguous (the union of the
    triangle mask and the sphere mask), ndot, is_drone.  tri None: no obstacle set.  offset: the camera drone's task offset."""
    stored = np.asarray(stored, np.float32)
    rng = far if rng is None else float(rng)
    if tri is None:
        tri, body = _NO_TRI, 0
    base = cr.reference_image(tri, body, stored[cam], quat, L, W, H, far=far, ground=ground, offset=offset)
    task = stored[cam].astype(np.float64) - (0.0 if offset is None else np.asarray(offset, np.float32).astype(np.float64))
    rays = cr.camera_rays(stored[cam], quat, L, W, H) if np.isfinite(stored[cam]).all() and np.isfinite(task).all() else None
    if rays is None or cr.camera_rays(task, quat, L, W, H) is None:      # no defined image: background everywhere
        return dict(base, is_drone=np.zeros((H, W), bool), sphere_mask_share=0.0)
    eye, d = rays
    near, far, rng = float(np.float32(L)), float(np.float32(far)), float(np.float32(rng))
    sph = cast_spheres(stored, radius, eye, d, near, min(far, rng), own=cam)
    wins = sph["t"] < base["t"]
    t = np.where(wins, sph["t"], base["t"])
    lab = np.arange(stored.shape[0]) if label is None else np.asarray(label)
    seg = np.where(wins, seg_drone(lab[np.maximum(sph["idx"], 0)]), base["seg"])
    smask = sphere_mask(sph, t, near, far, rng)
    return {"t": t, "seg": seg, "ambiguous": base["ambiguous"] | smask, "ndot": np.where(wins, sph["ndot"], base["ndot"]),
            "is_drone": wins, "sphere_mask_share": float(smask.mean())}


# ---- the kernel's sphere arithmetic in float32 ---------------------------------------------------------------------------------------
def rays32(pos, quat, L, W, H, fov_deg=60.0, aspect=1.0):
    """(eye [3], d [H, W, 3]) in float32, operation by operation as the kernel forms them (camera_ref.restated_image)."""
    f32 = np.float32
    p, q, L = np.asarray(pos, f32), np.asarray(quat, f32), f32(L)
    x, y, z, w = q
    s_ = f32(2.0) / (x * x + y * y + z * z + w * w)
    xs, ys, zs = x * s_, y * s_, z * s_
    r0, r3, r6 = f32(1.0) - (y * ys + z * zs), x * ys + w * zs, x * zs - w * ys
    fx, fy, fz = f32(1000.0) * r0, f32(1000.0) * r3, f32(1000.0) * r6 - L
    inv = f32(1.0) / np.sqrt(fx * fx + fy * fy + fz * fz)
    fx, fy, fz = fx * inv, fy * inv, fz * inv
    inv = f32(1.0) / np.sqrt(fx * fx + fy * fy)
    sx, sy = fy * inv, -fx * inv
    ux, uy, uz = sy * fz, -(sx * fz), sx * fy - sy * fx
    th = f32(np.tan(np.radians(float(f32(fov_deg))) / 2.0))
    tha = f32(th * f32(aspect))
    a = ((f32(2.0) * (np.arange(W, dtype=f32) + f32(0.5))) * f32(1.0 / W) - f32(1.0)) * tha
    b = (f32(1.0) - (f32(2.0) * (np.arange(H, dtype=f32) + f32(0.5))) * f32(1.0 / H)) * th
    a, b = a[None, :], b[:, None]
    d = np.stack([fx + a * sx + b * ux, fy + a * sy + b * uy, fz + b * uz + f32(0.0) * a], -1)
    assert d.dtype == np.float32
    return np.array([p[0], p[1], p[2] + L], f32), d


def restated_spheres(stored, radius, cam, quat, L, W, H, far=FAR, rng=None, chunk=512):
    """t [H, W] (inf: none) of the nearest sphere as the kernel computes it in float32 (numpy rounds every product and sum where the
    device contracts some into fused multiply-adds and takes a 1-ulp square root), over all spheres without the grid."""
    f32 = np.float32
    stored, radius = np.asarray(stored, f32), np.asarray(radius, f32)
    e, d = rays32(stored[cam], quat, L, W, H)
    dx, dy, dz = (d[..., k][..., None] for k in range(3))
    inv_a = f32(1.0) / (dx * dx + dy * dy + dz * dz)
    near, tmax = f32(L), min(f32(far), f32(far if rng is None else rng))
    best = np.full((H, W), np.inf, dtype=f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k0 in range(0, stored.shape[0], chunk):
            c, R = stored[k0:k0 + chunk], radius[k0:k0 + chunk].copy()
            if k0 <= cam < k0 + chunk:
                R[cam - k0] = f32(0.0)
            mx, my, mz = c[:, 0] - e[0], c[:, 1] - e[1], c[:, 2] - e[2]
            tc = (mx * dx + my * dy + mz * dz) * inv_a
            qx, qy, qz = mx - tc * dx, my - tc * dy, mz - tc * dz
            disc = R * R - (qx * qx + qy * qy + qz * qz)
            h = np.sqrt(np.maximum(disc, f32(0.0)) * inv_a)
            t0, t1 = tc - h, tc + h
            t = np.where(t0 >= near, t0, t1)
            hit = (R > 0) & (disc >= 0) & (t >= near) & (t <= tmax)
            assert t.dtype == np.float32
            best = np.minimum(best, np.where(hit, t, f32(np.inf)).min(-1))
    return best.astype(np.float64)


def walk_rays(stored, radius, grid, origin, d, own, near, tmax):
    """The walker the camera and the range scanner share: t [P] (inf: none) of rays (origin [P, 3] or [3], d [P, 3], own [P] or one
    index: the drone a ray never sees) by the kernels' own route in float32, ray by ray: the drones binned on grid = (cell, xmin,
    ymin, nx, ny) as the scatter pass bins them (a drone outside the box on the outside list, one whose position is not finite on
    no list), the 2-D walk over the box grown by one ring with the kernels' selects — s_in / s_out with fmin / fmax semantics, the
    3 x 3 block at the first cell, the newly adjacent column or row after a step — the early stop, then the outside list.  A ray
    whose origin or direction is not finite casts nothing.  Slow (a Python loop per ray).  -> (t, cell steps, sphere tests)."""
    f32 = np.float32
    stored, radius = np.asarray(stored, f32)[:, :3], np.asarray(radius, f32).copy()
    d = np.asarray(d, f32).reshape(-1, 3)
    P = d.shape[0]
    origin = np.broadcast_to(np.asarray(origin, f32), (P, 3))
    own = np.broadcast_to(np.asarray(own, np.int64), (P,))
    near, tmax = f32(near), f32(tmax)
    cell, xmin, ymin = (f32(v) for v in grid[:3])
    nx, ny = int(grid[3]), int(grid[4])
    icell = f32(1.0) / cell
    with np.errstate(invalid="ignore"):
        fx, fy = np.floor((stored[:, 0] - xmin) * icell), np.floor((stored[:, 1] - ymin) * icell)
    finite = np.isfinite(stored).all(1)
    inside = finite & (fx >= 0) & (fx < nx) & (fy >= 0) & (fy < ny)
    cells = {}
    for j in np.nonzero(inside)[0]:
        cells.setdefault((int(fx[j]), int(fy[j])), []).append(j)
    outside = [j for j in np.nonzero(finite & ~inside)[0] if radius[j] > 0]
    gx0, gx1 = xmin - cell, xmin + f32(nx + 1) * cell
    gy0, gy1 = ymin - cell, ymin + f32(ny + 1) * cell
    out = np.full(P, np.inf)
    steps = tests = 0

    def sphere(j, e, me, dv, inv_a, best):
        if j == me or not radius[j] > 0:
            return best
        m = stored[j] - e
        tc = (m[0] * dv[0] + m[1] * dv[1] + m[2] * dv[2]) * inv_a
        q = m - tc * dv
        disc = radius[j] * radius[j] - (q[0] * q[0] + q[1] * q[1] + q[2] * q[2])
        h = np.sqrt(max(disc, f32(0.0)) * inv_a)
        t0, t1 = tc - h, tc + h
        t = t0 if t0 >= near else t1
        return t if (disc >= 0 and near <= t <= tmax and t < best) else best

    with np.errstate(all="ignore"):
        for r in range(P):
            e, dv, me = origin[r], d[r], int(own[r])
            if not (np.isfinite(e).all() and np.isfinite(dv).all()):
                continue
            inv_a = f32(1.0) / (dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2])
            best = f32(np.inf)
            ix, iy = f32(1.0) / dv[0], f32(1.0) / dv[1]
            sx0, sx1, sy0, sy1 = (gx0 - e[0]) * ix, (gx1 - e[0]) * ix, (gy0 - e[1]) * iy, (gy1 - e[1]) * iy
            s_in = np.fmax(np.fmax(np.fmin(sx0, sx1), np.fmin(sy0, sy1)), near)
            s_out = np.fmin(np.fmin(np.fmax(sx0, sx1), np.fmax(sy0, sy1)), np.fmin(tmax, best))
            in_x = dv[0] != 0 or gx0 <= e[0] <= gx1
            in_y = dv[1] != 0 or gy0 <= e[1] <= gy1
            if s_in <= s_out and in_x and in_y:
                qx, qy = e[0] + s_in * dv[0], e[1] + s_in * dv[1]
                cx = min(max(int(np.floor((qx - gx0) * icell)), 0), nx + 1) - 1
                cy = min(max(int(np.floor((qy - gy0) * icell)), 0), ny + 1) - 1
                stx, sty = (1 if dv[0] > 0 else -1), (1 if dv[1] > 0 else -1)
                dtx = cell * abs(ix) if dv[0] != 0 else f32(np.inf)
                dty = cell * abs(iy) if dv[1] != 0 else f32(np.inf)
                tmx = (gx0 + f32(cx + 1 + (1 if dv[0] > 0 else 0)) * cell - e[0]) * ix if dv[0] != 0 else f32(np.inf)
                tmy = (gy0 + f32(cy + 1 + (1 if dv[1] > 0 else 0)) * cell - e[1]) * iy if dv[1] != 0 else f32(np.inf)
                bx0, bx1, by0, by1 = cx - 1, cx + 1, cy - 1, cy + 1
                for it in range(nx + ny + 4):
                    for yy in range(max(by0, 0), min(by1, ny - 1) + 1):
                        for xx in range(max(bx0, 0), min(bx1, nx - 1) + 1):
                            for j in cells.get((xx, yy), ()):
                                best = sphere(j, e, me, dv, inv_a, best)
                                tests += 1
                    t_exit = min(tmx, tmy)
                    if best <= t_exit or t_exit >= s_out:
                        break
                    gx = tmx <= tmy
                    if gx:
                        cx += stx; tmx = f32(tmx + dtx)
                    else:
                        cy += sty; tmy = f32(tmy + dty)
                    steps += 1
                    if cx < -1 or cx > nx or cy < -1 or cy > ny:
                        break
                    bx0, bx1 = (cx + stx, cx + stx) if gx else (cx - 1, cx + 1)
                    by0, by1 = (cy - 1, cy + 1) if gx else (cy + sty, cy + sty)
            for j in outside:
                best = sphere(j, e, me, dv, inv_a, best)
            out[r] = best
    return out, steps, tests


def walked_spheres(stored, radius, cam, quat, L, W, H, grid, far=FAR, rng=None):
    """t [H, W] by the kernel's own route in float32, ray by ray (walk_rays, which the range scanner's reference shares, with the
    camera's rays): the drones binned on grid = (cell, xmin, ymin, nx, ny) as the scatter pass bins them (a drone outside the box
    on the outside list), the 2-D walk over the box grown by one ring with the kernel's selects — the 3 x 3 block at the first
    cell, the newly adjacent column or row after a step — the early stop, then the outside list.  Slow (a Python loop per ray).
    Also returns the mean cell steps and sphere tests per ray."""
    f32 = np.float32
    stored = np.asarray(stored, f32)
    e, d = rays32(stored[cam], quat, L, W, H)
    near, tmax = f32(L), min(f32(far), f32(far if rng is None else rng))
    t, steps, tests = walk_rays(stored, radius, grid, e, d.reshape(-1, 3), cam, near, tmax)
    return t.reshape(H, W), steps / (W * H), tests / (W * H)


# ---- the tests' scenes ---------------------------------------------------------------------------------------------------------------
def type_radii(models):
    from dronesim_amd.params import builtin_type
    return np.array([builtin_type(m).collision_sphere for m in models], dtype=np.float32)


def main_fleet(with_offsets):
    """camera_ref.fleet_state with the 65 drones that carry no camera moved into the scene: (stored [70, 7] float32 in the caller's
    numbering, offsets [70, 3] or None, models [70], radius [70])."""
    st, _, off = cr.fleet_state(with_offsets)
    others = np.array([i for i in range(cr.FLEET_N) if i not in cr.CAMERAS])
    p = np.random.default_rng(11).uniform([0.5, -2.5, 0.2], [6.0, 2.5, 2.5], (others.size, 3))
    p = np.round(p * 1024.0) / 1024.0
    if with_offsets:
        # a camera sees the drones where they are STORED, from its own stored position: with per-drone task offsets of up to 8 m the
        # cluster would lie out of every view, so drone j of the 65 is stored with the offset of camera j mod 5 (multiples of 1/4 m on
        # multiples of 2^-10 m: exact in float32) — every camera finds thirteen of them where it finds the gate
        p = p + off[np.asarray(cr.CAMERAS)[np.arange(others.size) % len(cr.CAMERAS)]]
    st[others, :3] = p.astype(np.float32)
    models = [cr.FLEET_MODELS[i % 2] for i in range(cr.FLEET_N)]
    return st, off, models, type_radii(models)


def main_reference(subdiv, res, with_offsets, rng=None, stored=None, radius=None):
    """[(without ground, with ground)] x the five cameras of the main scene; subdiv None: no obstacle set."""
    st, off, _, rad = main_fleet(with_offsets)
    if stored is not None:
        st = stored
    if radius is not None:
        rad = radius
    sc = cr.scene(subdiv) if subdiv is not None else None
    out = []
    for k, (c, L) in enumerate(zip(cr.CAMERAS, cr.camera_arms())):
        kw = dict(far=FAR, rng=rng, offset=None if off is None else off[c])
        tri, body = (sc.triangles, sc.body) if sc is not None else (None, None)
        out.append(tuple(reference_image(tri, body, st[:, :3], rad, c, st[c, 3:], L, res[0], res[1], ground=g, **kw) for g in (False, True)))
    return out


LATTICE_N = 4096
LATTICE_CAMERAS = (1040, 2085, 3001, 1500)
LATTICE_RPY = ((0.0, -0.011, 0.8), (0.0, -0.011, 2.1), (0.0, 0.0, 3.3), (0.0, 0.3, 0.5))


def lattice_fleet():
    """4 096 tellos on a 64 x 64 lattice of 1 m pitch at z = 1; four of them carry a camera: yaw 0.8 and 2.1 rad with the
    nose 0.011 rad up, which lays one pixel row into the layer of spheres (its rays meet drones 13 to 53 m away: long walks, and
    hits on both sides of a range of 20 m; a level camera sees nothing beyond 10 m, its rows cross the layer too steeply), level at
    yaw 3.3 rad, and pitched 0.3 rad."""
    i = np.arange(LATTICE_N)
    st = np.zeros((LATTICE_N, 7), dtype=np.float32)
    st[:, 0], st[:, 1], st[:, 2], st[:, 6] = i % 64, i // 64, 1.0, 1.0
    for c, rpy in zip(LATTICE_CAMERAS, LATTICE_RPY):
        st[c, 3:] = cr.quat_from_rpy(*rpy)
    return st


def lattice_reference(rng, res=(64, 48)):
    st = lattice_fleet()
    rad = type_radii(["tello"] * LATTICE_N)
    return [reference_image(None, None, st[:, :3], rad, c, st[c, 3:], cr.ARM["tello"], res[0], res[1], far=FAR, rng=rng)
            for c in LATTICE_CAMERAS]


# the float32 restatement's worst weighted sphere error against the caster over the tests' scenes (main scene: both resolutions,
# offsets on and off; the lattice: range 20 and none): measured by tests/test_camera_drones_cpu.py::
# test_restated_sphere_error_is_what_is_recorded; the GPU tests grant the kernel 4 x this on pixels where a sphere wins
SPHERE_RESTATED_WORST = 3.14e-7
SPHERE_TOL = 4.0 * SPHERE_RESTATED_WORST


# ---- the axis fleet: the edge table's rays against spheres (tests/test_gpu_camera_edges.py) ------------------------------------------
AXIS_N = 128
AXIS_CAMERA = 6                  # a tello (even numbers are tellos, odd ones up to 63 hexas: stored type-major)
AXIS_EYE = (0.0, 0.0, 1.0)       # the camera drone's position
AXIS_RANGE = 25.0                # cuts the 41 m group
AXIS_RES = ((17, 17), (1, 33))
# per viewing direction: depth -> the rows of the 1 x 33 image whose pixel-centre rays the drones there are laid on (row 16 is the
# level ray, which is row 8 of 17 x 17 as well); the first of a depth lies exactly on the ray's line in xy, the second 0.125 m
# beside it, a third on the line again
_AXIS_ROWS = {"+": {7.0: (20, 11), 19.0: (18, 13), 41.0: (16, 15, 17)}, "-": {7.0: (20, 11), 19.0: (16, 13)}}
_AXIS_SIDE = {7.0: (9, 6), 19.0: (7, 10), 41.0: (9, 11)}       # 17 x 17: (row, column) of one more drone per depth, off the zero column


def axis_fleet():
    """The edge table's four axis cameras (camera_ref.EDGE_QUATS, carried in turn by drone AXIS_CAMERA, a tello at AXIS_EYE) in
    front of 32 hexa_6DOF_simple (R = 0.202 m) laid sparsely on and beside the lines x = 0 and y = 0 through the camera, about 7, 19
    and 41 m away (41 m along +x and +y only), at the heights where pixel-centre rays of the zero column pass; 95 more tellos
    scattered above.  Returns (stored [128, 7] float32 with the camera looking along +x, models [128], radius [128], info): info
    names, per direction, the hexas by depth."""
    L = cr.ARM["tello"]
    st = np.zeros((AXIS_N, 7), dtype=np.float32)
    st[:, 6] = 1.0
    models = ["hexa_6DOF_simple" if (i % 2 == 1 and i < 64) else "tello" for i in range(AXIS_N)]
    hexas = iter(range(1, 64, 2))
    st[AXIS_CAMERA, :3] = AXIS_EYE
    info = {}
    for name, q, zero in cr.EDGE_QUATS:
        eye, d33 = cr.camera_rays(AXIS_EYE, np.array(q, np.float32), L, 1, 33)
        _, d17 = cr.camera_rays(AXIS_EYE, np.array(q, np.float32), L, 17, 17)
        side = np.zeros(3)
        side[zero] = 0.125
        by_depth = {}
        for D, rows in _AXIS_ROWS[name[0]].items():
            pts = [eye + D * d33[r, 0] + (side if k == 1 else 0.0) for k, r in enumerate(rows)]
            if name[0] == "+" or D < 41.0:
                pts.append(eye + D * d17[_AXIS_SIDE[D]])
            ids = []
            for p in pts:
                j = next(hexas)
                st[j, :3] = p
                ids.append(j)
            assert st[ids[0], zero] == 0.0                     # exactly on the ray's line in xy
            by_depth[D] = ids
        info[name] = by_depth
    assert next(hexas, None) is None
    rest = [i for i in range(AXIS_N) if models[i] == "tello" and i != AXIS_CAMERA]
    p = np.random.default_rng(23).uniform([-15.0, -15.0, 3.0], [35.0, 35.0, 30.0], (len(rest), 3))
    st[rest, :3] = (np.round(p * 1024.0) / 1024.0).astype(np.float32)
    return st, models, type_radii(models), info


def axis_grid(box=None):
    """(cell, xmin, ymin, nx, ny) of the axis fleet's sphere grid as Downwash.sphere_grid chooses it: over the fleet's bounding box,
    or over a pinned box."""
    from dronesim_amd.downwash import clearance_grid
    from dronesim_amd.params import builtin_type
    st = axis_fleet()[0]
    r_max = max(float(builtin_type(m).collision_sphere) for m in ("tello", "hexa_6DOF_simple"))
    lo, hi = ((float(st[:, 0].min()), float(st[:, 1].min())), (float(st[:, 0].max()), float(st[:, 1].max()))) if box is None else (box[:2], box[2:])
    return clearance_grid(lo, hi, r_max, max(0.25 - 2.0 * r_max, 0.0), AXIS_N)


def axis_pinned_box():
    """A drone_box for the axis fleet, (xmin, ymin, xmax, ymax), laid so that (with the grid's one-cell margin and the cell size
    clearance_grid gives it) the grid's high x border lies 0.1 m beyond the 41 m drones of the +x line, whose spheres (R = 0.2 m)
    then reach out of the outermost cell into the ring the walk's box is grown by; a cell border lies along y = 0, the line of the
    cameras along x, to float32 rounding; and every drone of the lines along y lies outside, on the outside list."""
    cell = axis_grid((-19.5, -1.0, 41.0, 1.0))[0]
    nx = int(np.ceil((41.1 + 19.5 + cell) / cell)) + 1
    lo_x = 41.1 - nx * cell + cell
    box = (lo_x, -2.0 * cell, lo_x + (nx - 2.5) * cell, 1.5 * cell)
    got = axis_grid(box)
    assert got[0] == cell and got[3] == nx and got[4] == 6 and abs(got[1] + nx * cell - 41.1) < 1e-9 and abs(got[2] + 3.0 * cell) < 1e-12, got
    return box


def axis_reference(quat, res, rng=None, subdiv=None):
    """reference_image of the axis camera with the quaternion `quat`."""
    st, _, rad, _ = axis_fleet()
    sc = cr.scene(subdiv) if subdiv is not None else None
    tri, body = (sc.triangles, sc.body) if sc is not None else (None, None)
    return reference_image(tri, body, st[:, :3], rad, AXIS_CAMERA, np.array(quat, np.float32), cr.ARM["tello"], res[0], res[1], far=FAR, rng=rng)


def edge_fleet_reference(sc, pose, res, ground=False):
    """reference_image of one pose of camera_ref.edge_fleet(sc) with the fleet's other 69 drones drawn (the edge table's cameras
    sit around the set, the rest hover on a line 20 m off)."""
    st = cr.edge_fleet(sc)[0]
    rad = type_radii([cr.FLEET_MODELS[i % 2] for i in range(cr.FLEET_N)])
    return reference_image(sc.triangles, sc.body, st[:, :3], rad, pose["drone"], pose["quat"], pose["L"], res[0], res[1], far=FAR, ground=ground)
