"""The depth camera's reference: a numpy fp64 brute-force ray caster over ALL triangles (no grid, no cell walk), the scenes
the camera tests share, and a float32 restatement of the kernel's own arithmetic from which the tests' tolerance is derived.

Camera model (BaseAviary._getDroneImages): eye = p + (0, 0, L), target = p + R(q) (1000, 0, 0), up = (0, 0, 1), near = L.
f = normalize(target - eye), s = normalize(f x up), u = s x f, th = tan(fov / 2); the ray of pixel (row r, col c) is
d = f + ((c + 1/2) / W 2 - 1) th aspect s + (1 - (r + 1/2) / H 2) th u, NOT normalised, so that the ray parameter t of a hit is
its eye-space depth.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
AMBIG_REL_T = 1e-3       # a triangle whose t is this close (relative) to the winner's ...
AMBIG_MARGIN = 1e-3      # ... and whose barycentric margin is this close to 0 makes the pixel ambiguous
SEG_GROUND = -2


# ---- scenes --------------------------------------------------------------------------------------------------------------------------
def subdivide(tri: np.ndarray, times: int) -> np.ndarray:
    """Every triangle into four by its edge midpoints (fp64 midpoints of fp32 vertices, rounded to fp32)."""
    t = np.asarray(tri, dtype=np.float32).reshape(-1, 3, 3)
    for _ in range(times):
        a, b, c = (t[:, k].astype(np.float64) for k in range(3))
        ab, bc, ca = 0.5 * (a + b), 0.5 * (b + c), 0.5 * (c + a)
        t = np.concatenate([np.stack(q, 1) for q in ((a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca))]).astype(np.float32)
    return t


def scene(subdiv: int = 0):
    """The committed gate (body 0; 96 triangles, each subdivided `subdiv` times) at (2, 0, 1) and a rotated box (body 1) behind
    and beside it: 108 triangles at subdiv 0, 1548 at subdiv 2."""
    from dronesim_amd.obstacles import ObstacleSet
    gate = ObstacleSet.from_urdf(os.path.join(GOLDEN, "gate_50_curved.urdf"), (2.0, 0.0, 1.0), (0, 0, 0))
    gate = ObstacleSet(subdivide(gate.triangles, subdiv), 0)
    return gate + ObstacleSet.box((3.5, 0.6, 0.8), (0.5, 0.7, 0.9), (0.3, 0.2, 0.5))


def soup_600():
    """600 random triangles in a 6 m box: a set above 512 triangles for the grid checks."""
    rng = np.random.default_rng(77)
    ctr = rng.uniform(-3.0, 3.0, (600, 1, 3))
    return (ctr + rng.uniform(-0.4, 0.4, (600, 3, 3))).astype(np.float32)


def quat_from_rpy(r, p, y):
    """xyzw of R = Rz(y) Ry(p) Rx(r) (p.getQuaternionFromEuler)."""
    cr, sr, cp, sp, cy, sy = np.cos(r / 2), np.sin(r / 2), np.cos(p / 2), np.sin(p / 2), np.cos(y / 2), np.sin(y / 2)
    return np.array([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
                     cr * cp * cy + sr * sp * sy])


def _rot_col0(q):
    x, y, z, w = (float(v) for v in q)
    s = 2.0 / (x * x + y * y + z * z + w * w)
    return np.array([1.0 - s * (y * y + z * z), s * (x * y + w * z), s * (x * z - w * y)])


# ---- the fp64 caster -----------------------------------------------------------------------------------------------------------------
def camera_rays(pos, quat, L, W, H, fov_deg=60.0, aspect=1.0):
    """(eye [3], d [H, W, 3]) in fp64 from the fp32 pose, or None where the camera has no defined image: a non-finite pose or
    |f x up|^2 < 1e-12 (Bullet's view matrix is NaN there)."""
    pos, quat, L = np.asarray(pos, np.float32).astype(np.float64), np.asarray(quat, np.float32).astype(np.float64), float(np.float32(L))
    if not (np.isfinite(pos).all() and np.isfinite(quat).all()) or not (quat @ quat) > 0.0:
        return None
    eye = pos + np.array([0.0, 0.0, L])
    f = pos + 1000.0 * _rot_col0(quat) - eye
    f /= np.linalg.norm(f)
    s = np.cross(f, [0.0, 0.0, 1.0])
    if not np.isfinite(s).all() or s @ s < 1e-12:
        return None
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    th = np.tan(np.radians(float(np.float32(fov_deg))) / 2.0)
    a = ((np.arange(W) + 0.5) / W * 2.0 - 1.0) * th * float(np.float32(aspect))
    b = (1.0 - (np.arange(H) + 0.5) / H * 2.0) * th
    return eye, f[None, None, :] + a[None, :, None] * s[None, None, :] + b[:, None, None] * u[None, None, :]


def cast(tri, body, eye, d, near, far, ground=False, chunk=256):
    """Nearest hit of every ray over every triangle, fp64 on the fp32 vertices.  Returns a dict of [H, W] arrays:
    t (inf: no hit), seg (body, -1 none, -2 ground), ambiguous (see the module constants), ndot (|n^ . d^| of the winning
    surface, 1 where nothing is hit).  ground="both": the pair (without, with the plane z = 0) from one pass over the triangles."""
    tri = np.asarray(tri, np.float32).reshape(-1, 3, 3).astype(np.float64)
    body = np.broadcast_to(np.asarray(body, np.int64), (tri.shape[0],))
    shp = d.shape[:-1]
    D = d.reshape(-1, 3)
    P = D.shape[0]
    near, far = float(np.float32(near)), float(np.float32(far))
    best, seg = np.full(P, np.inf), np.full(P, -1, dtype=np.int64)
    ndot = np.ones(P)
    dn = D / np.linalg.norm(D, axis=1, keepdims=True)
    per_chunk = []
    for k0 in range(0, tri.shape[0], chunk):
        a, ab, ac = tri[k0:k0 + chunk, 0], tri[k0:k0 + chunk, 1] - tri[k0:k0 + chunk, 0], tri[k0:k0 + chunk, 2] - tri[k0:k0 + chunk, 0]
        n = np.cross(ab, ac)
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        pv = np.cross(D[:, None, :], ac[None, :, :])                   # [P, T, 3]
        det = (pv * ab[None]).sum(-1)
        tv = eye[None, None, :] - a[None]
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            u = (tv * pv).sum(-1) * inv
            qv = np.cross(np.broadcast_to(tv, pv.shape), ab[None])
            v = (D[:, None, :] * qv).sum(-1) * inv
            t = (ac[None] * qv).sum(-1) * inv
            m = np.minimum(np.minimum(u, v), 1.0 - u - v)              # barycentric margin (NaN for a parallel ray)
        hit = (m >= 0.0) & (t >= near) & (t <= far)
        th_ = np.where(hit, t, np.inf)
        j = th_.argmin(1)
        tj = th_[np.arange(P), j]
        better = tj < best
        best = np.where(better, tj, best)
        seg = np.where(better, body[k0 + j], seg)
        ndot = np.where(better, np.abs((dn * n[j]).sum(-1)), ndot)
        per_chunk.append((t, m))
    def finish(best, seg, ndot, ground):
        if ground:
            with np.errstate(divide="ignore", invalid="ignore"):
                tg = -eye[2] / D[:, 2]
            ok = np.isfinite(tg) & (tg >= near) & (tg <= far) & (tg < best)
            best, seg, ndot = np.where(ok, tg, best), np.where(ok, SEG_GROUND, seg), np.where(ok, np.abs(dn[:, 2]), ndot)
        # ambiguity: a triangle at (nearly) the winning depth hit (nearly) on its rim; a hit (nearly) on a clipping plane
        win = np.where(np.isfinite(best), best, far)
        amb = np.zeros(P, dtype=bool)
        for t, m in per_chunk:
            with np.errstate(invalid="ignore"):
                amb |= ((np.abs(t - win[:, None]) <= AMBIG_REL_T * win[:, None]) & (np.abs(m) < AMBIG_MARGIN)).any(1)
                clip = (m >= -AMBIG_MARGIN) & ((np.abs(t - near) <= AMBIG_REL_T * near) | (np.abs(t - far) <= AMBIG_REL_T * far))
                amb |= (clip & (t <= win[:, None] * (1.0 + AMBIG_REL_T))).any(1)
        if ground:
            with np.errstate(invalid="ignore"):
                amb |= (np.abs(tg - near) <= AMBIG_REL_T * near) | (np.abs(tg - far) <= AMBIG_REL_T * far)
        return {"t": best.reshape(shp), "seg": seg.reshape(shp), "ambiguous": amb.reshape(shp), "ndot": ndot.reshape(shp)}

    if isinstance(ground, str):
        return finish(best, seg, ndot, False), finish(best, seg, ndot, True)
    return finish(best, seg, ndot, bool(ground))


def depth_buffer(t, near, far):
    """PyBullet's depth-buffer value of eye-space depth t (1.0: nothing hit)."""
    t = np.asarray(t, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(t), far * (t - near) / (t * (far - near)), 1.0)


def depth_buffer_to_t(dep, near, far):
    """The inverse: eye-space depth of a depth-buffer value (inf for 1.0)."""
    dep = np.asarray(dep, np.float64)
    with np.errstate(divide="ignore"):
        return np.where(dep >= 1.0, np.inf, far * near / (far - dep * (far - near)))


def reference_image(tri, body, pos, quat, L, W, H, far=1000.0, ground=False, fov_deg=60.0, aspect=1.0, offset=None):
    """What dsim_depth_image is specified to give for one camera (metric depth), with the ambiguity mask."""
    pos = np.asarray(pos, np.float32).astype(np.float64)
    if offset is not None:
        pos = pos - np.asarray(offset, np.float32).astype(np.float64)
    cam = camera_rays(pos, quat, L, W, H, fov_deg, aspect) if np.isfinite(pos).all() else None
    if cam is None:
        none = {"t": np.full((H, W), np.inf), "seg": np.full((H, W), -1, dtype=np.int64), "ambiguous": np.zeros((H, W), bool),
                "ndot": np.ones((H, W))}
        return (none, none) if isinstance(ground, str) else none
    return cast(tri, body, cam[0], cam[1], float(np.float32(L)), far, ground)


# ---- the kernel's arithmetic in float32 ----------------------------------------------------------------------------------------------
def restated_image(tri, pos, quat, L, W, H, far=1000.0, fov_deg=60.0, aspect=1.0):
    """t [H, W] (inf: no hit) as the kernel computes it, operation by operation in float32 (numpy rounds every product and sum
    where the device contracts some into fused multiply-adds and takes a 1-ulp reciprocal), over all triangles without the
    grid.  The distance between this and cast() is what float32 itself costs; the GPU tests grant the kernel four times it."""
    f32 = np.float32
    tri = np.asarray(tri, f32).reshape(-1, 3, 3)
    rec_a = tri[:, 0]
    rec_ab = (tri[:, 1].astype(np.float64) - tri[:, 0]).astype(f32)   # the records: fp64 differences rounded once
    rec_ac = (tri[:, 2].astype(np.float64) - tri[:, 0]).astype(f32)
    p, q, L = np.asarray(pos, f32), np.asarray(quat, f32), f32(L)
    x, y, z, w = q
    s_ = f32(2.0) / (x * x + y * y + z * z + w * w)
    xs, ys, zs = x * s_, y * s_, z * s_
    r0, r3, r6 = f32(1.0) - (y * ys + z * zs), x * ys + w * zs, x * zs - w * ys
    fx, fy, fz = f32(1000.0) * r0, f32(1000.0) * r3, f32(1000.0) * r6 - L
    inv = f32(1.0) / np.sqrt(fx * fx + fy * fy + fz * fz)
    fx, fy, fz = fx * inv, fy * inv, fz * inv
    ss = fx * fx + fy * fy
    inv = f32(1.0) / np.sqrt(ss)
    sx, sy = fy * inv, -fx * inv
    ux, uy, uz = sy * fz, -(sx * fz), sx * fy - sy * fx
    ex, ey, ez = p[0], p[1], p[2] + L
    th = f32(np.tan(np.radians(float(f32(fov_deg))) / 2.0))
    tha = f32(th * f32(aspect))
    a = ((f32(2.0) * (np.arange(W, dtype=f32) + f32(0.5))) * f32(1.0 / W) - f32(1.0)) * tha
    b = (f32(1.0) - (f32(2.0) * (np.arange(H, dtype=f32) + f32(0.5))) * f32(1.0 / H)) * th
    a, b = a[None, :, None], b[:, None, None]
    dx, dy, dz = fx + a * sx + b * ux, fy + a * sy + b * uy, fz + b * uz
    ax, ay, az = (rec_a[:, k][None, None, :] for k in range(3))
    abx, aby, abz = (rec_ab[:, k][None, None, :] for k in range(3))
    acx, acy, acz = (rec_ac[:, k][None, None, :] for k in range(3))
    px, py, pz = dy * acz - dz * acy, dz * acx - dx * acz, dx * acy - dy * acx
    det = abx * px + aby * py + abz * pz
    tx, ty, tz = ex - ax, ey - ay, ez - az
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        idet = f32(1.0) / det
        u = (tx * px + ty * py + tz * pz) * idet
        qx, qy, qz = ty * abz - tz * aby, tz * abx - tx * abz, tx * aby - ty * abx
        v = (dx * qx + dy * qy + dz * qz) * idet
        t = (acx * qx + acy * qy + acz * qz) * idet
        hit = (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= L) & (t <= f32(far))
    assert t.dtype == np.float32
    return np.where(hit, t, f32(np.inf)).min(-1).astype(np.float64)


def walked_image(sc, pos, quat, L, W, H, far=1000.0):
    """t [H, W] by the kernel's own route in float32, pixel by pixel: slab clip against the ray grid's box, the Amanatides-Woo
    walk with the kernel's selects, the cell lists of ObstacleSet.ray_grid(), the restatement's triangle test, the early stop.
    Slow (a Python loop per ray): for small images.  Also returns cell steps and triangle tests per ray."""
    f32 = np.float32
    g,start,lst=sc.ray_grid()
    tri=sc.triangles
    a_=tri[:,0]; ab=(tri[:,1].astype(np.float64)-tri[:,0]).astype(f32); ac=(tri[:,2].astype(np.float64)-tri[:,0]).astype(f32)
    p,q,L=np.asarray(pos,f32),np.asarray(quat,f32),f32(L)
    x,y,z,w=q; s_=f32(2)/(x*x+y*y+z*z+w*w); xs,ys,zs=x*s_,y*s_,z*s_
    r0,r3,r6=f32(1)-(y*ys+z*zs), x*ys+w*zs, x*zs-w*ys
    fx,fy,fz=f32(1000)*r0,f32(1000)*r3,f32(1000)*r6-L
    inv=f32(1)/np.sqrt(fx*fx+fy*fy+fz*fz); fx,fy,fz=fx*inv,fy*inv,fz*inv
    inv=f32(1)/np.sqrt(fx*fx+fy*fy); sx,sy=fy*inv,-fx*inv
    ux,uy,uz=sy*fz,-(sx*fz),sx*fy-sy*fx
    e=np.array([p[0],p[1],p[2]+L],f32)
    th=f32(np.tan(np.radians(60.0)/2)); tha=th
    o=np.array(list(g.origin),f32); hi=np.array(list(g.hi),f32); cell=f32(g.cell); icell=f32(1)/cell
    nn=np.array([g.nx,g.ny,g.nz])
    out=np.full((H,W),np.inf); steps=0; tests=0
    with np.errstate(all='ignore'):
      for r in range(H):
        for c in range(W):
            ca=(f32(2)*(f32(c)+f32(.5))*f32(1/W)-f32(1))*tha; cb=(f32(1)-f32(2)*(f32(r)+f32(.5))*f32(1/H))*th
            d=np.array([fx+ca*sx+cb*ux, fy+ca*sy+cb*uy, fz+cb*uz],f32)
            idv=f32(1)/d
            t0=(o-e)*idv; t1=(hi-e)*idv
            tin=max(np.fmax.reduce(np.fmin(t0,t1)),L); tout=min(np.fmin.reduce(np.fmax(t0,t1)),f32(far))
            inside=all((d[k]!=0) or (o[k]<=e[k]<=hi[k]) for k in range(3))
            best=np.inf
            if not (tin<=tout and inside): continue
            qpt=e+f32(tin)*d
            cc=np.clip(np.floor((qpt-o)*icell).astype(int),0,nn-1)
            st=np.where(d>0,1,-1)
            dt=np.where(d!=0,cell*np.abs(idv),np.inf).astype(f32)
            tm=np.where(d!=0,(o+(cc+(d>0)).astype(f32)*cell-e)*idv,np.inf).astype(f32)
            for it in range(nn.sum()):
                ci=(cc[2]*g.ny+cc[1])*g.nx+cc[0]
                for t_ in lst[start[ci]:start[ci+1]]:
                    tests+=1
                    pv=np.array([d[1]*ac[t_,2]-d[2]*ac[t_,1], d[2]*ac[t_,0]-d[0]*ac[t_,2], d[0]*ac[t_,1]-d[1]*ac[t_,0]],f32)
                    det=ab[t_,0]*pv[0]+ab[t_,1]*pv[1]+ab[t_,2]*pv[2]
                    tv=e-a_[t_]; idet=f32(1)/det
                    u=(tv[0]*pv[0]+tv[1]*pv[1]+tv[2]*pv[2])*idet
                    qv=np.array([tv[1]*ab[t_,2]-tv[2]*ab[t_,1], tv[2]*ab[t_,0]-tv[0]*ab[t_,2], tv[0]*ab[t_,1]-tv[1]*ab[t_,0]],f32)
                    v=(d[0]*qv[0]+d[1]*qv[1]+d[2]*qv[2])*idet
                    t=(ac[t_,0]*qv[0]+ac[t_,1]*qv[1]+ac[t_,2]*qv[2])*idet
                    if u>=0 and v>=0 and u+v<=1 and t>=L and t<=f32(far) and t<best: best=t
                texit=min(tm)
                if best<=texit or texit>=tout: break
                gx=tm[0]<=tm[1] and tm[0]<=tm[2]; gy=(not gx) and tm[1]<=tm[2]; k=0 if gx else (1 if gy else 2)
                cc[k]+=st[k]; tm[k]+=dt[k]; steps+=1
                if cc[k]<0 or cc[k]>=nn[k]: break
            out[r,c]=best
    return out, steps/(W*H), tests/(W*H)


def t_error(t, ref):
    """|t - t_ref| |n^ . d^|-weighted relative error where both hit and the pixel is not ambiguous: the quantity the tolerance
    bounds, |t - t_ref| max(|n^ . d^|, 0.05) / t_ref."""
    ok = np.isfinite(t) & np.isfinite(ref["t"]) & ~ref["ambiguous"]
    if not ok.any():
        return 0.0
    return float((np.abs(t[ok] - ref["t"][ok]) * np.maximum(ref["ndot"][ok], 0.05) / ref["t"][ok]).max())


# ---- the GPU tests' fleet: five camera poses around scene() -------------------------------------------------------------------------
# the tests' fleet: 70 drones, even index tello, odd index hexa_6DOF_simple (stored type-major: another order than the caller's);
# five of them, named out of order, carry the five poses below
FLEET_N = 70
FLEET_MODELS = ("tello", "hexa_6DOF_simple")
ARM = {"tello": 0.0635, "hexa_6DOF_simple": 1.0635}
CAMERAS = (40, 7, 68, 12, 33)
# the float32 restatement's worst t_error against cast() over the tests' scenes (both sets, both resolutions, the five poses):
# measured by tests/test_camera_cpu.py::test_restated_error_is_what_is_recorded; the GPU tests grant the kernel 4 x this
RESTATED_WORST = 3.65e-7
KERNEL_TOL = 4.0 * RESTATED_WORST


def camera_arms():
    return [ARM[FLEET_MODELS[d % 2]] for d in CAMERAS]


def fleet_offsets():
    """[70, 3] task offsets, multiples of 1/4 m up to 8 m: the camera poses are multiples of 2^-10 m, so p + offset and the
    stored value minus the offset are exact in float32, and the cameras see the same numbers with and without offsets."""
    rng = np.random.default_rng(5)
    return rng.integers(-32, 33, (FLEET_N, 3)).astype(np.float64) * 0.25


def fleet_state(with_offsets: bool):
    """(stored [70, 7] float32 pos + quat in the caller's numbering, effective poses (pos [5, 3], quat [5, 4]) of CAMERAS,
    offsets [70, 3] or None).  The other drones hover on a line far from the scene."""
    pos, quat = camera_poses()
    st = np.zeros((FLEET_N, 7), dtype=np.float32)
    st[:, 0], st[:, 1], st[:, 2], st[:, 6] = np.arange(FLEET_N) * 0.5, -20.0, 3.0, 1.0
    off = fleet_offsets() if with_offsets else None
    for k, d in enumerate(CAMERAS):
        st[d, :3] = pos[k].astype(np.float64) + (off[d] if with_offsets else 0.0)
        st[d, 3:] = quat[k]
    eff = np.stack([(st[d, :3] - (off[d] if with_offsets else 0.0).astype(np.float32) if with_offsets else st[d, :3])
                    for d in CAMERAS]).astype(np.float32)
    return st, (eff, quat), off


def camera_poses():
    """(pos [5, 3], quat [5, 4] xyzw): inside the ray grid's box; outside looking in; outside looking away; 60 m off, rays
    entering the box late; rolled and pitched ~0.3 rad."""
    pos = np.array([[2.6, 0.1, 0.9], [0.2, 0.05, 0.95], [0.3, -0.2, 1.0], [-58.0, 0.4, 1.6], [0.6, 0.5, 1.4]])
    pos = (np.round(pos * 1024.0) / 1024.0).astype(np.float32)       # multiples of 2^-10 m: p + offset is exact in float32
    rpy = [(0.0, 0.0, 0.4), (0.0, 0.0, 0.05), (0.0, 0.0, 3.0), (0.0, 0.0, 0.0), (0.3, 0.3, -0.15)]
    return pos, np.array([quat_from_rpy(*e) for e in rpy], dtype=np.float32)


# ---- the edge table: axis-parallel rays, eyes on cell faces (tests/test_gpu_camera_edges.py) ---------------------------------------
# raw quaternions (the kernel normalises by 2 / q.q): for (0, 0, +-1, 1) q.q = 2 and r0 = 1 - 1 * 1 = 0 exactly.  On the centre
# column of an odd-width image ca = 0, so the component d.s of its rays — dy for the cameras along x, dx for those along y — is
# exactly zero in float32 (EDGE_QUATS' third entry names it); the yaw pi / 4 camera has no such column
EDGE_QUATS = (("+x", (0.0, 0.0, 0.0, 1.0), 1), ("-x", (0.0, 0.0, 1.0, 0.0), 1), ("+y", (0.0, 0.0, 1.0, 1.0), 0), ("-y", (0.0, 0.0, -1.0, 1.0), 0))
EDGE_DIAG = ("diag", tuple(float(v) for v in quat_from_rpy(0.0, 0.0, np.pi / 4).astype(np.float32)), None)
EDGE_EYES = ("corner", "lo_x", "hi_y", "off_y", "off_corner")
# every eye with the four axis cameras; yaw pi / 4 from the first two only: from hi_y and off_y it sees nothing, and from
# off_corner it grazes the gate's plane (17 to 19 of 289 pixels ambiguous, 33 of 33 at 1 x 33: over the 1 % cap, so left out)
EDGE_RES = ((17, 17), (1, 33), (33, 1), (1, 1), (5, 7))
EDGE_EYE_Z = 0.9635
# the fleet's drones that carry the 22 edge poses, in the table's order: both parities, so both arms (0.0635 / 1.0635) among the
# axis cameras; the two yaw pi / 4 cameras have the short arm (with the long one, whose near plane is 1.06 m away, the camera at the
# corner has 3 of 289 pixels ambiguous and the one on the low x face 1 of 33 at 33 x 1: over the cap)
EDGE_CAMERAS = (3, 8, 21, 30, 45, 52, 9, 14, 61, 2, 17, 26, 35, 44, 53, 66, 11, 20, 29, 38, 56, 58)


def edge_eyes(sc):
    """{name: eye [3] float32} from the set's own ray grid.  corner: x, y and z on interior cell planes, each formed as the kernel
    forms a face, fl(origin[k] + fl(j) cell); lo_x: on the box's low x face, y on a cell plane; hi_y: on its high y face; off_y:
    0.5 m beyond the high y face (a camera along x has dy = 0 with the eye outside that slab); off_corner: one cell out in x and y."""
    f32 = np.float32
    g = sc.ray_grid()[0]
    o, hi, cell = np.array(list(g.origin), f32), np.array(list(g.hi), f32), f32(g.cell)
    face = lambda k, j: f32(o[k] + f32(j) * cell)
    jx, jy, jz = g.nx // 2, g.ny // 3, g.nz // 2
    assert 0 < jx < g.nx and 0 < jy < g.ny and 0 < jz < g.nz
    z = f32(EDGE_EYE_Z)
    return {"corner": np.array([face(0, jx), face(1, jy), face(2, jz)], f32),
            "lo_x": np.array([o[0], face(1, jy), z], f32),
            "hi_y": np.array([f32(2.5), hi[1], z], f32),
            "off_y": np.array([f32(0.25), f32(hi[1] + f32(0.5)), z], f32),
            "off_corner": np.array([f32(o[0] - cell), f32(o[1] - cell), z], f32)}


def _below(ez, L):
    """pz with fl(pz + L) == ez: the stored height whose eye is exactly ez (searched among the neighbours of fl(ez - L))."""
    f32 = np.float32
    pz = f32(f32(ez) - f32(L))
    for cand in (pz, np.nextafter(pz, f32(np.inf)), np.nextafter(pz, f32(-np.inf))):
        if f32(cand + f32(L)) == f32(ez):
            return f32(cand)
    raise AssertionError((ez, L))


def edge_poses(sc):
    """The edge table of a set: a list of dicts eye (name), cam (name), drone (of the 70), L, pos [3] and quat [4] float32, zero
    (the component of d that is exactly 0 on the centre column of an odd-width image: 0, 1 or None), eye_xyz [3] float32."""
    eyes = edge_eyes(sc)
    combos = [(e, q) for e in EDGE_EYES for q in EDGE_QUATS] + [(e, EDGE_DIAG) for e in ("corner", "lo_x")]
    assert len(combos) == len(EDGE_CAMERAS)
    out = []
    for (e, (qn, q, zero)), d in zip(combos, EDGE_CAMERAS):
        L = ARM[FLEET_MODELS[d % 2]]
        eye = eyes[e]
        pos = np.array([eye[0], eye[1], _below(eye[2], L)], np.float32)
        out.append(dict(eye=e, cam=qn, drone=d, L=L, pos=pos, quat=np.array(q, np.float32), zero=zero, eye_xyz=eye))
    return out


def edge_fleet(sc):
    """(stored [70, 7] float32 in the caller's numbering, the table): fleet_state(False) with the table's poses on EDGE_CAMERAS."""
    st = fleet_state(False)[0]
    table = edge_poses(sc)
    for p in table:
        st[p["drone"], :3], st[p["drone"], 3:] = p["pos"], p["quat"]
    return st, table


# the edge pose whose 1 x 1024 and 1024 x 1 images (the documented maxima) are compared as well: the corner eye looking along -x
EDGE_STRIP = ("corner", "-x")
EDGE_STRIP_RES = ((1, 1024), (1024, 1))
# the float32 restatement's worst t_error against cast() over the edge table (both sets, the five resolutions, and the two strips
# of EDGE_STRIP): measured by tests/test_camera_cpu.py::test_edge_restated_error_is_what_is_recorded; on the edge images the
# kernel is granted 4 x max(RESTATED_WORST, EDGE_RESTATED_WORST)
EDGE_RESTATED_WORST = 3.32e-7
EDGE_KERNEL_TOL = 4.0 * max(RESTATED_WORST, EDGE_RESTATED_WORST)
