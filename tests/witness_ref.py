"""The reference of the obstacle-witness tests (numpy only, so the CPU tests use it without a device).

fp64: the closest point of every triangle by the region walk (Ericson 5.1.5, with the face region's quotient, which fp64 affords),
the minimum over triangles and, on scenes, over placements — the point into each placement's frame with the float32 R and t the
device holds, widened to fp64, as scenes_ref.brute_scenes does, and the witness back through R.  A float32 restatement of the
kernel's arithmetic (tri_dist2's walk for the winner, tri_closest on the winner's record, back through R), from which the three
tolerances are derived (tests/README_witness.md), the two masks, and the inputs the GPU cases and the CPU checks share."""
import functools

import numpy as np

from tests import scenes_ref as sr
from tests.util import f32

# the float32 restatement's worst errors against the fp64 reference over the GPU cases' own inputs (tests/test_witness_cpu.py::
# test_restated_errors_are_what_is_recorded: not above the record, the record not padded); the kernel is granted 4 x each
RESTATED_ON = 8.30e-7         # distance from q + rel to the triangle the witness is said to lie on (worst: the placed soup)
RESTATED_OPT = 7.82e-7        # | |rel| - d_ref |                                                    (worst: the placed soup)
RESTATED_POS = 8.28e-7        # |w - w*| outside the strict mask                                     (worst: the placed soup)
TOL_ON, TOL_OPT, TOL_POS = 4.0 * RESTATED_ON, 4.0 * RESTATED_OPT, 4.0 * RESTATED_POS
E = TOL_ON + TOL_OPT          # what the position bound is made of
TIE_CAP, STRICT_CAP = 0.01, 0.15
STRICT_DIST, STRICT_SEP = 1e-4, 1e-5


# ---- fp64 ----------------------------------------------------------------------------------------------------------------------------
def closest(p, tri, chunk=256):
    """The closest point of every triangle tri [T, 3, 3] to every point p [P, 3], fp64: (W [P, T, 3], D [P, T]).  The region walk
    in the order of the book: the first region that holds decides."""
    p, tri = np.asarray(p, dtype=np.float64), np.asarray(tri, dtype=np.float64)
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    ab, ac = b - a, c - a
    W = np.empty((p.shape[0], tri.shape[0], 3))
    D = np.empty((p.shape[0], tri.shape[0]))
    dot = lambda u, e: np.einsum("ptk,tk->pt", u, e)
    for k0 in range(0, p.shape[0], chunk):
        q = p[k0:k0 + chunk, None, :]
        ap, bp, cp = q - a[None], q - b[None], q - c[None]
        d1, d2, d3, d4, d5, d6 = dot(ap, ab), dot(ap, ac), dot(bp, ab), dot(bp, ac), dot(cp, ab), dot(cp, ac)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        with np.errstate(divide="ignore", invalid="ignore"):
            tab, tac, tbc = d1 / (d1 - d3), d2 / (d2 - d6), (d4 - d3) / ((d4 - d3) + (d5 - d6))
            den = va + vb + vc
            fv, fw = vb / den, vc / den
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
        zero, one = np.zeros_like(d1), np.ones_like(d1)
        v = np.select(conds, [zero, one, tab, zero, zero, 1.0 - tbc], fv)
        w = np.select(conds, [zero, zero, zero, one, tac, tbc], fw)
        x = a[None] + v[..., None] * ab[None] + w[..., None] * ac[None]
        W[k0:k0 + chunk] = x
        D[k0:k0 + chunk] = np.linalg.norm(q - x, axis=2)
    return W, D


def _finish(q, D, W, tri_body, n_tri, nb, rad, margin, e=None):
    """q [n, 3]; D [n, M], W [n, M, 3] over the M = G n_tri candidates (inf / anything where there is none), in the task frame."""
    e = E if e is None else e
    n = q.shape[0]
    r = np.asarray(rad, dtype=np.float32).astype(np.float64)
    some = np.isfinite(D).any(1) if D.shape[1] else np.zeros(n, bool)
    idx = np.where(some, np.argmin(np.where(np.isfinite(D), D, np.inf), axis=1), 0) if D.shape[1] else np.zeros(n, np.int64)
    d = np.where(some, D[np.arange(n), idx], np.inf) if D.shape[1] else np.full(n, np.inf)
    inr = (r > 0) & some & (d - r < margin)
    w = np.where(inr[:, None], W[np.arange(n), idx], q) if D.shape[1] else q.copy()
    tie, strict = np.zeros(n, bool), np.zeros(n, bool)
    for i in np.nonzero(inr)[0]:
        sep = np.linalg.norm(W[i] - w[i], axis=1)
        gap = D[i] - d[i]
        tie[i] = bool(((gap <= 2.0 * e) & (sep > 2.0 * np.sqrt(2.0 * d[i] * e) + e)).any())
        strict[i] = bool(((gap <= STRICT_DIST) & (sep > STRICT_SEP)).any())
    body = (idx // n_tri) * nb + tri_body[idx % n_tri]
    return {"rel": np.where(inr[:, None], w - q, 0.0), "d": d, "tri": np.where(inr, idx, -1), "in": inr, "tie": tie, "strict": strict,
            "clr": np.where(inr, d - r, margin), "near": np.where(inr, body, -1), "w": w, "q": q,
            "contacts": int(((r > 0) & some & (d - r < 0)).sum())}


def brute_witness(p32, obst, rad, margin, off32=None, e=None):
    """The witness of a plain set, fp64 on the fp32 inputs: a dict — rel [n, 3] (w* - q, zeros without a witness), d, tri (-1), in,
    the tie and the strict mask, clr, near, w (the witness in the task frame), q, contacts."""
    q = sr._task_points(p32, off32)
    W, D = closest(q, obst.triangles)
    return _finish(q, D, W, obst.body.astype(np.int64), obst.n_tri, obst.n_bodies, rad, margin, e)


def brute_witness_scenes(p32, scenes, scene_id, rad, margin, off32=None, e=None):
    """... of the placements of each drone's scene: the point into the placement's frame, R^T (q - t), with the float32 R and t
    the device holds; the closest point there; the VECTOR to it back through R: w = q + R (w_local - q_local).  (R holds nine
    rounded float32 entries and is orthonormal to 6e-8 only, so R w_local + t is another point, (I - R R^T)(q - t) away: 8e-7 m at
    14 m.  The vector's route loses 6e-8 of its own length only, and it is the kernel's.)  The candidates are instance-major,
    g n_tri + t."""
    q = sr._task_points(p32, off32)
    sid = np.asarray(scene_id, dtype=np.int64)
    n, G, proto = q.shape[0], scenes.G, scenes.prototype
    T = proto.n_tri
    valid = (sid >= 0) & (sid < scenes.K)
    cnt = np.where(valid, scenes.count[np.clip(sid, 0, scenes.K - 1)], 0)
    D, W = np.full((n, G * T), np.inf), np.zeros((n, G * T, 3))
    for g in range(G):
        m = np.nonzero(cnt > g)[0]
        if not len(m):
            continue
        R, t = (np.stack(x) for x in zip(*(sr.placement64(scenes, k, g) for k in sid[m])))
        local = np.einsum("nji,nj->ni", R, q[m] - t)
        Wl, Dl = closest(local, proto.triangles)
        D[m, g * T:(g + 1) * T] = Dl
        W[m, g * T:(g + 1) * T] = q[m][:, None, :] + np.einsum("nij,ntj->nti", R, Wl - local[:, None, :])
    return _finish(q, D, W, proto.body.astype(np.int64), T, proto.n_bodies, rad, margin, e)


def on_surface(q, rel, tri, obst, scenes=None, scene_id=None):
    """Distance from q + rel [n, 3] to the triangle tri [n] names, fp64.  On scenes in the placement's own frame, R^T (q - t) +
    R^T rel against the prototype's triangle: what the float32 R is not orthonormal by then scales with |rel|, not with |q - t|."""
    proto = (obst if scenes is None else scenes.prototype).triangles.astype(np.float64)
    T = proto.shape[0]
    out = np.empty(len(q))
    for i in range(len(q)):
        x = q[i] + rel[i]
        if scenes is not None:
            R, t = sr.placement64(scenes, int(scene_id[i]), int(tri[i] // T))
            x = R.T @ (q[i] - t) + R.T @ rel[i]
        out[i] = closest(x[None], proto[tri[i] % T][None])[1][0, 0]
    return out


def body_rotation(quat):
    """R(q) [n, 3, 3] of quaternions (x, y, z, w) of any positive length, fp64."""
    x, y, z, w = (np.asarray(quat, dtype=np.float64)[:, k] for k in range(4))
    s = 2.0 / (x * x + y * y + z * z + w * w)
    return np.stack([np.stack([1 - s * (y * y + z * z), s * (x * y - w * z), s * (x * z + w * y)], 1),
                     np.stack([s * (x * y + w * z), 1 - s * (x * x + z * z), s * (y * z - w * x)], 1),
                     np.stack([s * (x * z - w * y), s * (y * z + w * x), 1 - s * (x * x + y * y)], 1)], 1)


# ---- the kernel's arithmetic in float32 ----------------------------------------------------------------------------------------------
def tri_closest_32(rec, t, q):
    """rel = closest point - q, float32 [n, 3], of record t[i] for point q[i]: tri_closest of dsim_witness.hip operation by
    operation (numpy rounds every product and sum where the device contracts some into fused multiply-adds)."""
    a, ab, ac, nrm, e = (x[t] for x in rec)
    q = np.asarray(q, dtype=np.float32)
    one, zero = np.float32(1.0), np.float32(0.0)
    px, py, pz = (q[:, k] - a[:, k] for k in range(3))
    abx, aby, abz = (ab[:, k] for k in range(3))
    acx, acy, acz = (ac[:, k] for k in range(3))
    e00, e01, e11 = (e[:, k] for k in range(3))
    d1, d2 = abx * px + aby * py + abz * pz, acx * px + acy * py + acz * pz
    d3, d4, d5, d6 = d1 - e00, d2 - e01, d1 - e01, d2 - e11
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    d43, d56 = d4 - d3, d5 - d6
    num, den, mode = np.zeros_like(d1), np.ones_like(d1), np.full(d1.shape, 6)
    for cond, md, nu, de in (((va <= 0) & (d43 >= 0) & (d56 >= 0), 5, d43, d43 + d56), ((vb <= 0) & (d2 >= 0) & (d6 <= 0), 4, d2, d2 - d6),
                             ((d6 >= 0) & (d5 <= d6), 3, None, None), ((vc <= 0) & (d1 >= 0) & (d3 <= 0), 2, d1, d1 - d3),
                             ((d3 >= 0) & (d4 <= d3), 1, None, None), ((d1 <= 0) & (d2 <= 0), 0, None, None)):
        mode = np.where(cond, md, mode)
        if nu is not None:
            num, den = np.where(cond, nu, num), np.where(cond, de, den)
    with np.errstate(divide="ignore", invalid="ignore"):
        tt = np.where(den > 0, num * (one / den), zero).astype(np.float32)
    v = np.where(mode == 1, one, np.where(mode == 2, tt, np.where(mode == 5, one - tt, zero))).astype(np.float32)
    w = np.where(mode == 3, one, np.where((mode == 4) | (mode == 5), tt, zero)).astype(np.float32)
    ex, ey, ez = px - v * abx - w * acx, py - v * aby - w * acy, pz - v * abz - w * acz
    h = nrm[:, 0] * px + nrm[:, 1] * py + nrm[:, 2] * pz
    face = mode == 6
    out = np.stack([np.where(face, -(h * nrm[:, k]), -ek) for k, ek in enumerate((ex, ey, ez))], 1)
    assert out.dtype == np.float32
    return out


def restated_witness(p32, obst, rad, margin, off32=None, chunk=256):
    """(rel [n, 3] float32, tri [n], in [n]) as the unplaced kernel computes them, in float32: q = p - offset, the region walk over
    ALL triangles (no grid), the first least d2, sqrt, minus R against the margin, tri_closest on the winner."""
    q = np.asarray(p32, dtype=np.float32)
    if off32 is not None:
        q = q - np.asarray(off32, dtype=np.float32)
    r = np.asarray(rad, dtype=np.float32)
    rec = sr.records32(obst.triangles)
    n = q.shape[0]
    best, tri = np.full(n, np.inf, dtype=np.float32), np.zeros(n, dtype=np.int64)
    for k0 in range(0, n, chunk):
        d2 = sr.tri_dist2_32(rec, q[k0:k0 + chunk])
        tri[k0:k0 + chunk], best[k0:k0 + chunk] = d2.argmin(1), d2.min(1)
    inr = (r > 0) & ((np.sqrt(best) - r) < np.float32(margin))
    rel = tri_closest_32(rec, tri, q)
    return np.where(inr[:, None], rel, np.float32(0.0)), np.where(inr, tri, -1), inr


def restated_witness_scenes(p32, scenes, scene_id, rad, margin, off32=None, chunk=256):
    """... as the placed kernel computes them: per placement d = q - t, l = R^T d with every product and sum rounded, the walk, a
    strict < across placements in slot order; then tri_closest at the winner's local point and rel = sum_k col_k l_k."""
    q = np.asarray(p32, dtype=np.float32)
    if off32 is not None:
        q = q - np.asarray(off32, dtype=np.float32)
    r = np.asarray(rad, dtype=np.float32)
    sid = np.asarray(scene_id, dtype=np.int64)
    rec = sr.records32(scenes.prototype.triangles)
    n, T = q.shape[0], scenes.prototype.n_tri
    valid = (sid >= 0) & (sid < scenes.K)
    cnt = np.where(valid, scenes.count[np.clip(sid, 0, scenes.K - 1)], 0)
    best, tri, slot = np.full(n, np.inf, dtype=np.float32), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    loc = np.zeros((n, 3), dtype=np.float32)

    def local(mm, g):
        P = scenes.place[sid[mm], g]
        d = q[mm] - P[:, 9:]
        cols = [P[:, [k, 3 + k, 6 + k]] for k in range(3)]
        return np.stack([c[:, 0] * d[:, 0] + c[:, 1] * d[:, 1] + c[:, 2] * d[:, 2] for c in cols], 1), cols
    for g in range(scenes.G):
        m = np.nonzero(cnt > g)[0]
        for k0 in range(0, len(m), chunk):
            mm = m[k0:k0 + chunk]
            l, _ = local(mm, g)
            d2 = sr.tri_dist2_32(rec, l)
            b, t = d2.min(1), d2.argmin(1)
            better = b < best[mm]
            best[mm], tri[mm], slot[mm] = np.where(better, b, best[mm]), np.where(better, t, tri[mm]), np.where(better, g, slot[mm])
            loc[mm] = np.where(better[:, None], l, loc[mm])
    inr = (r > 0) & np.isfinite(best) & ((np.sqrt(best) - r) < np.float32(margin))
    rel = np.zeros((n, 3), dtype=np.float32)
    ix = np.nonzero(inr)[0]
    if len(ix):
        v = tri_closest_32(rec, tri[ix], loc[ix])
        P = scenes.place[sid[ix], slot[ix]]
        rel[ix] = np.stack([P[:, 3 * k] * v[:, 0] + P[:, 3 * k + 1] * v[:, 1] + P[:, 3 * k + 2] * v[:, 2] for k in range(3)], 1)
    assert rel.dtype == np.float32
    return rel, np.where(inr, slot * T + tri, -1), inr


def errors(rel, tri, ref, obst, scenes=None, scene_id=None):
    """(on-surface, optimality, position outside the strict mask, position over the tie bound outside the tie mask): the worst of
    each over the drones with a witness, of a result (rel [n, 3], tri [n]) against a reference dict."""
    m = ref["in"]
    ix = np.nonzero(m)[0]
    rel = np.asarray(rel, dtype=np.float64)
    on = on_surface(ref["q"][ix], rel[ix], np.asarray(tri)[ix], obst, scenes, None if scene_id is None else np.asarray(scene_id)[ix])
    opt = np.abs(np.linalg.norm(rel[ix], axis=1) - ref["d"][ix])
    pos = np.linalg.norm(rel[ix] - ref["rel"][ix], axis=1)
    d = ref["d"][ix]
    bound = 2.0 * (2.0 * np.sqrt(2.0 * d * E) + E)
    loose, strict = ~ref["tie"][ix], ~ref["strict"][ix]
    return (float(on.max(initial=0.0)), float(opt.max(initial=0.0)), float(pos[strict].max(initial=0.0)),
            float((pos[loose] / bound[loose]).max(initial=0.0)))


# ---- the inputs of the GPU cases -----------------------------------------------------------------------------------------------------
ONE_TRIANGLE = np.array([[[0.0, 0.0, 1.0], [2.0, 0.0, 1.0], [0.5, 1.5, 1.3]]])


def _settled(obst, rad, margin, draw, n, seed):
    from tests.obstacle_ref import brute
    decide = lambda p, o: (brute(p, obst.triangles, obst.body, rad[: len(p)], margin, o)[4], margin)
    pos, off, frac = _settle(np.random.default_rng(seed), draw, n, decide)
    assert frac <= 0.01, frac
    return pos, off


def _settle(rng, draw, n, decide):
    """The input rule of test_gpu_obstacles.py (numpy only: that module needs a device library to import)."""
    pos, off = draw(rng, n)
    redrawn = np.zeros(n, dtype=bool)
    for _ in range(50):
        c, margin = decide(pos, off)
        bad = (np.abs(c) < sr.GUARD) | (np.abs(c - margin) < sr.GUARD)
        if not bad.any():
            return pos, off, redrawn.mean()
        redrawn |= bad
        p2, o2 = draw(rng, int(bad.sum()))
        pos[bad] = p2
        if off is not None:
            off[bad] = o2
    raise AssertionError("the input rule did not settle")


def _robobee(n):
    return sr._radius("robobee", n)


@functools.lru_cache(maxsize=None)
def case_one_triangle():
    """GPU case 1: one triangle, 700 robobees about it, margin 0.5: all seven regions on both sides."""
    from dronesim_amd.obstacles import ObstacleSet
    s, n, margin = ObstacleSet(ONE_TRIANGLE, 0), 700, 0.5
    rad = _robobee(n)
    draw = lambda rng, k: (f32(rng.uniform([-0.5, -0.5, 0.6], [2.5, 2.0, 1.8], (k, 3))), None)
    pos, off = _settled(s, rad, margin, draw, n, 3)
    return {"set": s, "rad": rad, "margin": margin, "pos": pos, "off": off, "ref": brute_witness(pos, s, rad, margin, off)}


@functools.lru_cache(maxsize=None)
def case_gate(offsets: bool):
    """GPU cases 2 and 3: the gate, 700 robobees (three tiles, the last partial), margin 1.0, drawn as test_gpu_obstacles.py draws
    them; with offsets of +-128 m."""
    s, n, margin = sr.gate(), 700, 1.0
    rad = _robobee(n)

    def draw(rng, k):
        q = rng.uniform([-0.55, -1.05, -0.9], [0.55, 1.05, 0.9], (k, 3))
        return sr.with_offsets(rng, q) if offsets else (f32(q), None)
    pos, off = _settled(s, rad, margin, draw, n, 11)
    return {"set": s, "rad": rad, "margin": margin, "pos": pos, "off": off, "ref": brute_witness(pos, s, rad, margin, off)}


@functools.lru_cache(maxsize=None)
def case_soup():
    """GPU case 4: the soup (records through L2), 768 hexa_6DOF inside its box and 256 (four whole waves) outside, margin 0.6."""
    from dronesim_amd.obstacles import watch_reach
    from dronesim_amd import params
    from tests.test_gpu_obstacles import soup
    s, n, margin = soup(), 1024, 0.6
    rad = sr._radius("hexa_6DOF", n)
    g, _, _ = s.grid(watch_reach([params.builtin_type("hexa_6DOF")], margin))
    lo, hi = np.array(list(g.lo), dtype=np.float64), np.array(list(g.hi), dtype=np.float64)
    p_in, _ = _settled(s, rad, margin, lambda rng, k: (f32(rng.uniform(-10.0, 10.0, (k, 3))), None), 768, 29)
    q = np.random.default_rng(30).uniform(-16.0, 16.0, (4096, 3))
    p_out = f32(q[((q < lo - 1e-3) | (q > hi + 1e-3)).any(1)][:256])
    assert len(p_out) == 256
    pos = np.concatenate([p_in, p_out])
    return {"set": s, "rad": rad, "margin": margin, "pos": pos, "off": None, "ref": brute_witness(pos, s, rad, margin)}


@functools.lru_cache(maxsize=None)
def scene_ref(name, offsets=False):
    """The witness reference of a case of scenes_ref (case_gates with and without offsets, case_ragged, case_soup)."""
    d = {"gates": lambda: sr.case_gates(offsets), "ragged": sr.case_ragged, "soup": sr.case_soup}[name]()
    return d, brute_witness_scenes(d["pos"], d["scenes"], d["scene_id"], d["rad"], d["margin"], d["off"])


def mask_shares(ref):
    """(tie mask share of all drones, strict mask share of the drones in reach)."""
    return float(ref["tie"].mean()), float(ref["strict"].sum()) / max(int(ref["in"].sum()), 1)
