"""The reference of corridor clearance (dsim_corridor_clearance, corridor.Corridor, the env's corridor keyword): numpy only, so the
CPU tests use it without a device.  fp64 brute force, every segment against every triangle, no grid and no pieces, built from the
helpers the other references have: sweep_ref.seg_tri_dist for the distance, scenes_ref.placed_triangles for a drone's scene (on a
moved table: the ObstacleScenes motion.snapshot(tau) gives).  It works on the fp32 positions, rel rows, offsets and vertices the
device holds, offsets subtracted in fp64, and reduces per body, so that `body` can be judged where two bodies tie.
tests/README_corridor.md."""
import numpy as np

from tests.scenes_ref import placed_triangles
from tests.sweep_ref import seg_tri_dist

GROUND = -2                    # DSIM_SEG_GROUND
MAX_PIECES = 32


def ground_dist(e, d):
    """The half-space rule: the distance of the segment e -> e + d [..., 3] to z <= 0 is max(0, min(e.z, e.z + d.z))."""
    return np.maximum(0.0, np.minimum(e[..., 2], e[..., 2] + d[..., 2]))


def pieces(length, half):
    """The library's piece count: K = ceil(length / (2 half (1 - 2^-10))), at least 1; 1 throughout for half = inf."""
    if not np.isfinite(half):
        return np.ones_like(np.asarray(length, dtype=np.float64))
    return np.maximum(np.ceil(np.asarray(length, dtype=np.float64) / (2.0 * half * (1.0 - 2.0 ** -10))), 1.0)


def _per_body(q0, q1, tri, body, cols):
    """[P, cols]: the least distance of every segment to the triangles of each body (inf for a body without triangles)."""
    out = np.full((q0.shape[0], cols), np.inf)
    if len(tri) and len(q0):
        d, _ = seg_tri_dist(q0, q1, tri)
        for b in np.unique(body):
            out[:, int(b)] = d[:, body == b].min(1)
    return out


def corridor_brute(pos32, rel32, radius, margin, sag=0.0, off32=None, tri32=None, body=None, scenes=None, scene_id=None,
                   ground=False, index=None, half=np.inf):
    """What dsim_corridor_clearance is specified to give, in fp64 on the float32 inputs: pos [n, 3], rel [k, 3, n], radius [n],
    off [n, 3] or None; the world is (tri32 [T, 3, 3], body [T]) or (scenes, scene_id [n]), and the ground.  ``half``: the set's
    reach - (R_max + sag + margin), which decides which slots are served.  A dict of [k, n] arrays: clr = min(margin, c) (-inf
    where not evaluated or unserved), body (-1: none within the margin or no answer; -2: the ground), raw = c (inf where nothing
    was asked), gap between the two closest bodies' minima, evaluated and served (bool)."""
    p = np.asarray(pos32, dtype=np.float32).astype(np.float64)
    rel = np.asarray(rel32, dtype=np.float32).astype(np.float64)
    k, _, n = rel.shape
    e = p - np.asarray(off32, dtype=np.float32).astype(np.float64) if off32 is not None else p
    rs = np.asarray(radius, dtype=np.float32).astype(np.float64) + float(np.float32(sag))
    d = np.transpose(rel, (0, 2, 1))                                            # [k, n, 3]
    e_kn = np.broadcast_to(e[None], (k, n, 3))
    with np.errstate(invalid="ignore", over="ignore"):
        evaluated = np.isfinite(e).all(1)[None, :] & np.isfinite(d).all(2)
        if index is not None:
            evaluated &= np.asarray(index) >= 0
        length = np.linalg.norm(np.where(evaluated[..., None], d, 0.0), axis=2)
    served = evaluated & (pieces(length, half) <= MAX_PIECES)
    q0 = np.where(served[..., None], e_kn, 0.0).reshape(-1, 3)
    q1 = q0 + np.where(served[..., None], d, 0.0).reshape(-1, 3)
    if scenes is not None:
        sid = np.asarray(scene_id, dtype=np.int64)
        cols = scenes.G * scenes.n_bodies
        per = np.full((k * n, cols), np.inf)
        sid_kn = np.broadcast_to(sid[None], (k, n)).reshape(-1)
        for s in np.unique(sid[(sid >= 0) & (sid < scenes.K)]):
            tri, bod = placed_triangles(scenes, int(s))
            m = np.nonzero((sid_kn == s) & served.reshape(-1))[0]
            per[m] = _per_body(q0[m], q1[m], tri, bod, cols)
    elif tri32 is not None:
        body = np.asarray(body, dtype=np.int64)
        cols = int(body.max()) + 1
        m = np.nonzero(served.reshape(-1))[0]
        per = np.full((k * n, cols), np.inf)
        per[m] = _per_body(q0[m], q1[m], np.asarray(tri32, dtype=np.float32).astype(np.float64), body, cols)
    else:
        per = np.full((k * n, 0), np.inf)
    names = np.arange(per.shape[1])
    if ground:
        per = np.concatenate([per, ground_dist(q0, q1 - q0)[:, None]], 1)
        names = np.concatenate([names, [GROUND]])
    per = per.reshape(k, n, -1) - rs[None, :, None]
    srt = np.sort(per, axis=2)
    c = srt[..., 0]
    with np.errstate(invalid="ignore"):
        gap = srt[..., 1] - srt[..., 0] if per.shape[2] > 1 else np.full((k, n), np.inf)
    gap = np.where(np.isfinite(c) & ~np.isnan(gap), gap, np.inf)
    inr = served & (c < margin)
    return {"clr": np.where(served, np.where(inr, c, margin), -np.inf), "body": np.where(inr, names[per.argmin(2)], -1),
            "raw": np.where(served, c, np.inf), "gap": gap, "evaluated": evaluated, "served": served}
