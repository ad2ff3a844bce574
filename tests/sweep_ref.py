"""The reference of the swept obstacle watch's tests: brute-force segment-triangle distances in fp64 (numpy only, so the CPU tests
can use it without a device).  No grid and no pieces: every chord against every triangle."""
import numpy as np

from tests.obstacle_ref import tri_dist


def seg_seg(p, u, e, d):
    """Distance between the segments p + s u [P, 3] and e + t d [T, 3] (s, t in [0, 1]), fp64 [P, T]: the closest points of
    the two lines where they fall inside both segments, else the least of the four end-against-segment distances (the minimum
    of a convex quadratic over the unit square lies inside it or on its border)."""
    p, u, e, d = (np.asarray(x, dtype=np.float64) for x in (p, u, e, d))
    r = p[:, None, :] - e[None, :, :]                              # [P, T, 3]
    a = (u * u).sum(1)[:, None]
    dd = (d * d).sum(1)[None, :]
    b = u @ d.T
    c = np.einsum("pk,ptk->pt", u, r)
    f = np.einsum("tk,ptk->pt", d, r)
    den = a * dd - b * b
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (b * f - c * dd) / den
        t = (a * f - b * c) / den
        inside = (den > 1e-14 * a * dd) & (s >= 0) & (s <= 1) & (t >= 0) & (t <= 1)
        w = r + s[..., None] * u[:, None, :] - t[..., None] * d[None, :, :]
        best = np.where(inside, np.sqrt((w * w).sum(-1)), np.inf)
        for s_fix in (0.0, 1.0):                                   # an end of the chord against the edge
            x = r + s_fix * u[:, None, :]
            tt = np.clip(np.einsum("tk,ptk->pt", d, x) / dd, 0.0, 1.0)
            w = x - tt[..., None] * d[None, :, :]
            best = np.minimum(best, np.sqrt((w * w).sum(-1)))
        for t_fix in (0.0, 1.0):                                   # an end of the edge against the chord
            x = r - t_fix * d[None, :, :]
            ss = np.where(a > 0, np.clip(-np.einsum("pk,ptk->pt", u, x) / np.where(a > 0, a, 1.0), 0.0, 1.0), 0.0)
            w = x + ss[..., None] * u[:, None, :]
            best = np.minimum(best, np.sqrt((w * w).sum(-1)))
    return best


def pierces(q0, q1, tri):
    """Moeller-Trumbore: does the segment q0 -> q1 [P, 3] cross the face of triangle tri [T, 3, 3]?  bool [P, T]."""
    q0, q1, tri = (np.asarray(x, dtype=np.float64) for x in (q0, q1, tri))
    a, ab, ac = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    u = q1 - q0
    pv = np.cross(u[:, None, :], ac[None, :, :])
    det = np.einsum("tk,ptk->pt", ab, pv)
    tv = q0[:, None, :] - a[None, :, :]
    qv = np.cross(tv, ab[None, :, :])
    with np.errstate(divide="ignore", invalid="ignore"):
        bu = np.einsum("ptk,ptk->pt", tv, pv) / det
        bv = np.einsum("pk,ptk->pt", u, qv) / det
        bt = np.einsum("tk,ptk->pt", ac, qv) / det
        return (det != 0) & (bu >= 0) & (bv >= 0) & (bu + bv <= 1) & (bt >= 0) & (bt <= 1)


def seg_tri_dist(q0, q1, tri, chunk=128):
    """Distance from every segment q0 -> q1 [P, 3] to every triangle [T, 3, 3], fp64 [P, T]; and where it pierces."""
    q0, q1, tri = (np.asarray(x, dtype=np.float64) for x in (q0, q1, tri))
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    out, hit = np.empty((q0.shape[0], tri.shape[0])), np.empty((q0.shape[0], tri.shape[0]), dtype=bool)
    for k in range(0, q0.shape[0], chunk):
        x0, x1 = q0[k:k + chunk], q1[k:k + chunk]
        d = np.minimum(tri_dist(x0, tri), tri_dist(x1, tri))
        for e0, e1 in ((a, b), (a, c), (b, c)):
            d = np.minimum(d, seg_seg(x0, x1 - x0, e0, e1 - e0))
        h = pierces(x0, x1, tri)
        out[k:k + chunk], hit[k:k + chunk] = np.where(h, 0.0, d), h
    return out, hit


def sweep_brute(prev32, p32, tri32, body, radius, margin, sag=0.0, off32=None):
    """As obstacle_ref.brute, for the chord prev -> p and the radius + fp32(sag): clearance, nearest body (-1), |gap between the
    two closest bodies' minima|, contacts, raw clearance; on the fp32 inputs, in fp64."""
    q0 = np.asarray(prev32, dtype=np.float32).astype(np.float64)
    q1 = np.asarray(p32, dtype=np.float32).astype(np.float64)
    if off32 is not None:
        o = np.asarray(off32, dtype=np.float32).astype(np.float64)
        q0, q1 = q0 - o, q1 - o
    r = np.asarray(radius, dtype=np.float32).astype(np.float64)
    rs = r + float(np.float32(sag))
    d, _ = seg_tri_dist(q0, q1, np.asarray(tri32, dtype=np.float32))
    nb = int(np.max(body)) + 1
    per_body = np.stack([d[:, body == k].min(1) for k in range(nb)], 1) - rs[:, None]
    srt = np.sort(per_body, axis=1)
    c = srt[:, 0]
    gap = srt[:, 1] - srt[:, 0] if nb > 1 else np.full(len(c), np.inf)
    live = r > 0
    inr = live & (c < margin)
    return (np.where(inr, c, margin), np.where(inr, per_body.argmin(1), -1), gap, int((live & (c < 0)).sum()),
            np.where(live, c, np.inf))


def chords(rng, k, lo, hi, len_lo, len_hi):
    """k chords: a midpoint uniform in the box [lo, hi], a uniform direction, a length uniform in [len_lo, len_hi] -> (q0, q1) fp64."""
    mid = rng.uniform(lo, hi, (k, 3))
    v = rng.normal(size=(k, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    h = 0.5 * rng.uniform(len_lo, len_hi, (k, 1)) * v
    return mid - h, mid + h
