"""The reference of the static-obstacle watch's tests: brute-force point-triangle distances in fp64 (numpy only, so the CPU tests
can use it without a device).  Not the region walk the kernel makes."""
import numpy as np


def tri_dist(p, tri, chunk=256):
    """Euclidean distance from every point p [P, 3] to every triangle tri [T, 3, 3], fp64 [P, T]: the least of the distances to
    the three edge segments, or the distance to the plane where the point projects into the triangle.  (Not the region walk the
    kernel makes.)"""
    p, tri = np.asarray(p, dtype=np.float64), np.asarray(tri, dtype=np.float64)
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    ab, ac = b - a, c - a
    nrm = np.cross(ab, ac)
    nn = (nrm * nrm).sum(1)
    e00, e01, e11 = (ab * ab).sum(1), (ab * ac).sum(1), (ac * ac).sum(1)
    out = np.empty((p.shape[0], tri.shape[0]))

    def seg(w, e):
        t = np.clip(np.einsum("ptk,tk->pt", w, e) / (e * e).sum(1), 0.0, 1.0)
        d = w - t[..., None] * e
        return np.sqrt(np.einsum("ptk,ptk->pt", d, d))
    for k0 in range(0, p.shape[0], chunk):
        w = p[k0:k0 + chunk, None, :] - a[None]
        d = np.minimum(np.minimum(seg(w, ab), seg(w, ac)), seg(p[k0:k0 + chunk, None, :] - b[None], c - b))
        d1, d2 = np.einsum("ptk,tk->pt", w, ab), np.einsum("ptk,tk->pt", w, ac)
        v, u = (e11 * d1 - e01 * d2) / nn, (e00 * d2 - e01 * d1) / nn
        h = np.abs(np.einsum("ptk,tk->pt", w, nrm)) / np.sqrt(nn)
        out[k0:k0 + chunk] = np.where((v >= 0) & (u >= 0) & (v + u <= 1), np.minimum(h, d), d)
    return out


def region(p, tri):
    """Which feature of ONE triangle is closest to each point: 0 face, 1-3 the edges ab, ac, bc, 4-6 the vertices a, b, c; and
    the side of the plane (+1 / -1)."""
    p, tri = np.asarray(p, dtype=np.float64), np.asarray(tri, dtype=np.float64)
    a, b, c = tri
    ab, ac = b - a, c - a
    w = p - a
    nn = np.cross(ab, ac)
    e00, e01, e11 = ab @ ab, ab @ ac, ac @ ac
    d1, d2 = w @ ab, w @ ac
    v, u = (e11 * d1 - e01 * d2) / (nn @ nn), (e00 * d2 - e01 * d1) / (nn @ nn)
    inside = (v >= 0) & (u >= 0) & (v + u <= 1)
    feats = []                                                    # distance to each edge's interior / each vertex
    for o, e in ((a, ab), (a, ac), (b, c - b)):
        t = ((p - o) @ e) / (e @ e)
        d = np.linalg.norm(p - o - np.clip(t, 0, 1)[:, None] * e, axis=1)
        feats.append(np.where((t > 0) & (t < 1), d, np.inf))
    feats += [np.linalg.norm(p - x, axis=1) for x in (a, b, c)]
    reg = np.where(inside, 0, 1 + np.argmin(np.stack(feats, 1), axis=1))
    return reg, np.sign(w @ nn)


def brute(p32, tri32, body, radius, margin, off32=None):
    """-> clearance, nearest body (-1), |gap between the two closest bodies' minima|, contacts; on the fp32 inputs, in fp64."""
    q = np.asarray(p32, dtype=np.float32).astype(np.float64)
    if off32 is not None:
        q = q - np.asarray(off32, dtype=np.float32).astype(np.float64)
    r = np.asarray(radius, dtype=np.float32).astype(np.float64)
    d = tri_dist(q, np.asarray(tri32, dtype=np.float32))
    nb = int(np.max(body)) + 1
    per_body = np.stack([d[:, body == k].min(1) for k in range(nb)], 1) - r[:, None]
    srt = np.sort(per_body, axis=1)
    c = srt[:, 0]
    gap = srt[:, 1] - srt[:, 0] if nb > 1 else np.full(len(c), np.inf)
    live = r > 0
    inr = live & (c < margin)
    return (np.where(inr, c, margin), np.where(inr, per_body.argmin(1), -1), gap, int((live & (c < 0)).sum()),
            np.where(live, c, np.inf))
