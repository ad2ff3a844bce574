"""The reference of the nearest-neighbour observation (dsim_knn, Downwash.nearest, env.nearest_neighbors): brute force in fp64 on
the fp32 positions and velocities the device holds, the tie mask, the worlds the tests use and the comparison
(tests/README_knn.md has the rules and the tolerances).  numpy only: tests/test_knn_cpu.py checks it on the CPU."""
from typing import NamedTuple, Optional

import numpy as np

TIE = 1e-5       # [m] two consecutive sorted distances (or a distance and the radius) closer than this: index and order are not compared
ATOL = 1e-5      # [m], [m/s] distances, rel_pos, rel_vel: the drone watch's ATOL (two orders above the fp32 rounding of 1.5 m / 10 m/s)
EXEMPT_CAP = 0.01


class KnnRef(NamedTuple):
    index: np.ndarray        # [nr, k] world index in ascending (d, j), -1 in unused slots
    dist: np.ndarray         # [nr, k] fp64 distances, inf in unused slots
    rel_pos: np.ndarray      # [nr, k, 3] p_j - p_i, 0 in unused slots
    rel_vel: Optional[np.ndarray]   # [nr, k, 3] v_j - v_i, 0 in unused slots (None without velocities)
    count: np.ndarray        # [nr] drones with d < radius
    sorted_d: np.ndarray     # [nr, k + 1] the first k + 1 sorted distances below the radius, inf where there is none
    tie: np.ndarray          # [nr] bool: two consecutive of the first min(k, count) + 1 sorted distances closer than TIE
    edge: np.ndarray         # [nr] bool: some |d_ij - radius| < TIE (the count is ambiguous)
    d: np.ndarray            # [nr, m] every d_ij (inf on the diagonal and wherever a position is not finite)

    @property
    def exempt(self):
        return self.tie | self.edge


def brute(pos32, radius, k, lo=0, hi=None, vel32=None) -> KnnRef:
    """pos32 [m, 3] (vel32 [m, 3]) float32 -> the reference for the receivers [lo, hi) of the world."""
    p = np.asarray(pos32, dtype=np.float32).astype(np.float64)
    m = p.shape[0]
    hi = m if hi is None else hi
    nr = hi - lo
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.sqrt(((p[lo:hi, None, :] - p[None, :, :]) ** 2).sum(-1))
    d[~np.isfinite(d)] = np.inf
    d[np.arange(nr), np.arange(lo, hi)] = np.inf
    within = d < radius
    count = within.sum(1)
    dm = np.where(within, d, np.inf)
    order = np.argsort(dm, axis=1, kind="stable")[:, : k + 1]        # (stable: an exact tie goes to the lower index)
    sorted_d = np.take_along_axis(dm, order, axis=1)
    if sorted_d.shape[1] < k + 1:
        pad = k + 1 - sorted_d.shape[1]
        sorted_d = np.concatenate([sorted_d, np.full((nr, pad), np.inf)], 1)
        order = np.concatenate([order, np.zeros((nr, pad), dtype=order.dtype)], 1)
    used = np.isfinite(sorted_d[:, :k])
    index = np.where(used, order[:, :k], -1)
    dist = sorted_d[:, :k].copy()
    j = np.where(used, order[:, :k], np.arange(lo, hi)[:, None])
    with np.errstate(invalid="ignore"):
        rel_pos = np.where(used[..., None], p[j] - p[lo:hi, None, :], 0.0)
    rel_vel = None
    if vel32 is not None:
        v = np.asarray(vel32, dtype=np.float32).astype(np.float64)
        rel_vel = np.where(used[..., None], v[j] - v[lo:hi, None, :], 0.0)
    # the tie mask: the first min(k, count) + 1 sorted distances, the radius standing in for a missing (k + 1)-th
    e = sorted_d.copy()
    short = count < k + 1
    e[short, count[short]] = radius
    length = np.minimum(k, count) + 1
    with np.errstate(invalid="ignore"):
        gap = np.diff(e, axis=1)                                        # (inf - inf = nan, radius .. inf = inf: neither is < TIE)
        tie = ((gap < TIE) & (np.arange(k)[None, :] < (length - 1)[:, None])).any(1)
    edge = (np.abs(d - radius) < TIE).any(1)
    return KnnRef(index, dist, rel_pos, rel_vel, count, sorted_d, tie, edge, d)


# ---- the worlds -------------------------------------------------------------------------------------------------------------------
RADIUS = 1.5


def standard_world(seed, n_far=700, n_near=300):
    """700 drones uniform in 20 x 15 x 4 m and 300 in a 3 m cube inside it: sparse drones with a few or no neighbours, and a crowd
    whose drones have up to about 160.  (pos [n, 3], vel [n, 3]) float32-representable fp64, velocities up to 5 m/s per axis."""
    rng = np.random.default_rng(seed)
    far = rng.uniform(0.0, 1.0, (n_far, 3)) * np.array([20.0, 15.0, 4.0]) + np.array([-10.0, -7.5, 0.5])
    near = rng.uniform(0.0, 3.0, (n_near, 3)) + np.array([2.0, -1.0, 1.0])
    pos = np.concatenate([far, near])[rng.permutation(n_far + n_near)]
    vel = rng.uniform(-5.0, 5.0, pos.shape)
    return pos.astype(np.float32).astype(np.float64), vel.astype(np.float32).astype(np.float64)


def ragged_world(n=257, seed=29):
    """257 drones (a second, ragged workgroup) in 8 x 8 x 2 m: a dozen neighbours each at the standard radius."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.0, 1.0, (n, 3)) * np.array([8.0, 8.0, 2.0]) + np.array([3.0, -20.0, 0.5])
    vel = rng.uniform(-5.0, 5.0, pos.shape)
    return pos.astype(np.float32).astype(np.float64), vel.astype(np.float32).astype(np.float64)


def hetero_world(n=601, seed=31):
    """The env test's fleet: n drones in 14 x 12 x 3 m (the types alternate, so a storage order is in force)."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.0, 1.0, (n, 3)) * np.array([14.0, 12.0, 3.0]) + np.array([-7.0, -6.0, 1.0])
    return pos.astype(np.float32).astype(np.float64)


def slice_world(m=900, seed=41):
    """The world_pos test's world, far from the origin: m drones in 12 x 10 x 3 m."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.0, 1.0, (m, 3)) * np.array([12.0, 10.0, 3.0]) + np.array([-100.0, 100.0, 0.5])
    return pos.astype(np.float32).astype(np.float64)


def planted_world(k):
    """k + 1 drones at hand-picked distinct distances 0.30, 0.35, ... around receiver 0 (at the origin of the set), in directions
    that spiral round it, handed over far-to-near: the one left out of the k nearest is drone 1, the farthest, by construction.
    Every distance is below the standard radius and the planted drones are further from each other than from the receiver's
    list cut, which is all the test reads: it looks at receiver 0 only."""
    r = 0.30 + 0.05 * np.arange(k + 1)
    ang = 2.4 * np.arange(k + 1)
    sat = np.stack([r * np.cos(ang), r * np.sin(ang), 0.1 * np.cos(1.7 * np.arange(k + 1))], 1)
    sat *= (r / np.linalg.norm(sat, axis=1))[:, None]
    pos = np.concatenate([np.zeros((1, 3)), sat[::-1]]) + np.array([4.0, 2.0, 1.5])
    return pos.astype(np.float32).astype(np.float64)


def mirror_world():
    """Receiver 0 and two candidates, drones 1 and 2, that are mirror images about it (bit-equal d^2 in any rounding: the
    differences are exact and each other's negatives), and a third, nearer candidate handed over last.  The receiver's list is
    [3, 1, 2]: an exact tie goes to the lower index, in whatever order the grid's scatter left the two in their cell."""
    c = np.array([1.0, 2.0, 1.0])
    off = np.array([0.5, 0.25, 0.125])
    return np.stack([c, c + off, c - off, c + np.array([0.0, 0.0, 0.25])]).astype(np.float64)


# ---- the comparison -----------------------------------------------------------------------------------------------------------------
def compare(got, ref: KnnRef, k, radius, pos32, vel32=None, lo=0, what=""):
    """got: (index [k, n], dist, rel_pos [k, 3, n], rel_vel, count) as numpy arrays (None: not asked for) of the receivers
    [lo, lo + n).  Outside the mask, indices, order and count exactly; distances (as sorted values, a missing one standing at
    the radius), rel_pos and rel_vel with ATOL everywhere; unused slots -1 / +inf / 0 exactly."""
    index, dist, rel_pos, rel_vel, count = got
    n = index.shape[1]
    ok = ~ref.exempt
    assert ref.exempt.mean() <= EXEMPT_CAP, (what, ref.tie.mean(), ref.edge.mean())
    index = index.T.astype(np.int64)
    m = np.asarray(pos32).shape[0]
    used = index >= 0
    assert index.shape == (n, k) and np.all(index[used] < m) and np.all(index[~used] == -1)
    assert np.all(used[:, :-1] >= used[:, 1:]), what                   # the used slots come first
    assert not np.any(index == np.arange(lo, lo + n)[:, None]), what   # nobody lists itself
    if count is not None:
        count = count.astype(np.int64)
        np.testing.assert_array_equal(count[ok], ref.count[ok], err_msg=what)
        assert np.all(np.abs(count - ref.count)[~ok] <= (np.abs(ref.d - radius) < TIE).sum(1)[~ok]), what
        np.testing.assert_array_equal(used.sum(1)[ok], np.minimum(k, ref.count)[ok], err_msg=what)
    np.testing.assert_array_equal(index[ok], ref.index[ok], err_msg=what)
    p = np.asarray(pos32, dtype=np.float32).astype(np.float64)
    j = np.where(used, index, np.arange(lo, lo + n)[:, None])
    worst = {}
    if dist is not None:
        dist = dist.T.astype(np.float64)
        assert np.all(np.isposinf(dist[~used])) and np.all(np.isfinite(dist[used])) and np.all(dist[used] < radius + ATOL), what
        assert np.all(np.diff(np.minimum(dist, radius), axis=1) >= 0.0), what           # ascending
        worst["dist"] = np.abs(np.minimum(dist, radius) - np.minimum(ref.dist, radius)).max()
    if rel_pos is not None:
        rel_pos = rel_pos.transpose(2, 0, 1).astype(np.float64)
        assert np.all(rel_pos[~used] == 0.0), what
        want = np.where(used[..., None], p[j] - p[lo:lo + n, None, :], 0.0)
        worst["rel_pos"] = np.abs(rel_pos - want).max()
        worst["rel_pos vs ref"] = np.abs(rel_pos - ref.rel_pos)[ok].max() if ok.any() else 0.0
    if rel_vel is not None:
        v = np.asarray(vel32, dtype=np.float32).astype(np.float64)
        rel_vel = rel_vel.transpose(2, 0, 1).astype(np.float64)
        assert np.all(rel_vel[~used] == 0.0), what
        want = np.where(used[..., None], v[j] - v[lo:lo + n, None, :], 0.0)
        worst["rel_vel"] = np.abs(rel_vel - want).max()
        worst["rel_vel vs ref"] = np.abs(rel_vel - ref.rel_vel)[ok].max() if ok.any() else 0.0
    full = (ref.count >= k).mean()
    print(f"knn {what}: k = {k}, {n} receivers, exempt {ref.exempt.mean():.4f} (tie {ref.tie.mean():.4f}, radius {ref.edge.mean():.4f}), "
          f"full lists {full:.2f}, busiest {int(ref.count.max())}, alone {(ref.count == 0).mean():.4f}; worst |got - ref|: "
          + ", ".join(f"{name} {val:.2e}" for name, val in worst.items()))
    for name, val in worst.items():
        assert val <= ATOL, (what, name, val)
