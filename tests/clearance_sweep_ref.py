"""The tests' own reference of the swept drone-drone contact watch (dsim_clearance_sweep): brute force in fp64 on the fp32 inputs the
device holds, an fp32 restatement of the kernel's pair arithmetic, and the inputs the GPU cases share (numpy only).
tests/README_clearance_sweep.md."""
import functools

import numpy as np

GUARD = 1e-4
# The worst |c32 - c64| of restated_pairs against sweep_pairs_brute over the GPU cases' own inputs (the drones whose clearance the
# device reports, c < margin), measured by tests/test_clearance_sweep_cpu.py, which keeps it honest: not below what it measures,
# not padded.  The kernel is granted four times it.
RESTATED_WORST = 7.3e-8
ATOL = 4.0 * RESTATED_WORST
TRAVEL_BAND = 1e-5          # the input rule keeps chord lengths this far (relative) from `travel`: the library's comparison sits
                            # 2^-20 below it in fp32, the reference's at it in fp64


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32)


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def collapse(prev32, pos32, travel):
    """fp64 copies (p0, p1) of the fp32 ends with the unswept chords collapsed to p1, and the unswept mask: a chord longer than
    travel, or with a non-finite component on either end."""
    p0, p1 = np.asarray(prev32, np.float32).astype(np.float64), np.asarray(pos32, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        length = np.sqrt(((p1 - p0) ** 2).sum(1))
        unswept = ~(np.isfinite(p0).all(1) & np.isfinite(p1).all(1)) | ~(length <= float(np.float32(travel)))
    p0 = np.where(unswept[:, None], p1, p0)
    return p0, p1, unswept


def pair_dist(p0i, p1i, p0j, p1j):
    """The closed form, broadcasting: the distance between two points that move linearly and together from (p0i, p0j) to
    (p1i, p1j): min(|d0|, |d1|, |d0 + s* Delta|), s* = clamp(-d0.Delta / Delta.Delta, 0, 1), 0 where Delta = 0."""
    d0, d1 = p0j - p0i, p1j - p1i
    g = d1 - d0
    gg = (g * g).sum(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(gg > 0, np.clip(-(d0 * g).sum(-1) / np.where(gg > 0, gg, 1.0), 0.0, 1.0), 0.0)
    e = d0 + s[..., None] * g
    return np.sqrt(np.minimum(np.minimum((d0 * d0).sum(-1), (d1 * d1).sum(-1)), (e * e).sum(-1)))


def sweep_pairs_brute(prev32, pos32, radius, margin, sag, travel):
    """prev32, pos32 [m, 3] float32, radius [m] -> (clearance, nearest (-1: none), second-smallest c_ij (inf: none), overlapping
    pairs (i < j), unswept drones with R > 0, raw clearance min_j c_ij (inf: none)), every pair against every pair in fp64."""
    p0, p1, unswept = collapse(prev32, pos32, travel)
    r = np.asarray(radius, np.float32).astype(np.float64)
    rs = r + float(np.float32(sag))
    m, margin = len(r), float(np.float32(margin))
    live = r > 0
    clr, near, second, raw, pairs = np.empty(m), np.empty(m, np.int64), np.empty(m), np.empty(m), 0
    for k0 in range(0, m, 256):
        k1 = min(k0 + 256, m)
        with np.errstate(invalid="ignore"):
            c = pair_dist(p0[k0:k1, None, :], p1[k0:k1, None, :], p0[None, :, :], p1[None, :, :]) - rs[k0:k1, None] - rs[None, :]
        c[~np.isfinite(c)] = np.inf                               # (a non-finite position is seen by nobody and sees nobody)
        c[~live[k0:k1], :] = np.inf
        c[:, ~live] = np.inf
        c[np.arange(k1 - k0), np.arange(k0, k1)] = np.inf
        j = c.argmin(1)
        cm = c[np.arange(k1 - k0), j]
        raw[k0:k1] = cm
        clr[k0:k1] = np.minimum(cm, margin)
        near[k0:k1] = np.where(cm < margin, j, -1)
        second[k0:k1] = np.sort(c, axis=1)[:, 1] if m > 1 else np.inf
        pairs += int(((c < 0) & (np.arange(m)[None, :] > np.arange(k0, k1)[:, None])).sum())
    return clr, near, second, pairs, int((unswept & live).sum()), raw


def restated_pairs(prev32, pos32, radius, sag, travel):
    """The kernel's pair arithmetic in float32, every product and sum rounded (numpy's float32 operations round each): the raw
    clearance min_j c_ij per drone, inf where nobody is seen."""
    p0, p1, _ = collapse(prev32, pos32, travel)
    p0, p1 = p0.astype(np.float32), p1.astype(np.float32)
    r = np.asarray(radius, np.float32)
    rs = r + np.float32(sag)
    m = len(r)
    out = np.empty(m)
    dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    for k0 in range(0, m, 256):
        k1 = min(k0 + 256, m)
        with np.errstate(invalid="ignore", divide="ignore"):
            d1 = p1[None, :, :] - p1[k0:k1, None, :]
            d0 = p0[None, :, :] - p0[k0:k1, None, :]
            g = d1 - d0
            gg, bg = dot(g, g), dot(d0, g)
            inv = np.float32(1.0) / np.where(gg > 0, gg, np.float32(1.0))
            t = np.where(gg > 0, np.minimum(np.maximum(-bg * inv, np.float32(0.0)), np.float32(1.0)), np.float32(0.0))
            e = d0 + t[..., None] * g
            d2 = np.minimum(np.minimum(dot(d0, d0), dot(d1, d1)), dot(e, e))
            c = (np.sqrt(d2) - rs[None, :]) - rs[k0:k1, None]
        assert c.dtype == np.float32
        c = c.astype(np.float64)
        c[~np.isfinite(c)] = np.inf
        c[r[k0:k1] <= 0, :] = np.inf
        c[:, r <= 0] = np.inf
        c[np.arange(k1 - k0), np.arange(k0, k1)] = np.inf
        out[k0:k1] = c.min(1)
    return out


# ---- the input rule ---------------------------------------------------------------------------------------------------------------
def directions(rng, k):
    v = rng.normal(size=(k, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def settle_chords(rng, pos32, draw_prev, radius, margin, sag, travel, fixed=None):
    """The GUARD rule on the swept c_ij: the chords (pos is never moved) of the drones of every pair within GUARD of touching or of
    the margin, and those whose length is within TRAVEL_BAND of travel, are re-drawn with draw_prev(rng, idx) until none is left;
    drones in `fixed` keep theirs.  Returns (prev32, fraction of drones re-drawn)."""
    m = len(pos32)
    fixed = np.zeros(m, bool) if fixed is None else fixed
    prev = draw_prev(rng, np.arange(m))
    redrawn = np.zeros(m, bool)
    r = np.asarray(radius, np.float32).astype(np.float64)
    rs = r + float(np.float32(sag))
    for _ in range(100):
        p0, p1, _ = collapse(prev, pos32, travel)
        length = np.sqrt(((prev.astype(np.float64) - p1) ** 2).sum(1))
        bad = np.isfinite(length) & (np.abs(length - float(np.float32(travel))) <= TRAVEL_BAND * travel)
        for k0 in range(0, m, 256):
            k1 = min(k0 + 256, m)
            c = pair_dist(p0[k0:k1, None, :], p1[k0:k1, None, :], p0[None, :, :], p1[None, :, :]) - rs[k0:k1, None] - rs[None, :]
            c[~np.isfinite(c)] = np.inf
            c[r[k0:k1] <= 0, :] = np.inf
            c[:, r <= 0] = np.inf
            c[np.arange(k1 - k0), np.arange(k0, k1)] = np.inf
            hit = (np.abs(c) < GUARD) | (np.abs(c - float(np.float32(margin))) < GUARD)
            assert not (hit & fixed[k0:k1, None] & fixed[None, :]).any(), "a planted pair violates the input rule"
            # (one new chord per pair: the drone of the higher index, or the partner of a planted one)
            bad[k0:k1] |= (hit & ((np.arange(m)[None, :] < np.arange(k0, k1)[:, None]) | fixed[None, :])).any(1) & ~fixed[k0:k1]
        if not bad.any():
            return prev, redrawn.mean()
        idx = np.flatnonzero(bad)
        prev[idx] = draw_prev(rng, idx)
        redrawn[idx] = True
    raise AssertionError("the input rule did not settle")


def cell_of(grid, xy):
    """Cell indices (cx, cy) of xy [k, 2] in a grid (cell, xmin, ymin, nx, ny) of downwash.clearance_grid, clamped as the kernels do."""
    cell, xmin, ymin, nx, ny = grid
    cx = np.clip(np.floor((xy[:, 0] - xmin) / cell).astype(np.int64), 0, nx - 1)
    cy = np.clip(np.floor((xy[:, 1] - ymin) / cell).astype(np.int64), 0, ny - 1)
    return cx, cy


# ---- the GPU cases' inputs --------------------------------------------------------------------------------------------------------
# case 1: two robobees swap sides, 0.05 m apart in y where they pass
SWAP_PREV = np.array([[-0.5, 0.025, 1.0], [0.5, -0.025, 1.0]])
SWAP_POS = np.array([[0.5, 0.025, 1.0], [-0.5, -0.025, 1.0]])
SWAP_TRAVEL, SWAP_MARGIN = 1.1, 0.5

CROWD_TRAVEL, CROWD_MARGIN = 0.3, 0.5
PLANT_FIRST, PLANT_PAIRS = 340, 9          # drones 340 .. 357 of the crowded world: three pairs along x, three along y, three at 15 degrees
PLANT_GAP = 0.31                            # centre distance at the start of the interval: below 2 R = 0.316
PLANT_DIAG = np.deg2rad(15.0)               # (at travel = 0.3 the pair ends 0.88 m apart: a steeper diagonal cannot be two 0.817 m cells apart in x)


@functools.lru_cache(maxsize=None)
def case_crowded():
    """GPU case 2: the 1 000 robobees of test_gpu_clearance._crowded_world as the CURRENT positions, a chord of uniform direction
    and length uniform in [0, 0.3] m behind every one, and PLANT_PAIRS planted pairs that overlap at the start of the interval
    and fly apart by 0.95 travel each: their ends lie in adjacent cells of the sweep's grid and two cells apart (along the
    flight's main axis) in the grid of 2 R + margin the point watch chooses."""
    from dronesim_amd.downwash import clearance_grid
    from tests.test_gpu_clearance import _crowded_world
    t, pos, rad, point_grid = _crowded_world(1000, CROWD_MARGIN)
    R = float(np.float32(t.collision_sphere))
    travel, margin = CROWD_TRAVEL, CROWD_MARGIN
    sweep_grid = clearance_grid((-20.0, -15.0), (20.0, 15.0), float(t.collision_sphere) + 0.0, margin + 2.0 * travel, 1000)   # (as Downwash.clearance_sweep)
    pos = pos.copy()
    prev_planted = {}
    cp, cs = point_grid[0], sweep_grid[0]
    fly = 0.95 * travel
    sep = PLANT_GAP + 2.0 * fly                                     # centre distance at the end
    found = 0
    for k in range(PLANT_PAIRS):
        kind = k // 3                                               # 0: along x, 1: along y, 2: 15 degrees off x
        u = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [np.cos(PLANT_DIAG), np.sin(PLANT_DIAG), 0.0]][kind])
        axis = 1 if kind == 1 else 0
        # the lower end 0.02 m below a border of the point grid, so that a whole cell of it lies between the two ends, and a border
        # of the sweep's grid between them as well: searched over the point grid's borders
        for b in range(5 + 3 * k, 36):
            lo_end = point_grid[1 + axis] + b * cp - 0.02
            hi_end = lo_end + sep * u[axis]
            if hi_end > point_grid[1 + axis] + (b + 1) * cp + 0.01 and \
               np.floor((lo_end - sweep_grid[1 + axis]) / cs) + 1 == np.floor((hi_end - sweep_grid[1 + axis]) / cs):
                break
        else:
            raise AssertionError("no border serves the planted pair")
        other = 1.5 + 2.5 * k                                   # the other horizontal coordinate of the lower end
        z = 0.7 + 0.6 * k
        a1 = np.array([lo_end, point_grid[2] + other, z]) if axis == 0 else np.array([point_grid[1] + other, lo_end, z])
        b1 = a1 + sep * u
        i = PLANT_FIRST + 2 * k
        pos[i], pos[i + 1] = a1, b1
        prev_planted[i], prev_planted[i + 1] = a1 + fly * u, b1 - fly * u
        found += 1
    pos32 = f32(pos)
    fixed = np.zeros(1000, bool)
    fixed[PLANT_FIRST:PLANT_FIRST + 2 * PLANT_PAIRS] = True
    planted_prev = f32(np.array([prev_planted[i] for i in range(PLANT_FIRST, PLANT_FIRST + 2 * PLANT_PAIRS)]))

    def draw_prev(rng, idx):
        p = f32(pos32[idx].astype(np.float64) - rng.uniform(0.0, travel, (len(idx), 1)) * directions(rng, len(idx)))
        sel = fixed[idx]
        p[sel] = planted_prev[idx[sel] - PLANT_FIRST]
        return p
    prev32, redrawn = settle_chords(np.random.default_rng(101), pos32, draw_prev, rad, margin, 0.0, travel, fixed)
    ref = sweep_pairs_brute(prev32, pos32, rad, margin, 0.0, travel)
    return dict(type=t, pos=pos32, prev=prev32, rad=rad, margin=margin, sag=0.0, travel=travel, ref=ref, redrawn=redrawn,
                point_grid=point_grid, sweep_grid=sweep_grid, box=(-20.0, -15.0, 20.0, 15.0))


MIXED_N, MIXED_MARGIN, MIXED_SAG, MIXED_TRAVEL = 600, 0.6, 0.01, 0.25


def mixed_types():
    """Robobee, tello and a type without a collision sphere."""
    from dronesim_amd import params
    ghost = params.builtin_type("tello")
    ghost.name, ghost.collision_sphere = "ghost", 0.0
    return [params.builtin_type("robobee"), params.builtin_type("tello"), ghost]


@functools.lru_cache(maxsize=None)
def case_mixed():
    """GPU case 3: 600 drones of three types dealt in turn (the caller's numbering; type-major storage permutes them) in a
    12 x 10 x 2 m box, chords of up to travel behind them."""
    types = mixed_types()
    n = MIXED_N
    tid = (np.arange(n) % 3).astype(np.uint8)
    rad = np.array([np.float32(t.collision_sphere) for t in types])[tid]
    rng = np.random.default_rng(103)
    pos32 = f32(np.stack([rng.uniform(-6, 6, n), rng.uniform(-5, 5, n), rng.uniform(0.5, 2.5, n)], 1))

    def draw_prev(rng, idx):
        return f32(pos32[idx].astype(np.float64) - rng.uniform(0.0, MIXED_TRAVEL, (len(idx), 1)) * directions(rng, len(idx)))
    prev32, redrawn = settle_chords(rng, pos32, draw_prev, rad, MIXED_MARGIN, MIXED_SAG, MIXED_TRAVEL)
    ref = sweep_pairs_brute(prev32, pos32, rad, MIXED_MARGIN, MIXED_SAG, MIXED_TRAVEL)
    return dict(types=types, tid=tid, pos=pos32, prev=prev32, rad=rad, margin=MIXED_MARGIN, sag=MIXED_SAG, travel=MIXED_TRAVEL,
                ref=ref, redrawn=redrawn)


UNSWEPT_N, UNSWEPT_MARGIN, UNSWEPT_TRAVEL = 300, 0.5, 0.2


@functools.lru_cache(maxsize=None)
def case_unswept():
    """GPU case 4: 300 drones, two in three robobees and one in three without a sphere, in an 8 x 6 x 1.5 m box.  Drones 0 .. 39 have
    chords of 1.5 to 3 travel, 40 .. 44 a NaN or an infinity in prev, 45 a NaN in its position; 0, 3, ... have R = 0."""
    from dronesim_amd import params
    ghost = params.builtin_type("robobee")
    ghost.name, ghost.collision_sphere = "ghost", 0.0
    types = [params.builtin_type("robobee"), ghost]
    n, travel = UNSWEPT_N, UNSWEPT_TRAVEL
    tid = (np.arange(n) % 3 == 0).astype(np.uint8)
    rad = np.array([np.float32(t.collision_sphere) for t in types])[tid]
    rng = np.random.default_rng(107)
    pos32 = f32(np.stack([rng.uniform(-4, 4, n), rng.uniform(-3, 3, n), rng.uniform(0.5, 2.0, n)], 1))

    def draw_prev(rng, idx):
        length = np.where(idx < 40, rng.uniform(1.5 * travel, 3.0 * travel, len(idx)), rng.uniform(0.0, travel, len(idx)))
        p = f32(pos32[idx].astype(np.float64) - length[:, None] * directions(rng, len(idx)))
        for k, j in enumerate(idx):
            if 40 <= j < 45:
                p[k, j % 3] = [np.nan, np.inf, -np.inf, np.nan, np.inf][j - 40]
        return p
    prev32, redrawn = settle_chords(rng, pos32, draw_prev, rad, UNSWEPT_MARGIN, 0.0, travel)
    pos32 = pos32.copy()
    pos32[45, 1] = np.nan
    ref = sweep_pairs_brute(prev32, pos32, rad, UNSWEPT_MARGIN, 0.0, travel)
    return dict(types=types, tid=tid, pos=pos32, prev=prev32, rad=rad, margin=UNSWEPT_MARGIN, sag=0.0, travel=travel, ref=ref,
                redrawn=redrawn, box=(-4.5, -3.5, 4.5, 3.5))


def line_case(n=257):
    """GPU case 1's n = 257: robobees on a line 0.3 m apart (every neighbour in reach of margin 0.5), each moved 0.1 m along +x or -x
    in turn, so that neighbours close in to 0.1 m inside the step: a second tile of 256 holds one lane."""
    k = np.arange(n)
    pos = np.stack([0.3 * k, np.zeros(n), np.ones(n)], 1)
    prev = pos.copy()
    prev[:, 0] += np.where(k % 2 == 0, 0.1, -0.1)                   # evens came from the right, odds from the left
    return f32(prev), f32(pos)


def small_cases():
    """GPU case 1's pairs of robobees, name -> (prev [2, 3], pos [2, 3], travel): the swap, the same velocity on both (Delta = 0),
    one drone static, and minima attained at s = 0 (flying apart), at s = 1 (closing in) and inside."""
    return {
        "swap": (SWAP_PREV, SWAP_POS, SWAP_TRAVEL),
        "same velocity": (np.array([[0.0, 0.0, 1.0], [0.25, 0.1, 1.1]]), np.array([[0.6, 0.3, 1.2], [0.85, 0.4, 1.3]]), 1.1),
        "one static": (np.array([[2.0, 1.0, 1.0], [1.5, 1.2, 1.0]]), np.array([[2.0, 1.0, 1.0], [2.5, 0.9, 1.0]]), 1.1),
        "apart": (np.array([[0.0, 0.0, 1.0], [0.2, 0.0, 1.0]]), np.array([[-0.3, 0.0, 1.0], [0.5, 0.1, 1.0]]), 0.5),
        "closing": (np.array([[-0.4, 0.0, 1.0], [0.6, 0.1, 1.0]]), np.array([[-0.1, 0.0, 1.0], [0.3, 0.0, 1.0]]), 0.5),
        "inside": (np.array([[-0.3, 0.0, 1.0], [0.0, 0.3, 1.0]]), np.array([[0.3, 0.0, 1.0], [0.0, -0.3, 1.1]]), 0.7),
    }


def designed_inputs():
    """Every designed input of the GPU cases, as (name, prev32, pos32, radius, margin, sag, travel): what RESTATED_WORST is measured on."""
    from dronesim_amd import params
    R = np.float32(params.builtin_type("robobee").collision_sphere)
    for name, (prev, pos, travel) in small_cases().items():
        yield name, f32(prev), f32(pos), np.full(2, R), SWAP_MARGIN, 0.0, travel
    prev, pos = line_case()
    yield "line", prev, pos, np.full(len(pos), R), SWAP_MARGIN, 0.0, 0.3
    for name, d in (("crowded", case_crowded()), ("mixed", case_mixed()), ("unswept", case_unswept())):
        yield name, d["prev"], d["pos"], d["rad"], d["margin"], d["sag"], d["travel"]


# ---- the flown case (GPU case 6) ----------------------------------------------------------------------------------------------------
DROP_N, DROP_STEPS, DROP_SPEED, DROP_TRAVEL, DROP_MARGIN = 32, 24, 8.0, 0.4, 0.5
DROP_DT = 5 / 240


def drop_fleet():
    """A row of 32 tellos at z = 6 m, 1 m apart, and a column of 32 right above them, 2 m higher (staggered over one step's fall, so that
    the samples meet the passing pairs in every phase), with DROP_SPEED m/s downwards: (xyz [64, 3], vel [64, 3])."""
    k = np.arange(DROP_N)
    row = np.stack([1.0 * k, np.zeros(DROP_N), np.full(DROP_N, 6.0)], 1)
    col = row + np.stack([np.zeros(DROP_N), np.zeros(DROP_N), 2.0 + DROP_SPEED * DROP_DT * k / DROP_N], 1)
    vel = np.zeros((2 * DROP_N, 3))
    vel[DROP_N:, 2] = -DROP_SPEED
    return np.concatenate([row, col]), vel


def drop_model(radius, sag, accel):
    """The flight on paper: the row stands, the column falls from DROP_SPEED with `accel`.  (pairs x steps the swept query counts,
    pairs x steps the samples count), from sweep_pairs_brute on the modelled states."""
    xyz, vel = drop_fleet()
    rad = np.full(2 * DROP_N, np.float32(radius))
    swept = point = 0
    state = lambda t: xyz + vel * t + np.array([0.0, 0.0, -0.5 * accel * t * t]) * (vel[:, 2:3] != 0)
    for s in range(DROP_STEPS):
        a, b = f32(state(s * DROP_DT)), f32(state((s + 1) * DROP_DT))
        swept += sweep_pairs_brute(a, b, rad, DROP_MARGIN, sag, 10.0)[3]
        point += sweep_pairs_brute(b, b, rad, DROP_MARGIN, 0.0, 10.0)[3]
    return swept, point
