"""Min-snap at given segment times in arithmetic that does not care about conditioning.  TEST INFRASTRUCTURE: the product never
imports it.

Not the block sweep of trajgen_ref.py at a higher precision: the derivatives 1-4 at ALL interior waypoints are one unknown vector x
per axis, the cost sum_m e_m^T M e_m / T_m^7 (M: trajgen_ref.exact_tables(), exact rationals; e_m the scaled end values of segment
m, linear in x) is written out as one dense quadratic x^T H x + 2 g^T x + c, and H x = -g is solved by dense elimination; the
coefficients are then A^^-1 e_m.  The arithmetic is mpmath's at DIGITS decimal digits, or exact fractions.Fraction where mpmath is
not importable (every input is an fp64 number, so a rational: that route is exact and slower).

solve() returns the coefficients in the bank's convention ([n_seg * 10, 3], ascending powers of the time since the segment's
start), rounded ONCE to fp64, and the cost.  sample_fixed() samples a fixed number of points per segment (trajgen_ref.sample's
fixed rate gives a 5 ms leg one sample)."""
from fractions import Fraction

import numpy as np

from tests import trajgen_ref as R

try:
    import mpmath
    HAVE_MPMATH = True
except ImportError:                                   # pragma: no cover
    mpmath = None
    HAVE_MPMATH = False

DIGITS = 120
ORDER = R.ORDER
POINTS = 33                                           # samples per segment, both ends included


def _num(v):
    """An fp64 number or a Fraction in the working arithmetic, exactly (mpmath: to DIGITS digits for a Fraction)."""
    if HAVE_MPMATH:
        if isinstance(v, Fraction):
            return mpmath.mpf(v.numerator) / mpmath.mpf(v.denominator)
        return mpmath.mpf(float(v))
    return v if isinstance(v, Fraction) else Fraction(float(v))


def _context():
    if HAVE_MPMATH:
        return mpmath.workdps(DIGITS)
    import contextlib
    return contextlib.nullcontext()


def _solve_spd(H, G):
    """H X = G for symmetric positive definite H (list of lists) and G [N][k], by elimination without pivoting."""
    N = len(H)
    A = [H[i][:] + G[i][:] for i in range(N)]
    for c in range(N):
        piv = A[c][c]
        for r in range(c + 1, N):
            if A[r][c] != 0:
                f = A[r][c] / piv
                A[r] = [a - f * b if j >= c else a for j, (a, b) in enumerate(zip(A[r], A[c]))]
    k = len(G[0]) if N else 0
    X = [[None] * k for _ in range(N)]
    for r in range(N - 1, -1, -1):
        for j in range(k):
            s = A[r][N + j]
            for c in range(r + 1, N):
                s = s - A[r][c] * X[c][j]
            X[r][j] = s / A[r][r]
    return X


class Exact:
    """What solve_hp() returns, all in the working arithmetic: n, T [n], wp [n+1][3], der [n+1][4][3] (derivatives 1-4 at every
    waypoint, zero at both ends), coeffs [n][10][3], cost, and grad [4 (n-1)][3] (the cost's gradient in the interior derivatives at
    the solution, with grad_scale [4 (n-1)][3]: the sum of the magnitudes of the terms it is the sum of)."""


def _end_values(n, T, wp, der, m, x):
    """Scaled end values e^ of p - wp[m] on segment m, axis x."""
    e = [0] * ORDER
    e[5] = wp[m + 1][x] - wp[m][x]
    u = T[m]
    for r in range(4):
        e[1 + r] = der[m][r][x] * u
        e[6 + r] = der[m + 1][r][x] * u
        u = u * T[m]
    return e


def solve_hp(waypoints, T):
    """The min-snap course through ``waypoints`` [L, 3] with segment times ``T`` [L - 1] (fp64 numbers, taken exactly)."""
    with _context():
        Ainv_q, M_q = R.exact_tables()
        M = [[_num(v) for v in row] for row in M_q]
        Ainv = [[_num(v) for v in row] for row in Ainv_q]
        wp = [[_num(v) for v in p] for p in np.asarray(waypoints, dtype=np.float64)]
        T = [_num(t) for t in np.asarray(T, dtype=np.float64)]
        n = len(T)
        N = 4 * (n - 1)
        zero = _num(0.0)
        H = [[zero] * N for _ in range(N)]
        G = [[zero] * 3 for _ in range(N)]
        for m in range(n):
            i7 = 1 / T[m] ** 7
            u = [T[m] ** (r + 1) for r in range(4)]
            # unknown index and scale of the end values 1-4 (start) and 6-9 (end) of this segment; None: at rest
            idx = {}
            for r in range(4):
                if m >= 1:
                    idx[1 + r] = (4 * (m - 1) + r, u[r])
                if m < n - 1:
                    idx[6 + r] = (4 * m + r, u[r])
            d = [wp[m + 1][x] - wp[m][x] for x in range(3)]
            for p, (ip, sp) in idx.items():
                for q, (iq, sq) in idx.items():
                    H[ip][iq] = H[ip][iq] + M[p][q] * sp * sq * i7
                for x in range(3):
                    G[ip][x] = G[ip][x] - M[p][5] * sp * d[x] * i7
        X = _solve_spd(H, G) if N else []
        der = [[[zero] * 3 for _ in range(4)] for _ in range(n + 1)]
        for i in range(N):
            der[i // 4 + 1][i % 4] = X[i]
        out = Exact()
        out.n, out.T, out.wp, out.der = n, T, wp, der
        out.coeffs, out.cost = [], zero
        grad = [[zero] * 3 for _ in range(N)]
        scale = [[zero] * 3 for _ in range(N)]
        for m in range(n):
            i7 = 1 / T[m] ** 7
            seg = [[None] * 3 for _ in range(ORDER)]
            for x in range(3):
                e = _end_values(n, T, wp, der, m, x)
                Me = [sum((M[p][q] * e[q] for q in range(ORDER)), zero) for p in range(ORDER)]
                out.cost = out.cost + sum((e[p] * Me[p] for p in range(ORDER)), zero) * i7
                for r in range(4):
                    for p, i, free in ((1 + r, 4 * (m - 1) + r, m >= 1), (6 + r, 4 * m + r, m < n - 1)):
                        if free:
                            s = T[m] ** (r + 1) * i7 * 2
                            grad[i][x] = grad[i][x] + Me[p] * s
                            scale[i][x] = scale[i][x] + sum((abs(M[p][q] * e[q]) for q in range(ORDER)), zero) * s
                for j in range(ORDER):
                    c = sum((Ainv[j][q] * e[q] for q in range(ORDER)), zero) / T[m] ** j
                    seg[j][x] = c + wp[m][x] if j == 0 else c
            out.coeffs.append(seg)
        out.grad, out.grad_scale = grad, scale
        return out


def solve(waypoints, T):
    """(coeffs [n_seg * 10, 3] fp64 — the exact coefficients rounded once —, cost fp64)."""
    with _context():
        s = solve_hp(waypoints, T)
        co = np.array([[[float(v) for v in row] for row in seg] for seg in s.coeffs]).reshape(s.n * ORDER, 3)
        return co, float(s.cost)


def sample_fixed(coeffs, T, points=POINTS):
    """pos / vel / acc [3][n_seg * points, 3]: every segment at ``points`` equally spaced times from its start to its end, fp64,
    by Horner's rule element by element (no library matrix product: the same bits everywhere)."""
    coeffs, T = np.asarray(coeffs, dtype=np.float64), np.asarray(T, dtype=np.float64)
    out = [[], [], []]
    for m in range(len(T)):
        t = (T[m] * (np.arange(points) / (points - 1)))[:, None]
        c = coeffs[m * ORDER:(m + 1) * ORDER]
        for k in range(3):
            f = [float(np.prod(np.arange(j - k + 1, j + 1))) for j in range(k, ORDER)]      # j (j-1) .. (j-k+1)
            acc = np.zeros((points, 3))
            for j in range(ORDER - 1, k - 1, -1):
                acc = acc * t + c[j] * f[j - k]
            out[k].append(acc)
    return [np.concatenate(o, 0) for o in out]


def worst_relative(coeffs, ref_coeffs, T):
    """Worst |sample - reference sample| of pos / vel / acc over sample_fixed's points, each relative to the reference's largest
    magnitude of that quantity.  NaN or inf in ``coeffs`` gives inf."""
    a, b = sample_fixed(coeffs, T), sample_fixed(ref_coeffs, T)
    out = []
    for x, y in zip(a, b):
        d = np.abs(x - y).max() / np.abs(y).max()
        out.append(float(d) if np.isfinite(x).all() else float("inf"))
    return out


# ---- the course list of tests/golden/trajgen_exact.npz (make_goldens_trajgen_exact.py) ------------------------------------------
SEED = 20250317
FAMILIES = ("long-short-long", "short-long-short", "long-short", "short-long", "alternating", "one short leg", "ramp",
            "uniform", "far from the origin", "collinear", "there and back", "given times", "reference fixture")
RATIOS = (1.0, 10.0, 30.0, 100.0, 300.0, 1e3, 1e4, 1e5)
L_MAX = 9


def _legs(family, r):
    lo, hi = 3.0 / np.sqrt(r), 3.0 * np.sqrt(r)
    if family == 0:
        return [hi, lo, hi]
    if family == 1:
        return [lo, hi, lo]
    if family == 2:
        return [hi, lo]
    if family == 3:
        return [lo, hi]
    if family == 4:
        return [hi, lo] * 4
    if family == 5:
        return [hi] * 4 + [lo] + [hi] * 3
    return [3.0 * r ** (i / 7.0 - 0.5) for i in range(8)]


def _walk(rng, legs, start=(0.0, 0.0, 6.0)):
    """Waypoints from leg lengths: a seeded direction per leg."""
    v = rng.normal(size=(len(legs), 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return np.concatenate([[np.zeros(3)], np.cumsum(v * np.asarray(legs)[:, None], axis=0)], 0) + np.asarray(start)


def seeded_courses():
    """[dict(waypoints [L, 3], T [L - 1], max_vel, tmin (T is Tmin of max_vel, bit for bit), family, ratio)]: the seeded part of the
    list (the 16 courses of trajgen_courses.npz at the reference's own TS follow it in the fixture)."""
    rng = np.random.default_rng(SEED)
    out = []

    def add(wp, max_vel, family, ratio, T=None):
        wp = np.asarray(wp, dtype=np.float64)
        out.append(dict(waypoints=wp, T=R.tmin(wp, max_vel) if T is None else np.asarray(T, dtype=np.float64), max_vel=float(max_vel),
                        tmin=T is None, family=family, ratio=float(ratio)))
    for family in range(7):
        for r in RATIOS:
            for seed in range(2):
                add(_walk(rng, _legs(family, r)), 2.0, family, r)
    for leg in (1e-3, 1.0, 1e4):
        for max_vel in (0.01, 2.0, 100.0):
            add(_walk(rng, [leg] * 4), max_vel, 7, 1.0)
    add(np.cumsum(rng.uniform(-3.0, 3.0, (6, 3)), axis=0) + 1e6, 2.0, 8, 1.0)
    along = rng.normal(size=3)
    along /= np.linalg.norm(along)
    add(np.array([0.0, 2.0, 3.5, 7.0, 8.0])[:, None] * along + np.array([0.0, 0.0, 6.0]), 2.0, 9, 1.0)
    add(np.array([0.0, 3.0, 0.5, 2.5, -1.0, 2.0])[:, None] * along + np.array([0.0, 0.0, 6.0]), 2.0, 10, 1.0)
    add(_walk(rng, [3.0, 30.0, 3.0]), 2.0, 11, 1.0, T=[1.5, 1.5, 1.5])                   # a long leg given a short time
    add(_walk(rng, [3.0, 3.0, 3.0]), 2.0, 11, 10.0, T=[1.5, 0.15, 1.5])
    return out


def load_exact(golden_dir):
    """tests/golden/trajgen_exact.npz as a list of dicts: waypoints, T, max_vel, tmin, family, ratio, coeffs (the exact ones
    rounded once), cost."""
    import os
    g = np.load(os.path.join(golden_dir, "trajgen_exact.npz"))
    out = []
    for c in range(len(g["n_wp"])):
        L = int(g["n_wp"][c])
        out.append(dict(waypoints=g["waypoints"][c, :L], T=g["T"][c, :L - 1], max_vel=float(g["max_vel"][c]), tmin=bool(g["tmin"][c]),
                        family=int(g["family"][c]), ratio=float(g["ratio"][c]), coeffs=g["coeffs"][c, :(L - 1) * ORDER],
                        cost=float(g["cost"][c])))
    return out
