"""numpy fp64 restatement of what the device does in dsim_trajgen (dronesim_amd/csrc/dsim_traj.hip): the structured min-snap
solve, the cost J and the time search.  TEST INFRASTRUCTURE: the product never imports it.

The reference (trajGen.py:45-106) builds the dense 10 n_seg-square constraint matrix A(T), inverts it and eliminates the
4 (L - 2) free interior derivatives through R = A^-T Q A^-1.  A is block-structured: the ten coefficients of a segment are fixed
by position and derivatives 1-4 at its two ends.  In the segment's own time s = t / T, with c^_j = c_j T^j, the end values
e^ = (p, T p', .., T^4 p'''') at s = 0 and s = 1 are e^ = A^ c^ with a CONSTANT 10 x 10 Hermite matrix A^, and the reference's
c^T Q c is c^^T Q^ c^ / T^7 with the constant Q^ = Hessian([1]).  So one constant matrix M = A^^-T Q^ A^^-1 gives a segment's
cost from its end values, e^^T M e^ / T^7, and what is left is a symmetric positive definite block-tridiagonal system in the
interior derivatives (4 x 4 blocks), solved here the way the device solves it: in square-root form.  With M = F^T F (F 6 x 10,
factor_table()) the cost-so-far is |R a - s|^2 in the derivatives a at the current waypoint, R upper triangular; one sweep along
the course joins each segment's six rows to it by Householder reflections, then one sweep back.  The block Cholesky sweep the
library used before (cost-so-far as a quadratic, Schur complement K_bb - Y^T Y) is kept as minimize_snap_cholesky: it loses its
digits where a short leg follows a long one, and tests/test_trajgen_exact_cpu.py classes the courses of trajgen_exact.npz by it.

A constant position costs nothing, so each segment is solved for p(t) - wp[m]: its end values hold 0 and wp[m+1] - wp[m].

exact_tables() derives A^^-1 and M in rational arithmetic, factor_table() F; the library's table (dsim_trajgen_tables.h, written by
tools/gen_trajgen_tables.py from this function) is those numbers rounded once to fp64.
"""
from fractions import Fraction
from functools import lru_cache

import numpy as np

ORDER = 10
STEP0, STEP_END = 0.5, 1e-4          # the search's first and last relative step


@lru_cache(maxsize=None)
def exact_tables():
    """(A^^-1, M) as 10 x 10 lists of Fractions.  Row order of the end values: value and derivatives 1-4 at s = 0, then at s = 1."""
    n = ORDER

    def falling(j, k):               # j (j-1) .. (j-k+1): d^k/ds^k of s^j at s = 1
        r = 1
        for m in range(k):
            r *= (j - m)
        return r
    A = [[Fraction(0)] * n for _ in range(n)]
    for k in range(5):
        A[k][k] = Fraction(falling(k, k))
        for j in range(k, n):
            A[5 + k][j] = Fraction(falling(j, k))
    # Gauss-Jordan in Fractions
    aug = [row[:] + [Fraction(int(i == j)) for j in range(n)] for i, row in enumerate(A)]
    for c in range(n):
        p = next(r for r in range(c, n) if aug[r][c] != 0)
        aug[c], aug[p] = aug[p], aug[c]
        piv = aug[c][c]
        aug[c] = [v / piv for v in aug[c]]
        for r in range(n):
            if r != c and aug[r][c] != 0:
                f = aug[r][c]
                aug[r] = [a - f * b for a, b in zip(aug[r], aug[c])]
    Ainv = [row[n:] for row in aug]
    Q = [[Fraction(0)] * n for _ in range(n)]
    for i in range(4, n):
        for j in range(4, n):
            Q[i][j] = Fraction(2 * falling(i, 4) * falling(j, 4), i + j - 7)          # trajutils.py:24-36 at T = 1
    QA = [[sum(Q[i][k] * Ainv[k][j] for k in range(n)) for j in range(n)] for i in range(n)]
    M = [[sum(Ainv[k][i] * QA[k][j] for k in range(n)) for j in range(n)] for i in range(n)]
    return Ainv, M


@lru_cache(maxsize=None)
def tables():
    """(A^^-1, M) rounded once to fp64."""
    Ainv, M = exact_tables()
    return np.array([[float(v) for v in r] for r in Ainv]), np.array([[float(v) for v in r] for r in M])


FACTOR_BITS = 256                    # the six square roots of factor_table() are taken to this many bits, then rounded once to fp64


@lru_cache(maxsize=None)
def factor_table():
    """F, 6 x 10 as Fractions, with F^T F = M to FACTOR_BITS bits: a segment's cost is |F e^|^2 / T^7.  Q^'s non-zero 6 x 6 block is
    L D L^T in exact rationals; F = sqrt(D) L^T A^^-1[4:]: six square roots, each an integer square root at FACTOR_BITS bits."""
    from math import isqrt
    Ainv, _ = exact_tables()
    n = ORDER

    def falling(j, k):
        r = 1
        for m in range(k):
            r *= (j - m)
        return r
    Q = [[Fraction(2 * falling(i, 4) * falling(j, 4), i + j - 7) for j in range(4, n)] for i in range(4, n)]
    L = [[Fraction(int(i == j)) for j in range(6)] for i in range(6)]
    D = [Fraction(0)] * 6
    for j in range(6):
        D[j] = Q[j][j] - sum(L[j][k] * L[j][k] * D[k] for k in range(j))
        for i in range(j + 1, 6):
            L[i][j] = (Q[i][j] - sum(L[i][k] * L[j][k] * D[k] for k in range(j))) / D[j]
    F = []
    for i in range(6):
        root = Fraction(isqrt(D[i].numerator * D[i].denominator << (2 * FACTOR_BITS)), D[i].denominator << FACTOR_BITS)
        F.append([root * sum(L[k][i] * Ainv[4 + k][c] for k in range(i, 6)) for c in range(n)])
    return F


@lru_cache(maxsize=None)
def factor():
    """factor_table() rounded once to fp64: the library's DSIM_TG_F."""
    return np.array([[float(v) for v in r] for r in factor_table()])


def tmin(waypoints, max_vel):
    wp = np.asarray(waypoints, dtype=np.float64)
    return np.linalg.norm(wp[:-1] - wp[1:], axis=-1) / max_vel                       # trajGen.py:33-34


def _segment(T):
    """The blocks of one segment's cost matrix S M S / T^7 that meet (a, delta, b): derivatives at its start, the position step,
    derivatives at its end."""
    _, M = tables()
    u = T ** np.arange(1, 5)
    i7 = 1.0 / T ** 7
    a, b = slice(1, 5), slice(6, 10)
    return dict(aa=M[a, a] * np.outer(u, u) * i7, ab=M[a, b] * np.outer(u, u) * i7, bb=M[b, b] * np.outer(u, u) * i7,
                ad=M[a, 5] * u * i7, bd=M[b, 5] * u * i7, dd=M[5, 5] * i7)


def _forward_cholesky(wp, T):
    """THE PARENT'S sweep along the course (kept under a name of its own: tests/README_trajgen.md).  Returns (snap cost at the optimum, per interior waypoint the Cholesky factor L of its block
    and z = L^-1 w, for the sweep back)."""
    n = len(T)
    P, q, c = None, None, 0.0
    keep = []
    for m in range(n):
        k = _segment(T[m])
        d = wp[m + 1] - wp[m]                                                          # [3]
        if m == 0:
            P, q = k["bb"], np.outer(k["bd"], d)                                       # [4, 4], [4, 3]
            c = k["dd"] * (d @ d)
            continue
        L = np.linalg.cholesky(P + k["aa"])
        w = q + np.outer(k["ad"], d)
        z = np.linalg.solve(L, w)
        Y = np.linalg.solve(L, k["ab"])
        keep.append((L, z))
        c = c + k["dd"] * (d @ d) - np.sum(z * z)
        P = k["bb"] - Y.T @ Y
        q = np.outer(k["bd"], d) - Y.T @ z
    return c, keep


# ---- the square-root sweep: what the device does -------------------------------------------------------------------------------
# A segment's cost is |F e^|^2 / T^7, so the cost-so-far is carried as |R a - s|^2 (R upper triangular 4 x 4, s [4, 3]) and a
# segment joins it by Householder reflections: no Schur complement, no difference of nearly equal numbers.
COND_MAX = 2.0 ** 14                 # see _triangularize: the loss of digits beyond which a course is flagged (README_trajgen.md)
T9_MIN, T9_MAX = 2.0 ** -1000, 2.0 ** 1000       # T^9 must stay in here


class BadCondition(Exception):
    """DSIM_TRAJGEN_BAD_CONDITION."""


def _reflect(top, D, j, c0):
    """One Householder reflection on (top[j], D[:]) that zeroes D[:, j]; columns c0.. of the two follow.  Returns the pivot."""
    v0 = top[j, j]
    col = D[:, j].copy()
    norm = np.sqrt(v0 * v0 + np.sum(col * col))
    alpha = -norm if v0 >= 0.0 else norm
    v0 = v0 - alpha
    f = (v0 * top[j, c0:] + np.sum(col[:, None] * D[:, c0:], axis=0)) * (-1.0 / (alpha * v0))      # (no BLAS: the same bits everywhere)
    top[j, c0:] -= f * v0
    D[:, c0:] -= np.outer(col, f)
    top[j, j] = alpha
    return alpha


def _triangularize(D):
    """D [6, 4 + 3] = (columns of b | right-hand sides) -> (R [4, 4] upper, s [4, 3], the cost of the two rows left over, cond).
    cond: the largest ratio of a column's norm on entry to its pivot: what the pivot lost to the columns before it."""
    D = D.copy()
    cond = 0.0
    norms = np.sqrt(np.sum(D[:, :4] * D[:, :4], axis=0))
    for j in range(4):
        alpha = _reflect(D, D[j + 1:], j, j + 1)
        D[j + 1:, j] = 0.0
        cond = max(cond, norms[j] / abs(alpha))
    return D[:4, :4], D[:4, 4:], float(np.sum(D[4:, 4:] ** 2)), cond


def _blocks(T):
    """(F_a U w, F_d w, F_b U w): the factor's columns that meet the start derivatives, the position step and the end derivatives
    of a segment of time T; U = diag(T .. T^4), w = T^-3.5."""
    F = factor()
    u = T ** np.arange(1, 5)
    w = 1.0 / (u[2] * np.sqrt(T))
    return F[:, 1:5] * (u * w), F[:, 5] * w, F[:, 6:10] * (u * w)


def _forward(wp, T):
    """The sweep along the course.  Returns (snap cost at the optimum, per interior waypoint (R_a, R_ab, z_a) with
    R_a a = z_a - R_ab b, the largest cond of a block that a later segment went on from)."""
    n = len(T)
    Rm, s, c, worst = None, None, 0.0, 0.0
    keep = []
    for m in range(n):
        Fa, fd, Fb = _blocks(T[m])
        d = wp[m + 1] - wp[m]
        rhs = -np.outer(fd, d)                                                         # [6, 3]
        last = m == n - 1
        if m >= 1:
            top = np.concatenate([Rm, np.zeros((4, 4)), s], 1)                         # [4, 11]
            D = np.concatenate([Fa, Fb, rhs], 1)                                       # [6, 11]
            for j in range(4):
                _reflect(top, D, j, j + 1)
            keep.append((np.triu(top[:, :4]), top[:, 4:8].copy(), top[:, 8:].copy()))
            rest = D[:, 4:]
        else:
            rest = np.concatenate([Fb, rhs], 1)
        if last:
            c += float(np.sum(rest[:, 4:] ** 2))
        else:
            Rm, s, left, cond = _triangularize(rest)
            c += left
            worst = max(worst, cond)
    return c, keep, worst


def minimize_snap(waypoints, T, flag=False):
    """trajGen.MinimizeSnap (trajGen.py:45-70) as the device computes it: (coeffs [n_seg*10, 3], cost).  ``flag``: raise BadCondition
    where the device reports DSIM_TRAJGEN_BAD_CONDITION."""
    Ainv, _ = tables()
    wp, T = np.asarray(waypoints, dtype=np.float64), np.asarray(T, dtype=np.float64)
    n = len(T)
    with np.errstate(all="ignore"):
        t9 = T ** 9
        if flag and not ((t9 >= T9_MIN) & (t9 <= T9_MAX)).all():
            raise BadCondition("T^9 out of range")
        _, keep, cond = _forward(wp, T)
        if flag and not cond <= COND_MAX:
            raise BadCondition(f"cond {cond:.3g}")
        coeffs = np.zeros((n * ORDER, 3))
        b = np.zeros((4, 3))
        cost = 0.0
        for m in range(n - 1, -1, -1):
            Fa, fd, Fb = _blocks(T[m])
            d = wp[m + 1] - wp[m]
            if m >= 1:
                Ra, Rab, za = keep[m - 1]
                a = np.linalg.solve(Ra, za - Rab @ b)
            else:
                a = np.zeros((4, 3))
            res = Fa @ a + np.outer(fd, d) + Fb @ b
            cost += np.sum(res * res)
            u = T[m] ** np.arange(1, 5)
            e = np.concatenate([np.zeros((1, 3)), a * u[:, None], d[None, :], b * u[:, None]], 0)     # scaled end values [10, 3]
            ch = Ainv @ e
            ch[0] = wp[m]
            coeffs[m * ORDER:(m + 1) * ORDER] = ch / (T[m] ** np.arange(ORDER))[:, None]
            b = a
    if flag and not (np.isfinite(coeffs).all() and np.isfinite(cost)):
        raise BadCondition("not finite")
    return coeffs, cost


def snap_cost(waypoints, T):
    """min over the interior derivatives of trace(P^T Q P): what the search evaluates (one sweep, nothing stored)."""
    return _forward(np.asarray(waypoints, dtype=np.float64), np.asarray(T, dtype=np.float64))[0]


def J(waypoints, T, gamma):
    """trajGen.get_cost (trajGen.py:27-30)."""
    return snap_cost(waypoints, T) + gamma * np.sum(T)


def minimize_snap_cholesky(waypoints, T):
    """trajGen.MinimizeSnap as the library solved it BEFORE the square-root sweep: the block Cholesky sweep, whose Schur complement
    K_bb - Y^T Y loses its digits when a short leg follows a long one.  Kept as the yardstick that classes the courses of
    trajgen_exact.npz (tests/test_trajgen_exact_cpu.py).  (coeffs [n_seg*10, 3], cost)."""
    Ainv, M = tables()
    wp, T = np.asarray(waypoints, dtype=np.float64), np.asarray(T, dtype=np.float64)
    n = len(T)
    _, keep = _forward_cholesky(wp, T)
    coeffs = np.zeros((n * ORDER, 3))
    b = np.zeros((4, 3))
    cost = 0.0
    for m in range(n - 1, -1, -1):
        k = _segment(T[m])
        d = wp[m + 1] - wp[m]
        if m >= 1:
            L, z = keep[m - 1]
            a = -np.linalg.solve(L.T, z + np.linalg.solve(L, k["ab"] @ b))
        else:
            a = np.zeros((4, 3))
        u = T[m] ** np.arange(1, 5)
        e = np.concatenate([np.zeros((1, 3)), a * u[:, None], d[None, :], b * u[:, None]], 0)     # scaled end values [10, 3]
        cost += np.sum(e * (M @ e)) / T[m] ** 7
        ch = Ainv @ e
        ch[0] = wp[m]
        coeffs[m * ORDER:(m + 1) * ORDER] = ch / (T[m] ** np.arange(ORDER))[:, None]
        b = a
    return coeffs, cost


def search(waypoints, max_vel, gamma, max_evals=2000):
    """The device's time search: greedy multiplicative pattern search from T = Tmin.  Returns (T, evals)."""
    if not gamma > 0.0:
        raise ValueError("J has no minimum with gamma <= 0: the library refuses it (DSIM_E_ARG)")
    wp = np.asarray(waypoints, dtype=np.float64)
    lo = tmin(wp, max_vel)
    x = lo.copy()
    Jx = J(wp, x, gamma)
    evals, step = 1, STEP0
    while step > STEP_END and evals < max_evals:
        accepted = False
        for i in range(len(x)):
            for up in (True, False):
                yi = max(lo[i], x[i] * (1.0 + step) if up else x[i] / (1.0 + step))
                if yi == x[i] or evals >= max_evals:
                    continue
                y = x.copy()
                y[i] = yi
                Jy = J(wp, y, gamma)
                evals += 1
                if Jy < Jx:
                    x, Jx, accepted = y, Jy, True
                    break                                   # the other direction would only step back
        if not accepted:
            step *= 0.5
    return x, evals


def sample(coeffs, TS, hz=96.0):
    """pos / vel / acc [3][n_samples, 3] of every segment at ``hz`` (trajGen.py:115-120), segment by segment from its own start."""
    coeffs, TS = np.asarray(coeffs), np.asarray(TS)
    out = [[], [], []]
    j = np.arange(ORDER)
    for m in range(len(TS) - 1):
        t = np.arange(0.0, TS[m + 1] - TS[m], 1.0 / hz)
        c = coeffs[m * ORDER:(m + 1) * ORDER]
        pw = t[:, None] ** j[None, :]
        out[0].append(pw @ c)
        out[1].append((pw[:, :-1] * j[1:]) @ c[1:])
        out[2].append((pw[:, :-2] * (j[2:] * (j[2:] - 1))) @ c[2:])
    return [np.concatenate(o, 0) for o in out]


def worst_relative(coeffs, ref_coeffs, TS):
    """Worst |sample - reference sample| of pos / vel / acc, each relative to the reference's largest magnitude of that quantity."""
    a, b = sample(coeffs, TS), sample(ref_coeffs, TS)
    return [float(np.abs(x - y).max() / np.abs(y).max()) for x, y in zip(a, b)]


def load_courses(golden_dir):
    """tests/golden/trajgen_courses.npz (make_goldens_trajgen.py) as a list of dicts: waypoints, max_vel, gamma, Tmin, TS, coeffs,
    cost — the reference's own fp64 outputs."""
    import os
    g = np.load(os.path.join(golden_dir, "trajgen_courses.npz"))
    keys = ("waypoints", "max_vel", "gamma", "Tmin", "TS", "coeffs", "cost")
    return [{k: (g[f"c{c}_{k}"] if g[f"c{c}_{k}"].ndim else float(g[f"c{c}_{k}"])) for k in keys} for c in range(int(g["n_courses"]))]
