"""Reference of the velocity safety filter (dsim_velocity_filter): fp64 numpy, by brute force, sharing nothing with the kernel's
incremental method.  The rows are built in fp64 from the records as read back (build_rows); for a set S of rows every active set
of at most three rows of S is enumerated, u projected onto it (singular sets dropped), S is feasible when any candidate meets all
of S, its optimum the feasible candidate closest to u; the greedy drop rule is a loop over the rows around that (solve).  The
masks, the float32 restatement of the same enumeration and the generators of the GPU cases live here too, so that the CPU tests
check the caps on exactly what the GPU tests run (tests/README_filter.md)."""
import itertools

import numpy as np

ROWS, FLOOR_BIT, OBST_BIT, NB_BIT = 25, 0, 1, 9
TINY = 1e-6                  # [m] a distance at or below it gives no direction
SINGULAR = 1e-12             # Gram determinant of unit rows at or below it: no vertex
TAU, LIP = 1e-3, 8.0         # the masks: every b shifted by +-TAU [m/s]; a v that moves by more than 2 TAU LIP is a thin wedge
DECISION_CAP, VALUE_CAP = 0.005, 0.06                 # random rows
GEO_DECISION_CAP, GEO_VALUE_CAP = 0.005, 0.02         # geometric cases
# The feasibility and optimality assertions hold for ALL drones, thin wedges included, and float32 carries a row's a . v to 6e-8 |v|:
# a vertex that ran away to 40 m/s sits 1e-4 from where fp64 puts it however it is computed.  The cases keep |v_ref| <= V_CAP, twice
# the speed limit of the vehicles (whoever encodes a faster v clamps it); like the masks' caps a condition on the reference alone.
V_CAP = 16.0
F32_FIGURE = 1.33e-5         # what the float32 restatement costs outside the value mask, measured on the committed seeds (README_filter.md)
BAR = 4.0 * F32_FIGURE       # the bar of the GPU tests


def build_rows(pos, vel, u, rad, rad_of, alpha, share=0.5, buffer_drone=0.0, buffer_obstacle=0.0, floor=None, offz=None,
               nb=None, wit=None):
    """(A [n, 25, 3] unit normals, b [n, 25], valid [n, 25]) in fp64.  pos, vel, u [n, 3]; rad [n] the drones' own radii; rad_of
    [n_world] the radius of world entry j (storage order); nb = (index [k, n], dist [k, n], rel_pos [k, 3, n], rel_vel [k, 3, n]) or
    None; wit = (clearance [m, n], body [m, n], rel [m, 3, n], vel [m, 3, n] or None) or None; offz [n] or None."""
    f = lambda x: np.asarray(x, dtype=np.float64)
    pos, vel, u, rad, rad_of = f(pos), f(vel), f(u), f(rad), f(rad_of)
    n = pos.shape[0]
    A, b, valid = np.zeros((n, ROWS, 3)), np.zeros((n, ROWS)), np.zeros((n, ROWS), dtype=bool)
    oz = np.zeros(n) if offz is None else f(offz)
    with np.errstate(all="ignore"):
        if floor is not None:
            A[:, 0, 2] = 1.0
            b[:, 0] = -alpha * (pos[:, 2] - oz - float(floor) - rad)
            valid[:, 0] = True
        if wit is not None:
            clr, body, rel, wvel = wit
            clr, rel = f(clr), f(rel)
            for s in range(clr.shape[0]):
                d = clr[s] + rad
                a = -rel[s].T / d[:, None]
                vn = (a * f(wvel[s]).T).sum(1) if wvel is not None else 0.0
                A[:, OBST_BIT + s], b[:, OBST_BIT + s] = a, vn - alpha * (clr[s] - buffer_obstacle)
                valid[:, OBST_BIT + s] = (np.asarray(body[s]) >= 0) & (d > TINY)
        if nb is not None:
            index, dist, rel_pos, rel_vel = nb
            index, dist, rel_pos, rel_vel = np.asarray(index), f(dist), f(rel_pos), f(rel_vel)
            for t in range(index.shape[0]):
                ok = (index[t] >= 0) & (index[t] < n)
                a = -rel_pos[t].T / dist[t][:, None]
                h = dist[t] - (rad + rad_of[np.where(ok, index[t], 0)]) - buffer_drone
                c = (a * rel_vel[t].T).sum(1) - alpha * h
                A[:, NB_BIT + t], b[:, NB_BIT + t] = a, (a * vel).sum(1) + share * c
                valid[:, NB_BIT + t] = ok & (dist[t] > TINY)
        valid &= np.isfinite(A).all(2) & np.isfinite(b)
        sane = np.isfinite(u).all(1) & np.isfinite(pos).all(1) & np.isfinite(vel).all(1) & np.isfinite(oz)
        valid &= sane[:, None]
        A[~valid], b[~valid] = 0.0, 0.0
        # unit normals; a row without direction (0 . v >= b) stays 0 with its b
        nrm = np.linalg.norm(A, axis=2)
        has = nrm > 1e-6
        scale = np.where(has, 1.0 / np.where(has, nrm, 1.0), 1.0)
        A, b = np.where(has[:, :, None], A * scale[:, :, None], 0.0), b * scale
    return A, b, valid


def _subsets(cols):
    return [()] + [t for r in (1, 2, 3) for t in itertools.combinations(cols, r)]


def solve(A, b, valid, u, dtype=np.float64, shift=0.0, tol=None):
    """The greedy rule by brute force: (v [n, 3], dropped [n] int — bit j: row j was valid and could not be kept).  ``shift`` is
    added to every b; ``dtype`` float32 carries the same enumeration out in float32 (what float32 costs on this problem)."""
    n = A.shape[0]
    tol = (1e-12 if dtype == np.float64 else 1e-5) if tol is None else tol
    cols = [j for j in range(A.shape[1]) if valid[:, j].any()]
    A, b, u = A.astype(dtype), (b + shift).astype(dtype), np.asarray(u).astype(dtype)
    subs = _subsets(cols)
    nT = len(subs)
    M = A.shape[1]
    mem = np.zeros((nT, M), dtype=bool)
    X = np.empty((n, nT, 3), dtype=dtype)
    ok = np.ones((n, nT), dtype=bool)
    X[:, 0] = u
    at = 1
    for r in (1, 2, 3):
        T = np.array([t for t in subs if len(t) == r], dtype=np.int64).reshape(-1, r)
        if not len(T):
            continue
        mem[at + np.arange(len(T))[:, None], T] = True
        At = A[:, T]                                             # [n, nS, r, 3]
        G = At @ At.transpose(0, 1, 3, 2)
        rhs = b[:, T] - (At @ u[:, None, :, None])[..., 0]
        good = np.linalg.det(G.astype(np.float64)) > SINGULAR
        good &= valid[:, T].all(2)
        Gs = np.where(good[..., None, None], G, np.eye(r, dtype=dtype))
        lam = np.linalg.solve(Gs, rhs[..., None])[..., 0].astype(dtype)
        X[:, at:at + len(T)] = u[:, None, :] + (At.transpose(0, 1, 3, 2) @ lam[..., None])[..., 0]
        ok[:, at:at + len(T)] = good
        at += len(T)
    size = 1.0 + np.abs(X).max(2)                                          # (a far vertex meets its own rows to its own rounding)
    viol = (np.einsum("nmk,ntk->ntm", A, X) - b[:, None, :] < -tol * size[:, :, None]) & valid[:, None, :]
    # (the choice between candidates compares squared distances, which in float32 tie for two candidates 5e-4 apart along a face: the
    # restatement computes its candidates in float32 and chooses between them in fp64)
    d2 = ((X.astype(np.float64) - u[:, None, :].astype(np.float64)) ** 2).sum(2)
    n_out = np.broadcast_to(mem.sum(1)[None, :], (n, nT)).copy()          # members of T not in S yet
    n_viol = np.zeros((n, nT), dtype=np.int32)                            # rows of S the candidate violates
    dropped = np.zeros(n, dtype=np.int64)
    for j in cols:
        out2 = n_out - mem[None, :, j]
        viol2 = n_viol + viol[:, :, j]
        fits = (ok & (out2 == 0) & (viol2 == 0)).any(1)
        take = fits & valid[:, j]
        n_out = np.where(take[:, None], out2, n_out)
        n_viol = np.where(take[:, None], viol2, n_viol)
        dropped |= np.where(valid[:, j] & ~fits, 1 << j, 0)
    cand = ok & (n_out == 0) & (n_viol == 0)
    d2 = np.where(cand, d2, np.inf)
    if dtype != np.float64:
        # float32 points carry 1e-7 of error, which moves d2 by more than a step of 5e-4 along a face of the optimum costs: candidates
        # whose d2 agree to 1e-6 are a tie, and the tie goes to the first, the smallest active set (README_filter.md)
        d2 = np.where(d2 <= d2.min(1, keepdims=True) * (1.0 + 1e-6), d2.min(1, keepdims=True), d2)
    best = d2.argmin(1)
    assert cand[np.arange(n), best].all()                                 # (the empty set always fits the empty S)
    return X[np.arange(n), best], dropped


class Ref:
    """The reference of one case: v, dropped, the two masks and the rows."""

    def __init__(self, A, b, valid, u):
        self.A, self.b, self.valid, self.u = A, b, valid, np.asarray(u, dtype=np.float64)
        self.v, self.dropped = solve(A, b, valid, u)
        vp, dp = solve(A, b, valid, u, shift=TAU)
        vm, dm = solve(A, b, valid, u, shift=-TAU)
        self.decision = (dp != self.dropped) | (dm != self.dropped)
        with np.errstate(invalid="ignore"):
            self.value = self.decision | ~(np.abs(vp - vm).max(1) <= 2.0 * TAU * LIP)
        self.kept = valid & ((self.dropped[:, None] >> np.arange(A.shape[1])[None, :]) & 1 == 0)

    def shares(self):
        return float(self.decision.mean()), float(self.value.mean())

    def f32_figure(self):
        """max |v32 - v|_inf outside the value mask, and how many kept sets the float32 enumeration gets otherwise outside the
        decision mask."""
        v32, d32 = solve(self.A, self.b, self.valid, self.u, dtype=np.float32)
        same = (d32 == self.dropped) & ~self.value
        err = np.abs(v32.astype(np.float64) - self.v).max(1)
        return float(err[same].max()) if same.any() else 0.0, int(((d32 != self.dropped) & ~self.decision).sum()), err

    def check(self, v, dropped, bar=BAR, what=""):
        """The four assertions of a GPU case; returns the figures (kept-set mismatches, feasibility, optimality, position)."""
        v, dropped = np.asarray(v, dtype=np.float64), np.asarray(dropped).astype(np.int64)
        sane = np.isfinite(self.u).all(1)
        assert np.array_equal(v[~sane], self.u[~sane], equal_nan=True), what
        bad = (dropped != self.dropped) & ~self.decision
        # feasibility against the rows the KERNEL kept (outside the decision mask: the reference's)
        keptk = self.valid & ((dropped[:, None] >> np.arange(self.A.shape[1])[None, :]) & 1 == 0)
        with np.errstate(invalid="ignore"):
            slack = np.where(keptk & sane[:, None], np.einsum("nmk,nk->nm", self.A, np.nan_to_num(v)) - self.b, np.inf)
        feas = float(max(0.0, -slack.min()))
        du, dr = np.linalg.norm(v[sane] - self.u[sane], axis=1), np.linalg.norm(self.v[sane] - self.u[sane], axis=1)
        opt = float((du - dr).max()) if sane.any() else 0.0
        far = sane & ~self.value & ~bad
        pos = float(np.abs(v[far] - self.v[far]).max()) if far.any() else 0.0
        print(f"{what}: kept-set mismatches outside the decision mask {int(bad.sum())}, feasibility {feas:.3e}, optimality {opt:.3e}, "
              f"position {pos:.3e} (bar {bar:.3e}); masks {self.shares()}; changed {float((du > 0).mean()):.3f}, dropped "
              f"{float((self.dropped != 0).mean()):.3f}, |v_ref| max {float(np.abs(self.v[sane]).max()):.2f}, rows {int(self.valid.sum())}")
        assert not bad.any(), (what, np.nonzero(bad)[0][:8], dropped[bad][:8], self.dropped[bad][:8])
        assert feas <= bar, (what, feas)
        assert opt <= bar, (what, opt)
        assert pos <= bar, (what, pos)
        return int(bad.sum()), feas, opt, pos


# ---- the GPU cases' inputs: any row (a, b) through a synthesised slot ------------------------------------------------------------------
N_STD = 320                  # one full tile of 256 and a ragged one
ALPHA, SHARE, BUF_D, BUF_O = 2.0, 0.5, 0.05, 0.1
# (name, k, m, floor, b_lo, b_hi, seed).  The 9-row cases draw b as the issue's prototype did; seed 11 of the first put 6.25 % of its
# drones under the value mask, over the cap, and was changed.  At the full width those two distributions leave 82 % and 67 % of the
# drones infeasible and the masks at 2 % and 13 % at every seed (25 rows, a quarter of them violated and one in five asking for the
# impossible, b > 0): the full-width cases draw b lower, so that a drone violates as many rows as in the 9-row cases and some
# drones, not most, must drop one (README_filter.md).
RANDOM_CASES = (("k6m3", 6, 3, False, -2.0, 0.5, 12), ("k6m3", 6, 3, False, -1.5, 0.3, 12), ("full", 16, 8, True, -3.0, 0.1, 13),
                ("full", 16, 8, True, -2.0, 0.1, 14))


K_ALONE = ("k6", 6, 0, False, -2.0, 0.1, 41)       # neighbour rows alone (the edges' k > 0, m = 0 run)


def random_state(rng, n):
    """(pos, vel, u) [n, 3] float32: a loose crowd above the floor, slow, with |u| about 1.5 m/s."""
    pos = np.stack([rng.uniform(-20, 20, n), rng.uniform(-20, 20, n), rng.uniform(0.2, 3.0, n)], 1).astype(np.float32)
    vel = rng.normal(size=(n, 3)).astype(np.float32) * np.float32(0.5)
    u = (rng.normal(size=(n, 3)) * 1.5 / np.sqrt(3.0)).astype(np.float32)
    return pos, vel, u


def synth_witness(rng, a, b, rad, alpha=ALPHA, buf=BUF_O):
    """One obstacle slot per drone that gives the row (a, b): rel = -a (c + R) for a drawn clearance c, and the obstacle's velocity
    along a such that a . v_obs - alpha (c - buf) = b.  a [n, 3], b [n] -> (clearance [n], body [n], rel [3, n], vel [3, n]) float32."""
    n = len(b)
    c = rng.uniform(0.1, 1.0, n)
    rel = -(a * (c + rad)[:, None])
    vel = a * (b + alpha * (c - buf))[:, None] + np.cross(a, rng.normal(size=(n, 3))) * 0.3     # (a tangential part changes nothing)
    return c.astype(np.float32), np.zeros(n, dtype=np.int32), rel.T.astype(np.float32).copy(), vel.T.astype(np.float32).copy()


def synth_neighbor(rng, a, b, vel_i, rad, rad_of, alpha=ALPHA, share=SHARE, buf=BUF_D):
    """One neighbour slot per drone that gives the row (a, b): a drawn distance d and a drawn world entry j, rel_pos = -a d, and the
    relative velocity along a such that a . v_i + share (a . rel_vel - alpha h) = b."""
    n = len(b)
    d = rng.uniform(0.3, 2.0, n)
    j = (np.arange(n) + rng.integers(1, n, n)) % n
    h = d - (rad + rad_of[j]) - buf
    w = (b - (a * vel_i).sum(1)) / share + alpha * h
    rel_vel = a * w[:, None] + np.cross(a, rng.normal(size=(n, 3))) * 0.3
    return j.astype(np.int32), d.astype(np.float32), (-(a * d[:, None])).T.astype(np.float32).copy(), rel_vel.T.astype(np.float32).copy()


def random_case(name, k, m, floor, b_lo, b_hi, seed, n=N_STD, rad=0.1):
    """Uniformly random unit normals, b ~ U(b_lo, b_hi) in every slot (the floor's b is what the heights give)."""
    rng = np.random.default_rng(seed)
    pos, vel, u = random_state(rng, n)
    rad_n = np.full(n, np.float64(np.float32(rad)))

    def rows():
        a = rng.normal(size=(n, 3))
        return a / np.linalg.norm(a, axis=1, keepdims=True), rng.uniform(b_lo, b_hi, n)

    wit = [synth_witness(rng, *rows(), rad_n) for _ in range(m)]
    nb = [synth_neighbor(rng, *rows(), vel.astype(np.float64), rad_n, rad_n) for _ in range(k)]
    stack = lambda parts: tuple(np.stack([p[i] for p in parts]) for i in range(4))
    return dict(name=f"{name}-b{b_lo}", n=n, k=k, m=m, pos=pos, vel=vel, u=u, rad=rad_n, floor=0.0 if floor else None,
                nb=stack(nb) if k else None, wit=stack(wit) if m else None)


def case_ref(case, alpha=ALPHA, share=SHARE, buf_d=BUF_D, buf_o=BUF_O, vel=None, pos=None):
    """The Ref of a case's records (pos / vel: as the device holds them, when they were read back)."""
    pos = case["pos"] if pos is None else pos
    vel = case["vel"] if vel is None else vel
    A, b, valid = build_rows(pos, vel, case["u"], case["rad"], case.get("rad_of", case["rad"]), alpha, share, buf_d, buf_o,
                             case.get("floor"), case.get("offz"), case.get("nb"), case.get("wit"))
    return Ref(A, b, valid, case["u"])


_CACHE = {}


def random_ref(spec):
    """(case, Ref) of one of RANDOM_CASES, computed once per process."""
    if spec not in _CACHE:
        case = random_case(*spec)
        _CACHE[spec] = (case, case_ref(case))
    return _CACHE[spec]


def squeezed_case(n=N_STD, rad=0.1):
    """Drones built to be infeasible: every drone sits between two opposed obstacle rows (slots 0 and 1, +-x, both asking for more
    than the other allows) with a neighbour row across (+y); every fourth drone also has the floor pushing up against an obstacle
    row from above (slot 2, -z).  The obstacle in slot 0 wins over slot 1, both win over the neighbour where they cannot all be met,
    and the floor wins over slot 2."""
    rng = np.random.default_rng(21)
    pos, vel, u = random_state(rng, n)
    pos[:, 2] = np.where(np.arange(n) % 4 == 0, np.float32(0.5 * rad), pos[:, 2])  # below R + floor: the floor's b is positive
    rad_n = np.full(n, np.float64(np.float32(rad)))
    ex, ey, ez = np.eye(3)
    rows = [(np.tile(ex, (n, 1)), rng.uniform(0.2, 1.0, n)), (np.tile(-ex, (n, 1)), rng.uniform(0.2, 1.0, n)),
            (np.tile(-ez, (n, 1)), np.where(np.arange(n) % 4 == 0, rng.uniform(0.2, 1.0, n), -5.0))]
    wit = [synth_witness(rng, a, b, rad_n) for a, b in rows]
    # the neighbour row: across, and on every second drone tilted against slot 0 so that it cannot be met with it
    a_nb = np.where((np.arange(n) % 2 == 0)[:, None], np.tile(ey, (n, 1)), np.tile(-ex, (n, 1)))
    nb = [synth_neighbor(rng, a_nb, rng.uniform(0.2, 1.5, n), vel.astype(np.float64), rad_n, rad_n)]
    stack = lambda parts: tuple(np.stack([p[i] for p in parts]) for i in range(4))
    return dict(name="squeezed", n=n, k=1, m=3, pos=pos, vel=vel, u=u, rad=rad_n, floor=0.0, nb=stack(nb), wit=stack(wit))
