"""Min-snap courses against an exact solve, short legs beside long ones.  tests/trajgen_exact.py solves the quadratic programme densely
in high-precision arithmetic; tests/golden/trajgen_exact.npz (make_goldens_trajgen_exact.py) holds its answers for a list of courses
that reaches far outside the family of trajgen_courses.npz.  Here, on the CPU: the exact solve against itself and against the
reference, the restatement of the device's sweep (trajgen_ref.minimize_snap) and of the sweep it replaced (minimize_snap_cholesky)
against it, and the class of every course, which the GPU tests (test_gpu_trajgen_exact.py) go by.  tests/README_trajgen.md."""
import numpy as np
import pytest

from tests import trajgen_exact as X
from tests import trajgen_ref as R
from tests.test_trajgen_cpu import TRAJGEN_RESTATED_WORST

BAR = 4.0 * TRAJGEN_RESTATED_WORST          # the project's published bar for the device (tests/README_trajgen.md), unchanged

# Worst |restated - exact| of sampled pos / vel / acc (33 points per segment, each relative to the course's largest magnitude of that
# quantity) over the BENIGN courses of trajgen_exact.npz: those whose neighbouring segment times differ by a factor of 10 at most.
# MEASURED: 7.78e-12 (the three-leg course given the times 1.5, 0.15, 1.5 s; the courses of equal legs are at 1.4e-12 at most, most of which is the
# fp64 sampling of the two sets of coefficients).  It is rounding noise: another order of the sweep's sums gives 3e-12 .. 8e-12.
# The GPU tests allow the device 4 x this on the same courses.
TRAJGEN_EXACT_WORST = 8e-12


def neighbour_ratio(T):
    """The largest ratio of two neighbouring segment times."""
    T = np.asarray(T)
    return float(max([1.0] + [max(a / b, b / a) for a, b in zip(T[:-1], T[1:])]))


def _worst(fn, c):
    """Worst sampled difference of fn's course from the exact one, and the cost's relative difference; inf where fn fails."""
    try:
        with np.errstate(all="ignore"):
            co, cost = fn(c["waypoints"], c["T"])
    except np.linalg.LinAlgError:                                   # the Cholesky of a block that is not positive definite
        return float("inf"), float("inf")
    return max(X.worst_relative(co, c["coeffs"], c["T"])), abs(cost / c["cost"] - 1.0)


def classify(courses):
    """Per course "A", "B-easy" or "B-hard", from the exact solve and the sweep the library used before (minimize_snap_cholesky) alone:
    A: neighbouring T within a factor of 100 (the patterns' ratio 100 is 100 to rounding: 1e-9 of slack); B-easy: beyond, but the
    old sweep is within BAR / 4 of exact on sampled pos / vel / acc; B-hard: the rest.  And per course whether it is benign."""
    cls, benign = [], []
    for c in courses:
        nb = neighbour_ratio(c["T"])
        benign.append(nb <= 10.0 * (1 + 1e-9))
        if nb <= 100.0 * (1 + 1e-9):
            cls.append("A")
        else:
            cls.append("B-easy" if _worst(R.minimize_snap_cholesky, c)[0] <= BAR / 4 else "B-hard")
    return cls, benign


@pytest.fixture(scope="module")
def exact(golden_dir):
    return X.load_exact(golden_dir)


def test_fixture_is_the_list(exact, golden_dir):
    """The seeded list, then the 16 courses of trajgen_courses.npz at the reference's TS; T = Tmin bit for bit where the fixture says so;
    at most 128 seeded courses (one bank launch) and L <= 9."""
    seeded = X.seeded_courses()
    ref = R.load_courses(golden_dir)
    assert len(exact) == len(seeded) + 16 and len(seeded) <= 128
    assert [c["family"] for c in exact[:112]] == [f for f in range(7) for _ in range(16)]
    assert sorted(set(c["ratio"] for c in exact[:112])) == list(X.RATIOS)
    for c, s in zip(exact, seeded):
        np.testing.assert_array_equal(c["waypoints"], s["waypoints"])
        np.testing.assert_array_equal(c["T"], s["T"])
        assert c["tmin"] == s["tmin"] and c["max_vel"] == s["max_vel"] and len(c["waypoints"]) <= X.L_MAX
        if c["tmin"]:
            np.testing.assert_array_equal(c["T"], R.tmin(c["waypoints"], c["max_vel"]))
    for c, r in zip(exact[len(seeded):], ref):
        np.testing.assert_array_equal(c["waypoints"], r["waypoints"])
        np.testing.assert_array_equal(c["T"], np.diff(r["TS"]))
        assert c["family"] == 12 and not c["tmin"]
    # the patterns are what they say: long-short-long at ratio r has T in the ratio r
    assert abs(neighbour_ratio(exact[10]["T"]) / 1e3 - 1) < 1e-9 and exact[10]["family"] == 0 and exact[10]["ratio"] == 1e3


def test_fixture_is_what_its_script_writes(exact):
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_goldens_trajgen_exact.py")
    spec = importlib.util.spec_from_file_location("make_goldens_trajgen_exact", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.main(["--check"]) == 0


def test_exact_solve_against_itself(exact):
    """At the working precision, on every third course and every course of ratio 1e5: the course passes through its waypoints,
    derivatives 1-4 are continuous at interior waypoints and zero at both ends, and the cost is stationary in the interior
    derivatives — each to 1e-30 of the sum of the magnitudes of the terms involved."""
    from fractions import Fraction
    tol = X._num(Fraction(1, 10 ** 30))
    pick = [c for k, c in enumerate(exact) if k % 3 == 0 or c["ratio"] == 1e5]
    assert len(pick) >= 50
    with X._context():
        for c in pick:
            s = X.solve_hp(c["waypoints"], c["T"])
            fall = lambda j, k: X._num(float(np.prod(np.arange(j - k + 1, j + 1)))) if k else X._num(1.0)     # noqa: E731
            for m in range(s.n):
                for x in range(3):
                    co = [s.coeffs[m][j][x] for j in range(10)]
                    assert co[0] == s.wp[m][x]
                    for k in range(5):                                       # the k-th derivative at the segment's end
                        terms = [co[j] * fall(j, k) * s.T[m] ** (j - k) for j in range(k, 10)]
                        end, scale = sum(terms), sum(abs(t) for t in terms) + abs(s.wp[m + 1][x])
                        if k == 0:
                            want = s.wp[m + 1][x]
                        elif m == s.n - 1:
                            want = 0
                        else:
                            want = s.coeffs[m + 1][k][x] * fall(k, k)
                        assert abs(end - want) <= tol * scale, (m, x, k)
                    if m == 0:
                        assert co[1] == co[2] == co[3] == co[4] == 0
            for g, sc in zip(s.grad, s.grad_scale):
                for x in range(3):
                    assert abs(g[x]) <= tol * sc[x]
            co, cost = X.solve(c["waypoints"], c["T"])
            np.testing.assert_array_equal(co, c["coeffs"])
            assert cost == c["cost"]


def test_exact_solve_against_the_reference(exact, golden_dir):
    """On the 16 fixture courses the exact solve is within TRAJGEN_RESTATED_WORST of the reference's stored coefficients, in the
    metric that record was measured in (96 Hz): the new reference is tied to the old one."""
    ref = R.load_courses(golden_dir)
    worst = 0.0
    for c, r in zip(exact[-16:], ref):
        w = R.worst_relative(c["coeffs"], r["coeffs"], r["TS"])
        dc = abs(c["cost"] / r["cost"] - 1)
        print(f"L {len(r['TS'])}: pos {w[0]:.2e} vel {w[1]:.2e} acc {w[2]:.2e} cost {dc:.2e}")
        worst = max(worst, max(w))
        assert dc <= 1e-9
    print(f"worst {worst:.4e}")
    assert worst <= TRAJGEN_RESTATED_WORST


def flagged(c):
    try:
        R.minimize_snap(c["waypoints"], c["T"], flag=True)
        return False
    except R.BadCondition:
        return True


def test_restatement_against_the_exact_solve(exact):
    """The whole list: the restated sweep of the device and the Cholesky sweep it replaced, against the exact solve (the table of
    tests/README_trajgen.md).  The worst of the restatement over the benign courses is what is recorded, and the record is not padded;
    on A and B-easy courses the restatement serves the course within BAR (cost too), on B-hard it serves within BAR or flags."""
    cls, benign = classify(exact)
    worst_benign = 0.0
    for k, c in enumerate(exact):
        new, dc = _worst(R.minimize_snap, c)
        old, dco = _worst(R.minimize_snap_cholesky, c)
        fl = flagged(c)
        print(f"{k:3d} {X.FAMILIES[c['family']]:20s} ratio {c['ratio']:6g} L {len(c['T']) + 1} {cls[k]:6s} {'benign' if benign[k] else '      '} "
              f"Cholesky sweep {old:.1e} (cost {dco:.1e})  square-root sweep {new:.1e} (cost {dc:.1e}) {'FLAGGED' if fl else ''}")
        if benign[k]:
            worst_benign = max(worst_benign, new)
        if cls[k] != "B-hard":
            assert not fl and new <= BAR and dc <= BAR, k
        else:
            assert fl or (new <= BAR and dc <= BAR), k
    print(f"worst over the benign courses {worst_benign:.3e}")
    assert worst_benign <= TRAJGEN_EXACT_WORST <= 2.0 * worst_benign


def test_every_class_is_populated(exact):
    cls, benign = classify(exact)
    count = {k: cls.count(k) for k in ("A", "B-easy", "B-hard")}
    print(count, "benign", sum(benign))
    assert count["A"] >= 20 and count["B-easy"] >= 10 and count["B-hard"] >= 10
    assert sum(benign) >= 20
    # the families the issue names: long-short-long from ratio 300 on is B-hard; short-long-short and the two-leg courses B-easy
    for k, c in enumerate(exact[:112]):
        if c["ratio"] > 100:
            if c["family"] == 0:
                assert cls[k] == "B-hard", k
            if c["family"] in (1, 2, 3):
                assert cls[k] == "B-easy", k


def test_restated_refusals():
    """Segment times whose ninth power is no normal number are flagged, not served as NaN; the restated search refuses gamma <= 0."""
    wp = np.array([[0.0, 0, 1], [1, 0, 1], [1, 2, 1]])
    for T in (1e-60, 1e60):
        with pytest.raises(R.BadCondition):
            R.minimize_snap(wp, [T, T], flag=True)
    co, cost = R.minimize_snap(wp, [1e-5, 1e6], flag=False)
    assert np.isfinite(co).all() and np.isfinite(cost)
    for gamma in (0.0, -1.0):
        with pytest.raises(ValueError):
            R.search(wp, 2.0, gamma)
