"""The trajectory bank on the CPU: tests/trajgen_ref.py — the numpy fp64 restatement of what dsim_trajgen does on the device —
against the reference's own trajGenerator outputs (tests/golden/trajgen_courses.npz, written by make_goldens_trajgen.py), the
library's constant tables against exact rationals, and the new structs and symbols of the C-ABI.  tests/README_trajgen.md."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as graft
from tests import trajgen_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Worst |restated - reference| of sampled pos / vel / acc (96 Hz over every segment, each relative to the course's largest magnitude
# of that quantity), over the 16 fixture courses at the reference's own T.  MEASURED: 3.145e-8, on acceleration of the
# L = 6, (max_vel 5, gamma 100) course; position 2.2e-9 and velocity 1.5e-8 on the same course, every other course below 2.2e-9.
# The reference inverts a matrix of condition 3e6 .. 1e8 (trajGen.py:51); the structured route never forms it.  The GPU tests
# allow 4 x this (the project's convention, tests/README_camera.md).
TRAJGEN_RESTATED_WORST = 3.2e-8


@pytest.fixture(scope="module")
def courses(golden_dir):
    return R.load_courses(golden_dir)


def test_fixture_is_the_sixteen_courses(courses):
    assert len(courses) == 16
    assert [len(c["waypoints"]) for c in courses] == [2] * 3 + [3] * 3 + [4] * 3 + [6] * 3 + [8] * 3 + [3]
    assert [(c["max_vel"], c["gamma"]) for c in courses] == [(0.7, 1e6), (2.0, 1e3), (5.0, 100.0)] * 5 + [(0.7, 1e6)]
    np.testing.assert_array_equal(courses[15]["waypoints"], [[-3, 0, 2], [0.5, 1, 5], [3, 0, 2]])
    for c in courses:
        L = len(c["waypoints"])
        assert c["coeffs"].shape == ((L - 1) * 10, 3) and c["TS"].shape == (L,) and c["TS"][0] == 0.0
        assert (np.diff(c["TS"]) >= c["Tmin"] * (1 - 1e-12)).all()
        np.testing.assert_array_equal(c["Tmin"], R.tmin(c["waypoints"], c["max_vel"]))


def test_restated_minimize_snap_against_the_reference(courses):
    """The structured solve at the reference's T: sampled trajectories within TRAJGEN_RESTATED_WORST of the reference's coeffs (and
    that below 1e-7: above it the route would be wrong, not the tolerance), cost within 1e-9 relative of the reference's."""
    worst = 0.0
    for k, c in enumerate(courses):
        T = np.diff(c["TS"])
        coeffs, cost = R.minimize_snap(c["waypoints"], T)
        w = R.worst_relative(coeffs, c["coeffs"], c["TS"])
        print(f"course {k} (L {len(T) + 1}, max_vel {c['max_vel']}, gamma {c['gamma']:g}): pos {w[0]:.2e} vel {w[1]:.2e} acc {w[2]:.2e}; "
              f"cost/ref - 1 {cost / c['cost'] - 1:+.2e}, sweep's {R.snap_cost(c['waypoints'], T) / c['cost'] - 1:+.2e}")
        worst = max(worst, max(w))
        assert abs(cost / c["cost"] - 1) <= 1e-9, k
        assert abs(R.snap_cost(c["waypoints"], T) / c["cost"] - 1) <= 1e-9, k       # the J of the search and of the GPU tests
    print(f"worst {worst:.4e}")
    assert TRAJGEN_RESTATED_WORST < 1e-7
    assert worst <= TRAJGEN_RESTATED_WORST


def test_restated_search_reaches_the_references_cost(courses):
    """J <= J_ref (1 + 1e-6) with T >= Tmin on every course.  A condition, not a measurement: COBYLA's stopping radius on the flat
    minimum is worth about 1e-9 in J; a search stuck at Tmin misses by orders of magnitude on the (5, 100) courses — checked here."""
    stuck = []
    for k, c in enumerate(courses):
        wp, ga = c["waypoints"], c["gamma"]
        T, evals = R.search(wp, c["max_vel"], ga)
        Jd, Jr = R.J(wp, T, ga), R.J(wp, np.diff(c["TS"]), ga)
        print(f"course {k}: J/J_ref - 1 {Jd / Jr - 1:+.2e} in {evals} evaluations")
        assert (T >= c["Tmin"]).all() and evals <= 2000, k
        assert Jd <= Jr * (1 + 1e-6), k
        if c["max_vel"] == 5.0:
            stuck.append(R.J(wp, c["Tmin"], ga) / Jr - 1)
    assert min(stuck) > 1e-3, stuck
    wp = courses[14]["waypoints"]
    T1, e1 = R.search(wp, 5.0, 100.0, max_evals=1)
    np.testing.assert_array_equal(T1, courses[14]["Tmin"])
    assert e1 == 1
    T7, e7 = R.search(wp, 5.0, 100.0, max_evals=7)
    assert e7 == 7


def test_two_waypoints_is_the_closed_form(courses):
    """L = 2 (the reference's unkns == 0 branch): rest to rest, the coefficients are the step times A^^-1's column of the end value."""
    Ainv, _ = R.tables()
    for c in courses[:3]:
        T = np.diff(c["TS"])[0]
        coeffs, _ = R.minimize_snap(c["waypoints"], [T])
        d = c["waypoints"][1] - c["waypoints"][0]
        want = np.outer(Ainv[:, 5] / T ** np.arange(10), d)
        want[0] = c["waypoints"][0]
        np.testing.assert_allclose(coeffs, want, rtol=1e-15, atol=0)


def test_library_tables_are_the_exact_rationals():
    """dsim_trajgen_tables.h holds exact_tables() rounded once: A^^-1 is the inverse of the Hermite matrix, M is symmetric and costs a
    constant nothing; factor_table() rounded once: F^T F = M to the bits its square roots were taken to; and the committed header is
    what tools/gen_trajgen_tables.py writes."""
    from fractions import Fraction
    Ainv, M = R.exact_tables()
    for i in range(10):
        for j in range(10):
            assert M[i][j] == M[j][i]
    for r in range(10):
        assert M[r][0] + M[r][5] == 0                       # a constant position has no snap
        if r >= 5:
            assert Ainv[r][0] + Ainv[r][5] == 0
    assert [Ainv[k][k] for k in range(5)] == [Fraction(1, f) for f in (1, 1, 2, 6, 24)]
    txt = open(os.path.join(ROOT, "dronesim_amd", "csrc", "dsim_trajgen_tables.h")).read()
    got = [float.fromhex(h) for h in re.findall(r"-?0x[0-9a-f.]+p[+-]?\d+", txt)]
    F = R.factor_table()
    assert len(F) == 6 and all(len(row) == 10 for row in F)
    for i in range(10):
        for j in range(10):
            FtF = sum(F[k][i] * F[k][j] for k in range(6))
            assert abs(FtF - M[i][j]) <= Fraction(1, 2 ** (R.FACTOR_BITS - 40)) * max(abs(M[i][i]), abs(M[j][j])), (i, j)
    want = [float(v) for t in (Ainv, M, F) for row in t for v in row]
    assert got == want
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_trajgen_tables", os.path.join(ROOT, "tools", "gen_trajgen_tables.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.render() == txt


@pytest.fixture(scope="module")
def nat():
    graft.build()
    from dronesim_amd import _native
    return _native


def test_new_symbols_and_struct_sizes(nat, tmp_path):
    """dsim_trajgen, dsim_trajgen_workspace, dsim_traj_sample_bank are declared, bound and exported; dsim_traj_bank and
    dsim_trajgen_args have the C compiler's size and offsets (a plain-C translation unit, as tests/test_abi_cpu.py does); the
    constants agree; the ABI numbers stand."""
    hdr = open(os.path.join(ROOT, "include", "dronesim_amd.h")).read()
    lib = nat.load()
    for sym in ("dsim_trajgen", "dsim_trajgen_workspace", "dsim_traj_sample_bank"):
        assert sym in nat.EXPORTS and getattr(lib, sym) is not None
        assert re.search(r"^\s*(?:int|int64_t)\s+" + sym + r"\s*\(", hdr, flags=re.M)
    assert lib.dsim_abi_version() == 11 and lib.dsim_abi_minor() == 1
    mirrors = {"dsim_traj_bank": nat.TrajBank, "dsim_trajgen_args": nat.TrajGenArgs}
    consts = {"DSIM_TRAJGEN_GIVEN": nat.TRAJGEN_GIVEN, "DSIM_TRAJGEN_TMIN": nat.TRAJGEN_TMIN, "DSIM_TRAJGEN_OPTIMIZE": nat.TRAJGEN_OPTIMIZE,
              "DSIM_TRAJGEN_LMAX": nat.TRAJGEN_LMAX, "DSIM_TRAJGEN_BAD_COUNT": nat.TRAJGEN_BAD_COUNT,
              "DSIM_TRAJGEN_BAD_WAYPOINT": nat.TRAJGEN_BAD_WAYPOINT, "DSIM_TRAJGEN_BAD_SEGMENT": nat.TRAJGEN_BAD_SEGMENT,
              "DSIM_TRAJGEN_BAD_TIME": nat.TRAJGEN_BAD_TIME, "DSIM_TRAJGEN_BAD_CONDITION": nat.TRAJGEN_BAD_CONDITION}
    lines = [f'printf("{c} %d\\n", (int){c});' for c in consts]
    for cname, cls in mirrors.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dronesim_amd.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    for c, v in consts.items():
        assert int(got[c]) == v, c
    for cname, cls in mirrors.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, (cname, fname)
    # the workspace rule needs no device: 38 fp64 per interior waypoint and course (the square-root sweep keeps R_a, R_ab and z_a)
    assert nat.TRAJGEN_BAD_CONDITION == 5
    assert lib.dsim_trajgen_workspace(64, 2) == 0 and lib.dsim_trajgen_workspace(128, 9) == 38 * 7 * 128
    assert lib.dsim_trajgen_workspace(64, 10) == 0 and lib.dsim_trajgen_workspace(0, 4) == 0


def test_host_classes_exist():
    from dronesim_amd import fleet
    assert issubclass(fleet.BankTrajectoryTargets, fleet.Targets) and hasattr(fleet.TrajectoryBank, "coeffs_of")
