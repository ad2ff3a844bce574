#!/usr/bin/env python3
"""Generate tests/golden/trajgen_exact.npz: the min-snap courses of tests/trajgen_exact.py's list, solved by its dense
high-precision solve and rounded once to fp64, so that the GPU tests need neither mpmath nor minutes.

TEST INFRASTRUCTURE.  The list: trajgen_exact.seeded_courses() (leg-length patterns x ratios x two seeds, uniform legs from 1 mm to
10 km, a course 1e6 m from the origin, collinear waypoints, a there-and-back course, given times that are not Tmin), then the 16
courses of trajgen_courses.npz at the reference's own TS.  Numbers only, padded to L_MAX = 9 waypoints with NaN:
waypoints [C, 9, 3], n_wp [C], T [C, 8], max_vel [C], tmin [C] (T is Tmin of max_vel), family [C] (index into
trajgen_exact.FAMILIES), ratio [C], coeffs [C, 80, 3], cost [C].

Usage:  python tests/golden/make_goldens_trajgen_exact.py            (writes the fixture)
        python tests/golden/make_goldens_trajgen_exact.py --check    (exit 0 when a fresh run is bit-identical)
"""
import argparse
import os
import sys
import tempfile

import numpy as np

GOLDEN = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(GOLDEN)))

from tests import trajgen_exact as X  # noqa: E402
from tests import trajgen_ref as R  # noqa: E402

NAME = "trajgen_exact.npz"


def courses():
    cs = X.seeded_courses()
    for c in R.load_courses(GOLDEN):
        cs.append(dict(waypoints=c["waypoints"], T=np.diff(c["TS"]), max_vel=c["max_vel"], tmin=False, family=12, ratio=1.0))
    return cs


def generate(path):
    cs = courses()
    C, Lm = len(cs), X.L_MAX
    data = dict(waypoints=np.full((C, Lm, 3), np.nan), n_wp=np.zeros(C, dtype=np.int32), T=np.full((C, Lm - 1), np.nan),
                max_vel=np.zeros(C), tmin=np.zeros(C, dtype=np.bool_), family=np.zeros(C, dtype=np.int32), ratio=np.zeros(C),
                coeffs=np.full((C, (Lm - 1) * X.ORDER, 3), np.nan), cost=np.zeros(C))
    for k, c in enumerate(cs):
        L = len(c["waypoints"])
        co, cost = X.solve(c["waypoints"], c["T"])
        data["waypoints"][k, :L], data["n_wp"][k], data["T"][k, :L - 1] = c["waypoints"], L, c["T"]
        data["max_vel"][k], data["tmin"][k], data["family"][k], data["ratio"][k] = c["max_vel"], c["tmin"], c["family"], c["ratio"]
        data["coeffs"][k, :(L - 1) * X.ORDER], data["cost"][k] = co, cost
    np.savez(path, **data)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    A = ap.parse_args(argv)
    if not A.check:
        generate(os.path.join(GOLDEN, NAME))
        print("written", os.path.join(GOLDEN, NAME))
        return 0
    with tempfile.TemporaryDirectory() as tmp:
        generate(os.path.join(tmp, NAME))
        a, b = np.load(os.path.join(tmp, NAME)), np.load(os.path.join(GOLDEN, NAME))
        same = sorted(a.files) == sorted(b.files) and all(a[k].tobytes() == b[k].tobytes() and a[k].shape == b[k].shape for k in a.files)
    print("bit-identical" if same else "DIFFERS")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
