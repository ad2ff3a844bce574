#!/usr/bin/env python3
"""Generate tests/golden/trajgen_courses.npz by RUNNING the reference's trajGenerator (dronesim/utils/trajGen.py, imported
unmodified from the checkout given with --reference; nothing of it is copied).

TEST INFRASTRUCTURE, beside make_goldens.py and independent of it.  The fixture holds numbers only: per course c the seeded
waypoints and what the generator made of them — c{c}_waypoints [L, 3], c{c}_max_vel, c{c}_gamma, c{c}_Tmin [L-1], c{c}_TS [L],
c{c}_coeffs [(L-1)*10, 3], c{c}_cost — and n_courses.  Courses: waypoints cumsum(uniform(-3, 3)) + (0, 0, 6), seeded, with
L in {2, 3, 4, 6, 8} x (max_vel, gamma) in {(0.7, 1e6), (2, 1e3), (5, 100)}, then the three gates of
examples/fly_INDI_TrajectoryTrack.py:127-131 at (0.7, 1e6): 16 courses.

Usage:  python tests/golden/make_goldens_trajgen.py --reference CHECKOUT            (writes the fixture)
        python tests/golden/make_goldens_trajgen.py --reference CHECKOUT --check    (exit 0 when a fresh run is bit-identical)
"""
import argparse
import os
import sys
import tempfile

import numpy as np

GOLDEN = os.path.dirname(os.path.abspath(__file__))
NAME = "trajgen_courses.npz"
SEED = 20240611
LENGTHS = (2, 3, 4, 6, 8)
SETTINGS = ((0.7, 1e6), (2.0, 1e3), (5.0, 100.0))


def courses():
    """[(waypoints, max_vel, gamma)]: seeded, in the fixture's order."""
    rng = np.random.default_rng(SEED)
    out = []
    for L in LENGTHS:
        for max_vel, gamma in SETTINGS:
            wp = np.cumsum(rng.uniform(-3.0, 3.0, (L, 3)), axis=0) + np.array([0.0, 0.0, 6.0])
            out.append((wp, max_vel, gamma))
    gates = np.vstack((np.array([[-3.0, 0, 2]]), np.array([0.5, 1, 5]), np.array([3, 0, 2])))
    out.append((gates, 0.7, 1e6))
    return out


def generate(path):
    from dronesim.utils.trajGen import trajGenerator
    data = {}
    cs = courses()
    for c, (wp, max_vel, gamma) in enumerate(cs):
        g = trajGenerator(wp.copy(), max_vel=max_vel, gamma=gamma)
        data[f"c{c}_waypoints"] = wp
        data[f"c{c}_max_vel"] = np.float64(max_vel)
        data[f"c{c}_gamma"] = np.float64(gamma)
        data[f"c{c}_Tmin"] = np.linalg.norm(wp[:-1] - wp[1:], axis=-1) / max_vel
        data[f"c{c}_TS"] = g.TS
        data[f"c{c}_coeffs"] = g.coeffs
        data[f"c{c}_cost"] = np.float64(g.cost)
    data["n_courses"] = np.int64(len(cs))
    np.savez(path, **data)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference package (the directory that holds dronesim/)")
    ap.add_argument("--check", action="store_true")
    A = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(A.reference))
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
