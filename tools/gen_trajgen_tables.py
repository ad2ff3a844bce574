#!/usr/bin/env python3
"""Writes dronesim_amd/csrc/dsim_trajgen_tables.h: the constant tables of dsim_trajgen, derived in rational arithmetic
(tests/trajgen_ref.py:exact_tables; factor_table, whose six square roots are taken to 256 bits) and rounded once to fp64.  tests/test_trajgen_cpu.py holds the committed header to this.

    python tools/gen_trajgen_tables.py            (rewrites the header)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.trajgen_ref import exact_tables, factor_table  # noqa: E402

OUT = os.path.join(ROOT, "dronesim_amd", "csrc", "dsim_trajgen_tables.h")


def render():
    Ainv, M = exact_tables()

    def rows(t):
        return ",\n".join("  {" + ", ".join(float(v).hex() for v in r) + "}" for r in t)
    return (
        "// dsim_trajgen_tables.h — written by tools/gen_trajgen_tables.py; do not edit.\n"
        "// End values of a degree-9 segment in its own time s = t / T: e^ = (p, T p', T^2 p'', T^3 p''', T^4 p'''') at s = 0, then at s = 1.\n"
        "// DSIM_TG_AINV: c^ = AINV e^, c^_j = c_j T^j (the inverse of the constant Hermite matrix; its entries are integers and 1 / k!).\n"
        "// DSIM_TG_M = AINV^T Q^ AINV, Q^ the reference's Hessian at T = 1 (trajutils.py:24-36): a segment's snap cost is e^^T M e^ / T^7.\n"
        "// DSIM_TG_F: 6 x 10 with F^T F = M (sqrt(D) L^T of Q^'s 6 x 6 block = L D L^T, times AINV's last six rows): the cost is |F e^|^2 / T^7.\n"
        "// Exact rationals (F: to 256 bits) rounded once to fp64, written as hexadecimal floating literals.\n"
        "#pragma once\n"
        "__constant__ const double DSIM_TG_AINV[10][10] = {\n" + rows(Ainv) + "};\n"
        "__constant__ const double DSIM_TG_M[10][10] = {\n" + rows(M) + "};\n"
        "__constant__ const double DSIM_TG_F[6][10] = {\n" + rows(factor_table()) + "};\n")


if __name__ == "__main__":
    with open(OUT, "w") as fh:
        fh.write(render())
    print("written", OUT)
