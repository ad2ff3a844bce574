"""CPU-side checks of the swept obstacle watch (dsim_obstacle_sweep): the ABI surface, the arithmetic of sweep_reach / sweep_sag,
and the tests' own fp64 reference (tests/sweep_ref.py) against dense sampling of the chord.  tests/README_sweep.md."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as graft
from dronesim_amd import params
from tests.obstacle_ref import brute, tri_dist
from tests.sweep_ref import chords, seg_tri_dist, sweep_brute

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def nat():
    graft.build()
    from dronesim_amd import _native
    return _native


def _gate():
    from dronesim_amd.obstacles import ObstacleSet
    return ObstacleSet.from_urdf(os.path.join(GOLDEN, "gate_50_curved.urdf"), (0, 0, 0), (0, 0, 0))


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
def test_symbol_flags_and_struct_layout(nat, tmp_path):
    hdr = open(os.path.join(ROOT, "include", "dronesim_amd.h")).read()
    lib = nat.load()
    assert re.search(r"^int\s+dsim_obstacle_sweep\s*\(", hdr, flags=re.M)
    assert "dsim_obstacle_sweep" in nat.EXPORTS and lib.dsim_obstacle_sweep is not None
    assert lib.dsim_abi_version() == 11 and lib.dsim_abi_minor() == 1
    assert nat.SWEEP_KEEP_PREV == 1 and nat.SWEEP_PRIME == 2
    assert os.path.join(ROOT, "dronesim_amd", "csrc", "dsim_sweep.hip") in graft.HIP_DEPS and len(graft.HIP_SRCS) == 6
    fields = [f for f, _ in nat.SweepArgs._fields_]
    lines = ['printf("size %zu\\n", sizeof(dsim_sweep_args));', 'printf("keep %d\\n", (int)DSIM_SWEEP_KEEP_PREV);',
             'printf("prime %d\\n", (int)DSIM_SWEEP_PRIME);']
    lines += [f'printf("{f} %zu\\n", offsetof(dsim_sweep_args, {f}));' for f in fields]
    src = tmp_path / "sweep.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dronesim_amd.h"\nint main(void) {\n' + "\n".join(lines)
                   + "\nreturn 0; }\n")
    exe = tmp_path / "sweep"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(nat.SweepArgs)
    assert int(got["keep"]) == nat.SWEEP_KEEP_PREV and int(got["prime"]) == nat.SWEEP_PRIME
    for f in fields:
        assert int(got[f]) == getattr(nat.SweepArgs, f).offset, f
    # refused before anything is looked at: no ctx, no set, no args
    assert lib.dsim_obstacle_sweep(None, None, 1, nat.View(), None, None) == -1


# ---- host arithmetic ---------------------------------------------------------------------------------------------------------------
def test_sweep_reach_and_sag_arithmetic():
    from dronesim_amd.obstacles import sweep_reach, sweep_sag, watch_reach
    types = [params.builtin_type(k) for k in ("robobee", "tello", "hexa_6DOF")]
    r_max = max(float(np.float32(t.collision_sphere)) for t in types)
    for margin, sag, travel in ((1.0, 0.0, 0.0), (0.6, 0.01, 0.5), (0.25, 5e-4, 3.0)):
        want = np.float32((r_max + float(np.float32(sag)) + float(np.float32(margin)) + travel / 2) * (1 + 2.0 ** -10))
        got = sweep_reach(types, margin, sag, travel)
        assert got == float(want)
        # the library's own condition, half = reach - (R_max + sag + margin) >= reach / 1024, holds for any chord worth a lookup
        # (travel = 0 leaves half = reach / 1025: such a set serves the point query only)
        half = got - (r_max + float(np.float32(sag)) + float(np.float32(margin)))
        assert half >= travel / 2 and (half >= got / 1024) == (travel > 0)
    assert sweep_reach(types, 1.0, 0.0, 0.0) == watch_reach(types, 1.0)
    assert sweep_sag(9.8, 5 / 240) == 9.8 * (5 / 240) ** 2 / 8
    assert sweep_sag(0.0, 1.0) == 0.0
    # the bound is attained by the path of constant acceleration: x(t) = a t (T - t) / 2 away from its chord, at t = T / 2
    a, T = 7.0, 0.3
    t = np.linspace(0, T, 2001)
    assert abs((a * t * (T - t) / 2).max() - sweep_sag(a, T)) < 1e-12


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def test_reference_against_dense_sampling():
    s = _gate()
    rng = np.random.default_rng(71)
    q0, q1 = chords(rng, 200, [-0.55, -1.05, -0.9], [0.55, 1.05, 0.9], 0.0, 0.8)
    ref, hit = seg_tri_dist(q0, q1, s.triangles)
    ref = ref.min(1)
    w = np.linspace(0.0, 1.0, 401)
    pts = q0[:, None, :] + w[None, :, None] * (q1 - q0)[:, None, :]
    sampled = tri_dist(pts.reshape(-1, 3), s.triangles).min(1).reshape(200, 401).min(1)
    length = np.linalg.norm(q1 - q0, axis=1)
    print(f"reference vs 401 samples per chord: {int(hit.any(1).sum())} chords pierce, worst sampled - reference "
          f"{(sampled - ref).max():.3e} m, worst reference - sampled {(ref - sampled).max():.3e} m")
    assert hit.any(1).sum() >= 5
    assert np.all(ref <= sampled + 1e-12)                         # never above the sampled minimum
    assert np.all(sampled - ref <= length / 400 + 1e-12)          # and within one sample spacing of it


def test_a_chord_straight_through_the_top_bar():
    """Both ends further than R from every triangle, the chord through the bar: the chord's clearance is -R, the ends' positive."""
    s = _gate()
    t = params.builtin_type("robobee")
    R = np.float32(t.collision_sphere)
    lo, hi = s.aabb
    z = 0.5 * (float(hi[2]) + 0.19)                                # inside the top bar (the opening ends at z = 0.19)
    q0, q1 = np.array([[-0.35, 0.0, z]], dtype=np.float32), np.array([[0.35, 0.0, z]], dtype=np.float32)
    rad = np.array([R])
    ends = [brute(q, s.triangles, s.body, rad, 1.0) for q in (q0, q1)]
    assert ends[0][4][0] > 0.1 and ends[1][4][0] > 0.1 and ends[0][3] == ends[1][3] == 0
    ref = sweep_brute(q0, q1, s.triangles, s.body, rad, 1.0)
    assert ref[3] == 1 and ref[1][0] == 0 and abs(ref[4][0] + float(R)) < 1e-12
    # with a sag the sphere is that much larger
    assert abs(sweep_brute(q0, q1, s.triangles, s.body, rad, 1.0, sag=0.01)[4][0] + float(R) + float(np.float32(0.01))) < 1e-12
    # a zero-length chord is the point query
    same = sweep_brute(q1, q1, s.triangles, s.body, rad, 1.0)
    assert abs(same[4][0] - ends[1][4][0]) < 1e-12 and same[3] == 0
