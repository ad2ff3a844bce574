"""CPU-side checks of the gate passage watch (dsim_gate_passage): the ABI surface, Aperture's and the env's refusals, and the
tests' own fp64 reference (tests/passage_ref.py) against dense sampling of the chord, with the conditions on the GPU cases' inputs
and the recorded error of the float32 restatement.  tests/README_passage.md."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as graft
from tests import passage_ref as pr
from tests import scenes_ref as sr
from tests.obstacle_ref import tri_dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nat():
    graft.build()
    from dronesim_amd import _native
    return _native


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
def test_symbol_flags_and_struct_layout(nat, tmp_path):
    hdr = open(os.path.join(ROOT, "include", "dronesim_amd.h")).read()
    lib = nat.load()
    m = re.search(r"^int\s+dsim_gate_passage\s*\(([^;]*)\);", hdr, flags=re.M)
    assert m and len(m.group(1).split(",")) == 7 == len(lib.dsim_gate_passage.argtypes)
    assert "dsim_gate_passage" in nat.EXPORTS and lib.dsim_gate_passage is not None
    assert lib.dsim_abi_version() == 11 and lib.dsim_abi_minor() == 1
    assert (nat.APERTURE_RECT, nat.APERTURE_ELLIPSE, nat.GATE_WRAP) == (0, 1, 4)
    assert os.path.join(ROOT, "dronesim_amd", "csrc", "dsim_passage.hip") in graft.HIP_DEPS and len(graft.HIP_SRCS) == 6
    assert '#include "dsim_passage.hip"' in open(os.path.join(ROOT, "dronesim_amd", "csrc", "dsim_obstacles.hip")).read()
    lines = ['printf("size %zu\\n", sizeof(dsim_gate_args));', 'printf("apsize %zu\\n", sizeof(dsim_aperture));',
             'printf("wrap %d\\n", (int)DSIM_GATE_WRAP);', 'printf("rect %d\\n", (int)DSIM_APERTURE_RECT);',
             'printf("ellipse %d\\n", (int)DSIM_APERTURE_ELLIPSE);']
    fields = [f for f, _ in nat.GateArgs._fields_]
    ap_fields = [f for f, _ in nat.ApertureC._fields_]
    lines += [f'printf("{f} %zu\\n", offsetof(dsim_gate_args, {f}));' for f in fields]
    lines += [f'printf("ap_{f} %zu\\n", offsetof(dsim_aperture, {f}));' for f in ap_fields]
    src = tmp_path / "passage.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dronesim_amd.h"\nint main(void) {\n' + "\n".join(lines)
                   + "\nreturn 0; }\n")
    exe = tmp_path / "passage"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(nat.GateArgs) and int(got["apsize"]) == ctypes.sizeof(nat.ApertureC)
    assert (int(got["wrap"]), int(got["rect"]), int(got["ellipse"])) == (nat.GATE_WRAP, nat.APERTURE_RECT, nat.APERTURE_ELLIPSE)
    for f in fields:
        assert int(got[f]) == getattr(nat.GateArgs, f).offset, f
    for f in ap_fields:
        assert int(got["ap_" + f]) == getattr(nat.ApertureC, f).offset, f


def test_refusals_before_any_device_is_touched(nat):
    """No ctx: every call is refused with DSIM_E_ARG before anything is looked at, so none of these pointers is followed."""
    lib = nat.load()
    a = nat.GateArgs()
    assert lib.dsim_gate_passage(None, None, 1, nat.View(), None, None, None) == -1
    assert lib.dsim_gate_passage(None, None, 1, nat.View(), None, None, ctypes.byref(a)) == -1
    a.flags = nat.SWEEP_PRIME
    assert lib.dsim_gate_passage(None, None, 1, nat.View(), None, None, ctypes.byref(a)) == -1
    # with a stand-in ctx the argument checks are reached: still nothing is dereferenced before the refusal
    fake = ctypes.create_string_buffer(4096)
    v = nat.View()
    v.n_pad = 64
    prev = ctypes.create_string_buffer(16)
    for flags in (8, 64, nat.SWEEP_KEEP_PREV | nat.SWEEP_PRIME, nat.SWEEP_KEEP_PREV | nat.SWEEP_PRIME | nat.GATE_WRAP):
        a = nat.GateArgs()
        a.prev, a.flags = ctypes.addressof(prev), flags
        assert lib.dsim_gate_passage(fake, None, 1, v, None, None, ctypes.byref(a)) == -1, flags
    a = nat.GateArgs()
    a.flags = 0                                                         # no prev
    assert lib.dsim_gate_passage(fake, None, 1, v, None, None, ctypes.byref(a)) == -1
    a.prev = ctypes.addressof(prev)
    assert lib.dsim_gate_passage(fake, None, 1, v, None, None, ctypes.byref(a)) == -1      # no scenes, no ids, no due
    assert lib.dsim_gate_passage(fake, None, 0, v, None, None, ctypes.byref(a)) == -1      # n <= 0
    assert lib.dsim_gate_passage(fake, None, 65, v, None, None, ctypes.byref(a)) == -1     # n > n_pad


def test_aperture_validation():
    from dronesim_amd.obstacles import Aperture
    ok = dict(center=(0, 0, 0), normal=(1, 0, 0), u=(0, 1, 0), half=(0.3, 0.2))
    a = Aperture(**ok, shape="ellipse", outer=(0.3, 0.25))
    assert np.array_equal(a.v, [0, 0, 1]) and a.to_c().shape == 1 and list(a.to_c().outer) == [np.float32(0.3), np.float32(0.25)]
    assert list(Aperture(**ok).to_c().outer) == [0.0, 0.0] and Aperture(**ok).to_c().shape == 0
    s = np.sqrt(0.5)
    assert np.allclose(Aperture((1, 2, 3), (s, s, 0), (-s, s, 0), (1, 1)).v, [0, 0, 1], atol=1e-7)
    for bad in (dict(normal=(1.001, 0, 0)), dict(normal=(0, 0, 0)), dict(u=(0, 2, 0)), dict(u=(1e-3, 1, 0)), dict(u=(1, 0, 0)),
                dict(half=(0.3, 0.0)), dict(half=(-0.3, 0.2)), dict(half=(0.3,)), dict(center=(0, np.nan, 0)),
                dict(normal=(1, 0)), dict(shape="circle"), dict(outer=(0.29, 0.5)), dict(outer=(0.5, 0.1)), dict(outer=(np.inf, 1))):
        with pytest.raises(ValueError):
            Aperture(**{**ok, **bad})


def test_env_refusals():
    """All before a context is made."""
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.obstacles import ObstacleScenes
    z = np.zeros((2, 3, 3))
    s, ap = ObstacleScenes(sr.gate(), z, z), pr.gate_aperture()
    kw = dict(initial_xyzs=np.zeros((4, 3)), dict_io=False)
    ids = np.zeros(4, dtype=int)
    for lone in (dict(gate_scenes=s, obstacle_scene_id=ids), dict(gate_start=1), dict(gate_laps=True), dict(gate_travel=0.5)):
        with pytest.raises(ValueError, match="without gate_watch"):
            CtrlAviary(["tello"], 4, **lone, **kw)
    with pytest.raises(ValueError, match="gates' placements"):
        CtrlAviary(["tello"], 4, gate_watch=ap, **kw)
    with pytest.raises(ValueError, match="gates' placements"):
        CtrlAviary(["tello"], 4, gate_watch=ap, obstacle_watch=sr.gate(), **kw)        # a plain set has no placements
    for bad in ((0, 0, 0), "rect", ap.to_c()):
        with pytest.raises(ValueError, match="Aperture"):
            CtrlAviary(["tello"], 4, gate_watch=bad, gate_scenes=s, obstacle_scene_id=ids, **kw)
    with pytest.raises(ValueError, match="obstacle_scene_id .* is required"):
        CtrlAviary(["tello"], 4, gate_watch=ap, gate_scenes=s, **kw)
    with pytest.raises(ValueError, match="gate_start"):
        CtrlAviary(["tello"], 4, gate_watch=ap, gate_scenes=s, obstacle_scene_id=ids, gate_start=4, **kw)
    with pytest.raises(ValueError, match="gate_travel"):
        CtrlAviary(["tello"], 4, gate_watch=ap, gate_scenes=s, obstacle_scene_id=ids, gate_travel=0.0, **kw)


# ---- the aperture of the golden gate ---------------------------------------------------------------------------------------------
def test_the_examples_aperture_lies_inside_the_meshs_opening():
    """81 x 81 points of the rectangle |y| <= 0.30, |z| <= 0.20 on the plane x = 0: none closer to a triangle of gate_50_curved than
    0.038 m (the opening is |y| <= 0.35, |z| <= 0.25 with cut corners); the outer rectangle covers the frame's front."""
    ap, g = pr.gate_aperture(), sr.gate()
    y, z = np.meshgrid(np.linspace(-ap.half[0], ap.half[0], 81), np.linspace(-ap.half[1], ap.half[1], 81))
    pts = np.stack([np.zeros(y.size), y.ravel(), z.ravel()], 1)
    d = tri_dist(pts, g.triangles).min(1)
    print(f"least distance from the aperture to the mesh {d.min():.4f} m")
    assert 0.038 <= d.min() <= 0.05
    lo, hi = g.aabb
    assert ap.outer[0] >= max(-lo[1], hi[1]) - 1e-3 and ap.outer[1] >= max(-lo[2], hi[2]) - 1e-3


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def test_reference_against_dense_sampling():
    """200 chords of case 2 that the reference says cross a plane, 2 001 samples each: a sign change of n.(l - c) in the sampled
    chord exactly where the closed form has its crossing, tau within one sample spacing, and the sampled point on the same side
    of the aperture's border."""
    d = pr.case_placed(False)
    sc, sid, ap = d["scenes"], d["scene_id"], d["ap"]
    x = pr.crossings(d["prev"], d["pos"], None, sc, sid, ap)
    kind_any = np.argwhere(x["tau"] != 0)                                # (every plane crossing, whatever became of it)
    assert len(kind_any) >= 200
    q0, q1 = d["prev"].astype(np.float64), d["pos"].astype(np.float64)
    rng = np.random.default_rng(5)
    seen = {0: 0, 1: 0, 2: 0, 3: 0}
    for i, g in kind_any[rng.permutation(len(kind_any))[:200]]:
        R, t = sr.placement64(sc, sid[i], g)
        up, down, w = pr.dense_events(q0[i], q1[i], R, t, ap)
        k, tau = x["kind"][i, g], x["tau"][i, g]
        assert len(up) + len(down) <= 1                                     # a line crosses a plane once
        if k in (1, 3):
            assert len(up) == 1 and w[up[0]] - 1e-12 <= tau <= w[up[0] + 1] + 1e-12
        elif k == 2:
            assert len(down) == 1 and w[down[0]] - 1e-12 <= tau <= w[down[0] + 1] + 1e-12
        if len(up) + len(down) == 1 and k == 0:
            # a crossing the reference calls nothing: outside the aperture (and, forward, outside the outer rectangle too)
            j = (up if len(up) else down)[0]
            e = (q0[i] + 0.5 * (w[j] + w[j + 1]) * (q1[i] - q0[i]) - t) @ R - ap.center
            yy, zz = abs(e @ ap.u), abs(e @ ap.v)
            lim = ap.outer if len(up) else ap.half
            assert yy > lim[0] - 1e-3 or zz > lim[1] - 1e-3
        seen[int(k)] += 1
    print(f"dense sampling: {seen}")
    assert min(seen[1], seen[2], seen[3]) >= 5


def test_the_rule_on_the_row_of_three():
    """+3 in order with ascending times, +1 out of order, the wrap with its lap, a finished course staying put without it."""
    d = pr.case_row()
    for wrap, due, laps in ((False, [3, 1, 3, 3, 3, 3, 2, -1], [0] * 8), (True, [0, 1, 0, 3, 1, 0, 2, -1], [1, 0, 1, 0, 1, 1, 0, 0])):
        r = pr.reference(d["prev"], d["pos"], None, d["scenes"], d["scene_id"], d["ap"], d["due"], d["laps"], wrap=wrap, clock=7)
        assert r["due"].tolist() == due and r["laps"].tolist() == laps
        assert (r["fwd"] == 7).all() and not r["back"].any() and not r["miss"].any()
        assert 7 < r["times"][(0, 0)] < r["times"][(1, 0)] < r["times"][(2, 0)] < 8
        assert r["passes"] + r["out_of_order"] == 24 and r["passes"] == (10 if wrap else 9)


def test_redraw_caps_and_what_the_cases_hold():
    """For every GPU case's draw: at most 1 % of the chords re-drawn, none left within GUARD of a decision but the planted state,
    and every kind of event present."""
    for shape in ("rect", "ellipse"):
        d = pr.case_one(shape)
        assert d["redrawn"] <= 0.01
        x = pr.crossings(d["prev"], d["pos"], None, d["scenes"], d["scene_id"], d["ap"])
        assert np.nonzero(x["bad"])[0].tolist() == [pr.ONE_PLANTED]
        k = x["kind"][:, 0]
        assert min((k == 1).sum(), (k == 2).sum(), (k == 3).sum()) >= 20 and (x["look"] & ~x["swept"]).sum() == 2
        assert k[pr.ONE_PLANTED] == 1 and x["tau"][pr.ONE_PLANTED, 0] == 1.0 and k[pr.ONE_TELEPORT] == 0
        assert not k[list(pr.ONE_PARALLEL)].any() and not k[list(pr.ONE_ZERO)].any()
        x2 = pr.crossings(d["pos"], d["pos2"], None, d["scenes"], d["scene_id"], d["ap"])
        assert not x2["kind"].any()                                         # the state on the plane was counted by the first chord
    for d in (pr.case_placed(False), pr.case_placed(True), pr.case_ragged()):
        assert d["redrawn"] <= 0.01
        x = pr.crossings(d["prev"], d["pos"], d["off"], d["scenes"], d["scene_id"], d["ap"])
        assert not x["bad"].any() and x["swept"].all()
    for off in (False, True):
        d = pr.case_placed(off)
        r = pr.reference(d["prev"], d["pos"], d["off"], d["scenes"], d["scene_id"], d["ap"], d["due"], d["laps"], wrap=off)
        assert min(r["passes"], r["wrong_way"], r["out_of_order"], r["misses"]) >= 10
        assert (np.bincount(d["due"], minlength=4) > 100).all()
    assert not pr.crossings(*(pr.case_row()[k] for k in ("prev", "pos", "off", "scenes", "scene_id", "ap")))["bad"].any()


def test_restated_tau_error_is_what_is_recorded():
    """The float32 restatement of gate_eval against the fp64 reference on the GPU cases' own inputs: the same crossings, and its
    worst |tau32 - tau64| |s1 - s0| is the recorded RESTATED_WORST (not above it, and the record is not padded); the kernel is
    granted 4 x it, far below GUARD."""
    worst = 0.0
    for name, prev, pos, off, sc, sid, ap in pr.gpu_cases():
        x = pr.crossings(prev, pos, off, sc, sid, ap)
        t32 = pr.restated_tau(prev, pos, off, sc, sid, ap)
        ok = ~x["bad"] & x["swept"]
        assert np.array_equal((t32 != 0)[ok], (x["tau"] != 0)[ok]), name                 # (outside GUARD: the same signs)
        worst = max(worst, pr.tau_error(t32, x))
    print(f"restated worst {worst:.3e} m")
    assert worst <= pr.RESTATED_WORST <= 1.02 * worst, worst
    assert pr.TAU_TOL == 4.0 * pr.RESTATED_WORST and pr.TAU_TOL <= pr.GUARD / 4 and pr.GUARD == 1e-4


def test_two_half_chords_pass_what_the_whole_chord_passes():
    d = pr.case_row()
    mid = (0.55 * d["prev"] + 0.45 * d["pos"]).astype(np.float32).astype(np.float64)
    a = (d["scenes"], d["scene_id"], d["ap"])
    whole = pr.reference(d["prev"], d["pos"], None, *a, d["due"], d["laps"])
    h1 = pr.reference(d["prev"], mid, None, *a, d["due"], d["laps"])
    h2 = pr.reference(mid, d["pos"], None, *a, h1["due"], h1["laps"])
    assert not pr.crossings(d["prev"], mid, None, *a)["bad"].any() and not pr.crossings(mid, d["pos"], None, *a)["bad"].any()
    assert h2["due"].tolist() == whole["due"].tolist() and h1["passes"] + h2["passes"] == whole["passes"] and 0 < h1["passes"]
