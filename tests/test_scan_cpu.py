"""What the range scanner's GPU tests rely on, checked without a device (tests/README_scan.md): the 1 % caps of the ambiguity masks
and the hit counts on the references alone, the recorded error of the float32 restatement, fan() geometry, beam validation, the
refusals of the env and of the scanner that come before a context exists, and the ctypes mirror of dsim_scan_args."""
import ctypes
import os

import numpy as np
import pytest

import __graft_entry__ as graft
from tests import scan_ref as sf


@pytest.fixture(scope="module")
def nat():
    graft.build()
    from dronesim_amd import _native
    return _native


def test_restated_error_is_what_is_recorded():
    """The float32 restatement of the kernel's arithmetic against the fp64 caster over the inputs of every GPU case: its worst
    camera_ref.t_error is the recorded SCAN_RESTATED_WORST (not above it, and the record is not padded); outside the mask the
    restatement hits exactly the rays the reference hits; and the mask covers at most 1 % of every case's rays."""
    worst = 0.0
    for name, t32, ref in sf.restated_inputs():
        share = float(ref["ambiguous"].mean())
        err = sf.t_error(t32, ref)
        print(f"{name}: restated t_error {err:.3e}, mask {share:.4%}")
        assert share <= sf.MASK_CAP, name
        assert not ((np.isfinite(t32) != np.isfinite(ref["t"])) & ~ref["ambiguous"]).any(), name
        worst = max(worst, err)
    print(f"restated worst {worst:.3e}")
    assert worst <= sf.SCAN_RESTATED_WORST <= 1.02 * worst, worst
    assert sf.SCAN_TOL == 4.0 * sf.SCAN_RESTATED_WORST


def test_the_cases_hit_what_they_are_meant_to_hit():
    c1, c2 = sf.case_main(0), sf.case_main(2)
    for c, least in ((c1, 300), (c2, 150)):
        h = c["ref"][0]["hit"]
        assert int((h >= 0).sum()) >= least and set(np.unique(h[h >= 0])) == {0, 1}
        assert int((c["ref"][1]["hit"] == -2).sum()) > 1000
    assert int((sf.case_edges()["ref"]["hit"] >= 0).sum()) >= 10 and not sf.EDGE_LEFT_OUT
    h = sf.case_scenes()["ref"][0]["hit"]
    assert int((h >= 0).sum()) >= 50 and set(np.unique(h[h >= 0])) == {0, 1, 2}
    assert int(sf.case_carry()["carry"].sum()) >= 5
    alone = sf.case_lattice(None)["ref"]
    assert int((alone["hit"] <= -3).sum()) >= 200
    who = -3 - alone["hit"]
    assert not ((alone["hit"] <= -3) & (who == np.arange(256)[None, :])).any()
    both = sf.case_lattice("set")
    sc = sf.lattice_scene(0)
    bare = sf.scan_brute(both["st"], both["beams"], sf.T_MIN, sf.T_MAX, tri=sc.triangles, body=sc.body)
    assert int(((both["ref"]["hit"] >= 0) & (alone["hit"] <= -3)).sum()) >= 3
    assert int(((both["ref"]["hit"] <= -3) & (bare["hit"] >= 0)).sum()) >= 3
    assert (alone["t"][alone["hit"] <= -3] <= sf.LATTICE_RANGE).all()


def test_offsets_are_exact():
    st = sf.case_main(0)["st"]
    off = sf.quarter_offsets(7, st.shape[0])
    moved = sf.with_offsets(st, off)
    assert np.array_equal(moved[:, :3] - off.astype(np.float32), st[:, :3]) and np.abs(off).max() <= 8.0


def test_fan_geometry():
    from dronesim_amd.scanner import RangeScanner
    b = RangeScanner.fan(16, up=True, down=True)
    assert b.shape == (18, 3) and b.dtype == np.float32
    assert np.allclose(np.linalg.norm(b.astype(np.float64), axis=1), 1.0, atol=1e-7)
    assert np.array_equal(b[0], [1, 0, 0]) and np.array_equal(b[4], [0, 1, 0]) and np.array_equal(b[8], [-1, 0, 0])
    assert np.array_equal(b[16], [0, 0, 1]) and np.array_equal(b[17], [0, 0, -1]) and (b[:16, 2] == 0).all()
    az = np.arctan2(b[:16, 1].astype(np.float64), b[:16, 0].astype(np.float64)) % (2 * np.pi)
    assert np.allclose(az, 2 * np.pi * np.arange(16) / 16, atol=1e-6)
    e = RangeScanner.fan(8, elevations=(-0.3, 0.0, 0.4))
    assert e.shape == (24, 3)
    for k, el in enumerate((-0.3, 0.0, 0.4)):
        assert np.allclose(e[8 * k: 8 * k + 8, 2], np.sin(el), atol=1e-7)
    assert RangeScanner.fan(0, down=True).shape == (1, 3) and RangeScanner.fan(16, elevations=(-0.6, -0.2, 0.2, 0.6)).shape == (64, 3)
    for bad in (dict(n_ring=0), dict(n_ring=64, up=True), dict(n_ring=-1), dict(n_ring=4, elevations=(np.pi / 2,))):
        with pytest.raises(ValueError):
            RangeScanner.fan(**bad)


def test_beam_validation():
    from dronesim_amd.scanner import check_range, unit_beams
    b = unit_beams([[3.0, 0.0, 4.0], [0.0, -2.0, 0.0], [1e-30, 0.0, 0.0], [1e200, 1e200, 0.0]])
    assert b.dtype == np.float32 and np.allclose(b[0], [0.6, 0.0, 0.8]) and np.array_equal(b[1], [0, -1, 0])
    assert np.array_equal(b[2], [1, 0, 0]) and np.allclose(b[3], [np.sqrt(0.5), np.sqrt(0.5), 0.0])
    for bad in ([[0.0, 0.0, 0.0]], [[1.0, np.nan, 0.0]], [[np.inf, 0.0, 0.0]], [[1.0, 0.0]], [1.0, 0.0, 0.0], np.zeros((0, 3)),
                np.ones((65, 3))):
        with pytest.raises(ValueError):
            unit_beams(bad)
    check_range(0.0, 1e-3)
    for lo, hi in ((-0.1, 1.0), (1.0, 1.0), (2.0, 1.0), (0.0, np.inf), (np.nan, 1.0), (0.0, np.nan)):
        with pytest.raises(ValueError):
            check_range(lo, hi)


class _NoContext:
    """Stands where a context would: every refusal below comes before anything touches it."""
    types = ()

    def __getattr__(self, name):
        raise AssertionError(f"the scanner touched ctx.{name} before it refused")


def test_scanner_refusals_before_a_context_is_used():
    from dronesim_amd.obstacles import ObstacleScenes, ObstacleSet
    from dronesim_amd.scanner import RangeScanner
    box = ObstacleSet.box((0, 0, 1), (1, 1, 1))
    scenes = ObstacleScenes(box, np.zeros((1, 1, 3)), np.zeros((1, 1, 3)))
    fan = RangeScanner.fan(4)
    ctx = _NoContext()
    for exc, kw in ((ValueError, dict(world=None)), (ValueError, dict(world=box, beams=[[0, 0, 0]])),
                    (ValueError, dict(world=box, t_min=2.0, t_max=1.0)), (ValueError, dict(world=box, drone_range=3.0)),
                    (ValueError, dict(world=box, drone_box=(0, 0, 1, 1))), (ValueError, dict(world=box, drones=True, drone_range=0.0)),
                    (ValueError, dict(world=box, drones=True, drone_box=(1, 0, 0, 1))), (TypeError, dict(world="gate")),
                    (ValueError, dict(world=scenes)), (ValueError, dict(world=box, scene_id=[0]))):
        kw.setdefault("beams", fan)
        world = kw.pop("world")
        with pytest.raises(exc):
            RangeScanner(ctx, None, world, **kw)


def test_env_refusals_before_a_context_is_made(monkeypatch):
    from dronesim_amd import fleet
    from dronesim_amd.envs import CtrlAviary, VelocityAviary
    from dronesim_amd.obstacles import ObstacleScenes, ObstacleSet
    from dronesim_amd.scanner import RangeScanner

    def no_context(*a, **k):
        raise AssertionError("a context was made before the refusal")
    monkeypatch.setattr(fleet, "Context", no_context)
    box = ObstacleSet.box((0, 0, 1), (1, 1, 1))
    fan = RangeScanner.fan(4)
    for env in (CtrlAviary, VelocityAviary):
        for kw in (dict(range_scene=box), dict(range_min=0.1), dict(range_max=5.0), dict(range_ground=False), dict(range_clamp=True),
                   dict(range_see_drones=True), dict(range_drone_range=2.0)):
            with pytest.raises(ValueError, match="without range_scan"):
                env(["tello"], 4, **kw)
        with pytest.raises(ValueError, match="world"):
            env(["tello"], 4, range_scan=fan, range_ground=False)
        with pytest.raises(ValueError):
            env(["tello"], 4, range_scan=[[0.0, 0.0, 0.0]])
        with pytest.raises(ValueError):
            env(["tello"], 4, range_scan=fan, range_min=3.0, range_max=2.0)
        with pytest.raises(ValueError):
            env(["tello"], 4, range_scan=fan, range_drone_range=2.0)
        with pytest.raises(ValueError, match="obstacle_scene_id"):
            env(["tello"], 4, range_scan=fan, range_scene=ObstacleScenes(box, np.zeros((1, 1, 3)), np.zeros((1, 1, 3))))

    class Sharded:
        def is_initialized(self): return True
        def get_world_size(self): return 2
        def get_rank(self): return 0
    with pytest.raises(NotImplementedError, match="radii of the other ranks"):
        CtrlAviary(["tello"], 4, range_scan=fan, range_see_drones=True, dist=Sharded())


def test_scan_args_mirror_matches_c(nat, tmp_path):
    """The ctypes mirror of dsim_scan_args has the C compiler's size and field offsets (the method of
    test_abi_cpu.py::test_struct_sizes_match_c), and the flags their values."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['printf("size %zu\\n", sizeof(dsim_scan_args));', 'printf("GROUND %u\\n", (unsigned)DSIM_SCAN_GROUND);',
             'printf("CLAMP %u\\n", (unsigned)DSIM_SCAN_CLAMP);']
    for fname, _ in nat.ScanArgs._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(dsim_scan_args, {fname}));')
    src = tmp_path / "scan_sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dronesim_amd.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "scan_sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(root, "include"), "-o", str(exe), str(src)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(nat.ScanArgs)
    for fname, _ in nat.ScanArgs._fields_:
        assert int(got[fname]) == getattr(nat.ScanArgs, fname).offset, fname
    assert (int(got["GROUND"]), int(got["CLAMP"])) == (nat.SCAN_GROUND, nat.SCAN_CLAMP)
    assert "dsim_range_scan" in nat.EXPORTS


# ---- the drones' walk at its edges: what tests/test_gpu_scan_edges.py takes for granted ---------------------------------------------
def test_edge_cases_are_what_the_gpu_tests_need():
    """Every case of scan_ref.restated_edge_inputs, on the references alone: the mask covers at most 1 % of the case's own rays,
    outside it the float32 restatement hits exactly what the reference hits, its worst t_error is the recorded
    SCAN_EDGE_RESTATED_WORST (not above it, the record not padded), which is not above SCAN_RESTATED_WORST: SCAN_EDGE_TOL is
    SCAN_TOL.  Then the floors: what each case must contain to be worth running."""
    worst = 0.0
    for name, t32, ref in sf.restated_edge_inputs():
        share = float(ref["ambiguous"].mean())
        err = sf.t_error(t32, ref)
        print(f"{name}: restated t_error {err:.3e}, mask {share:.4%}")
        assert share <= sf.MASK_CAP, name
        assert not ((np.isfinite(t32) != np.isfinite(ref["t"])) & ~ref["ambiguous"]).any(), name
        worst = max(worst, err)
    print(f"restated worst over the edge cases {worst:.3e}")
    assert worst <= sf.SCAN_EDGE_RESTATED_WORST <= 1.02 * worst, worst
    assert sf.SCAN_EDGE_RESTATED_WORST <= sf.SCAN_RESTATED_WORST and sf.SCAN_EDGE_TOL == sf.SCAN_TOL
    t_min, t_max, rng = sf.STACK_LIMITS
    # the stack: level drones, beams along the axes
    near, far = sf.case_stack(), sf.case_stack(sf.FAR_SHIFT)
    h = near["ref"]["hit"]
    assert near["st"].shape[0] == 300 and not near["ref"]["ambiguous"].any()
    assert int((h[4] <= -3).sum()) == 200 and int((h[5] <= -3).sum()) == 200         # up: layers 0 and 1; down: layers 1 and 2
    assert all(int((h[b] <= -3).sum()) >= 260 for b in range(4)) and int((h <= -3).sum()) >= 2000
    _, _, d = sf._rays32(near["st"], near["beams"], None)
    assert int((d == 0.0).sum()) == 4800 and d.size == 9000
    assert np.array_equal(far["ref"]["hit"], h) and np.abs(far["ref"]["t"][h <= -3] - near["ref"]["t"][h <= -3]).max() < 1e-9
    who = -3 - h
    assert not ((h <= -3) & (who == np.arange(300)[None, :])).any() and int(((h <= -3) & (who >= 256)).sum()) >= 200
    for shift in ((0.0, 0.0), sf.FAR_SHIFT):
        sf.stack_pinned_box(shift)                             # (asserts its construction)
    # offsets: the set and the plane from p - offset, the spheres from p
    c = sf.case_stack_offsets(0)
    ref, alt = c["ref"], sf.stack_offsets_partial()
    h = ref["hit"]
    assert int((h >= 0).sum()) >= 30 and int((h == -2).sum()) >= 150 and int((h <= -3).sum()) >= 2000
    bare = sf.scan_brute(c["st"], c["beams"], t_min, t_max, c["sc"].triangles, c["sc"].body, ground=True, offsets=c["off"])
    alone = sf.scan_brute(c["st"], c["beams"], t_min, t_max, radius=c["rad"], drone_range=rng)
    assert int(((h >= 0) & (alone["hit"] <= -3)).sum()) >= 20                    # a triangle in front of a sphere
    assert int(((h <= -3) & (bare["hit"] != -1)).sum()) >= 200                   # a sphere in front of a triangle or the plane
    both = ~ref["ambiguous"] & ~alt["ambiguous"]
    gap = np.abs(np.where(np.isfinite(ref["t"]), ref["t"], 1e9) - np.where(np.isfinite(alt["t"]), alt["t"], 1e9))
    differ = int((both & ((h != alt["hit"]) | (gap > 1e-3))).sum())
    print(f"beams that tell the spheres met from p from those met with part of the offset applied: {differ}")
    assert differ >= 20
    assert int((sf.case_stack_offsets(2)["ref"]["hit"] >= 0).sum()) >= 30
    # lost drones
    lost = sf.case_stack_lost()
    hb, hl = lost["before"]["hit"], lost["ref"]["hit"]
    saw = (hb <= -3) & np.isin(-3 - hb, sf.STACK_LOST[:2])
    saw[:, list(sf.STACK_LOST)] = False
    assert int(saw.sum()) >= 10 and not ((hl <= -3) & np.isin(-3 - hl, sf.STACK_LOST[:2])).any()
    assert int(((hl <= -3) & (-3 - hl == 255)).sum()) >= 5
    assert np.isinf(lost["ref"]["t"][:, list(sf.STACK_LOST)]).all() and (hl[:, list(sf.STACK_LOST)] == -1).all()
    # the sparse layer: a doubled cell
    sp = sf.case_sparse()
    assert sf.scan_grid(sp["st"])[0] >= 4.0 * sf.scan_grid(near["st"])[0] and int((sp["ref"]["hit"] <= -3).sum()) >= 200
    # the big fleet's sample
    big = sf.case_big()
    assert np.isin([0, 255, 256, sf.BIG_N - 256, sf.BIG_N - 1], big["sample"]).all() and big["sample"].size == 512
    assert int((big["ref"]["hit"] <= -3).sum()) >= 2000 and int((-3 - big["ref"]["hit"]).max()) > 65000
    # the raw table
    raw = sf.case_raw_beams()
    hr = raw["ref"]["hit"]
    assert int((hr >= 0).sum()) >= 50 and int((hr == -2).sum()) >= 500 and all((hr[k] != -1).any() for k in (0, 1, 2, 3, 5, 6))


def test_the_scanners_walk_finds_what_brute_force_finds():
    """walked_scan — the DRONES route of k_range_scan restated in float32 through the walker the camera's reference uses: the
    binning, s_in / s_out, the INFINITY branches of a zero dx or dy, the 3 x 3 block, the newly adjacent column or row, the early
    stop, the outside list — is restated_scan over all spheres BIT FOR BIT: the walk as designed loses no sphere, on axis beams,
    with centres on cell borders, 4 km out, with lost drones on no list and over a doubled cell."""
    t_min, t_max, rng = sf.STACK_LIMITS
    for shift in ((0.0, 0.0), sf.FAR_SHIFT):
        c = sf.case_stack(shift)
        t32 = sf.restated_scan(c["st"], c["beams"], t_min, t_max, radius=c["rad"], drone_range=rng)
        assert int(np.isfinite(t32).sum()) >= 2000
        for box in (None, sf.stack_pinned_box(shift)):
            assert np.array_equal(sf.walked_scan(c["st"], c["beams"], c["rad"], sf.scan_grid(c["st"], box), t_min, t_max, rng), t32), (shift, box)
    c = sf.case_stack_lost()
    t32 = sf.restated_scan(c["st"], c["beams"], t_min, t_max, radius=c["rad"], drone_range=rng)
    assert np.isinf(t32[:, list(sf.STACK_LOST)]).all()
    assert np.array_equal(sf.walked_scan(c["st"], c["beams"], c["rad"], sf.scan_grid(c["st"]), t_min, t_max, rng), t32)
    c = sf.case_sparse()
    t32 = sf.restated_scan(c["st"], c["beams"], t_min, sf.SPARSE_RANGE, radius=c["rad"], drone_range=sf.SPARSE_RANGE)
    assert np.array_equal(sf.walked_scan(c["st"], c["beams"], c["rad"], sf.scan_grid(c["st"]), t_min, sf.SPARSE_RANGE, sf.SPARSE_RANGE), t32)
