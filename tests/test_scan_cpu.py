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
