"""CPU-side checks of line of sight (dsim_line_of_sight, LineOfSight, CtrlAviary(neighbor_sight=True)): the recorded float32 error
the GPU tolerance comes from, the cap of the ambiguity mask and the floors on every GPU case's reference, the fp64 reference by
hand, the ABI names and the struct mirror, the Python class through a recording stand-in for the library, and the env's keyword
checks (tests/README_sight.md)."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

import __graft_entry__ as graft
from tests import camera_ref as cr
from tests import scenes_ref as sr
from tests import sight_ref as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nat():
    graft.build()
    from dronesim_amd import _native
    return _native


# ---- the recorded error, the mask and the floors ---------------------------------------------------------------------------------------
def test_restated_error_is_what_is_recorded():
    """The float32 restatement of the kernel's arithmetic against sight_brute over the inputs of every GPU case: its worst
    camera_ref.t_error is the recorded SIGHT_RESTATED_WORST (not above it, and the record not padded by more than 2 %); outside
    the mask the restatement blocks exactly the segments the reference blocks; the kernel is granted 4 x the record."""
    worst = 0.0
    for name, c in sg.gpu_cases():
        r, ref = sg.restated(c), c["ref"]
        err = cr.t_error(r, ref)
        wrong = int((np.isfinite(r) != np.isfinite(ref["t"]))[~ref["ambiguous"]].sum())
        print(f"restated {name}: t_error {err:.3e}, {wrong} blocked / clear differ outside the mask")
        assert wrong == 0, name
        worst = max(worst, err)
    print(f"restated worst: {worst:.4e}")
    assert worst <= sg.SIGHT_RESTATED_WORST <= 1.02 * worst, worst
    assert sg.SIGHT_TOL == 4.0 * sg.SIGHT_RESTATED_WORST


def test_mask_cap_holds_on_every_gpu_case():
    """On the reference alone: the ambiguity mask covers at most 1 % of a case's cast segments."""
    for name, c in sg.gpu_cases():
        share = sg.mask_share(c["ref"])
        print(f"{name}: mask {share:.4f} of {int(c['ref']['cast'].sum())} cast segments")
        assert share <= sg.MASK_CAP, name
    assert sg.MASK_CAP == 0.01


def test_cases_hold_what_the_gpu_tests_need():
    """The floors: what each case must contain to be worth running."""
    for w, (subdiv, k, _, _, floor) in enumerate(sg.MAIN):
        c = sg.case_main(w)
        ref, n = c["ref"], c["pos"].shape[0]
        assert n == (300 if subdiv == 0 else 192) and c["rel"].shape == (k, 3, n) and ref["cast"].all()
        blocked = ref["blocker"] >= 0
        print(f"main {w}: {int(blocked.sum())} of {blocked.size} segments blocked, bodies {np.unique(ref['blocker'][blocked])}")
        assert int(blocked.sum()) >= floor and set(np.unique(ref["blocker"][blocked])) == {0, 1}
        assert np.array_equal(ref["visible"] == 0, blocked) and np.array_equal(np.isfinite(ref["frac"]), blocked)
        assert ((ref["frac"][blocked] >= 0.0) & (ref["frac"][blocked] <= 1.0)).all()
        # no unmasked pair is seen one way and hidden the other (no offsets: the segment j -> i is the segment i -> j)
        vis = {}
        for t in range(k):
            for i in range(n):
                if not ref["ambiguous"][t, i]:
                    vis[(i, int(c["index"][t, i]))] = int(ref["visible"][t, i])
        assert all(vis.get((j, i), v) == v for (i, j), v in vis.items())
    # the knn record: sparse drones leave slots unused, and those read 0 / -1 / +inf
    c = sg.case_knn(0)
    unused = c["index"] < 0
    assert 10 <= int(unused.sum()) and (c["index"] >= 0).sum() > 4000 and int((c["ref"]["blocker"] >= 0).sum()) >= 100
    assert not c["ref"]["cast"][unused].any() and np.all(c["rel"].transpose(0, 2, 1)[unused] == 0.0)
    assert sg.case_knn(1)["rel"].shape[0] == 1
    # the edges: every kind of slot that is not cast, axis segments that hit, the wall's two sides
    c = sg.case_edges(0)
    ref, names = c["ref"], c["names"]
    assert not ref["cast"][:, names.index("nan position")].any() and not ref["cast"][:, names.index("inf position")].any()
    assert ref["cast"][:, names.index("bad rel")].tolist() == [False, False, False, True, False, False, False, True]
    for nm in ("corner", "lo_x", "hi_y", "off_y", "off_corner", "aim_x", "aim_z", "aim_back"):
        assert ref["cast"][:, names.index(nm)].tolist() == [True] * 6 + [False, False], nm
    assert int((ref["blocker"][:6, [names.index(nm) for nm in ("aim_x", "aim_z", "aim_back")]] >= 0).sum()) >= 3
    assert ref["visible"][:, names.index("wall")].tolist() == [1, 0, 1, 0, 1, 0, 1, 0]
    assert ref["visible"][:, names.index("outside")].all() and ref["visible"][:6, names.index("off_corner")].sum() >= 4
    for key, fill in (("visible", 0), ("blocker", -1), ("frac", np.inf)):
        assert np.all(ref[key][~ref["cast"]] == fill)
    # scenes: drones whose id is outside [0, K) or whose scene is empty are all clear; the others meet every slot's gate
    for c, empty in ((sg.case_scenes(), (-1, 0, 6)), (sg.case_lattice_scenes(0), (-1, 2)), (sg.case_lattice_scenes(2), (-1, 2))):
        ref, sid = c["ref"], np.asarray(c["scene_id"])
        none = np.isin(sid, empty)
        assert none.sum() >= 50 and ref["visible"][:, none].all() and int((ref["blocker"] >= 0).sum()) >= 20
    assert sg.case_scenes()["ref"]["blocker"].max() >= 2                 # (a body of a second placement: instance-major numbering)
    # the ground: every target below the plane is hidden by it or by a body before it, none above it by the plane
    for with_set in (True, False):
        c = sg.case_ground(with_set)
        ref, below = c["ref"], c["below"]
        assert (ref["visible"][below] == 0).all() and not (ref["blocker"][~below] == sg.SEG_GROUND).any()
        assert int((ref["blocker"][below] == sg.SEG_GROUND).sum()) >= (1000 if with_set else 1200)
        if not with_set:
            assert (ref["blocker"][below] == sg.SEG_GROUND).all() and ref["visible"][~below].all()


def test_reference_by_hand():
    """One wall x = 1 (two triangles, body 3) and the plane: a segment through it, one that stops short, one that ends ON it (both
    ends closed), one that starts behind it, one parallel to it, one dropping through the plane first."""
    wall = np.array([[[1, -1, -1], [1, 1, -1], [1, 1, 2]], [[1, -1, -1], [1, 1, 2], [1, -1, 2]]], dtype=np.float32)
    pos = np.array([[0.0, 0.0, 0.5]] * 5 + [[1.5, 0.0, 0.5]], dtype=np.float32)
    rel = np.array([[2, 0, 0], [0.5, 0, 0], [1, 0, 0], [0, 0.5, 0.25], [4, 0, -1], [1, 0, 0]], dtype=np.float32).T[None]
    ref = sg.sight_brute(pos, rel, None, wall, 3, ground=True)
    assert ref["visible"][0].tolist() == [0, 1, 0, 1, 0, 1]
    assert ref["blocker"][0].tolist() == [3, -1, 3, -1, 3, -1]
    np.testing.assert_allclose(ref["frac"][0][[0, 2, 4]], [0.5, 1.0, 0.25], atol=1e-15)
    ref = sg.sight_brute(pos, rel, None, None, None, ground=True)
    assert ref["blocker"][0].tolist() == [-1, -1, -1, -1, -2, -1] and ref["frac"][0][4] == 0.5
    # offsets move the drone, not the segment's direction; an index below 0 is not cast
    off = np.zeros((6, 3)); off[0, 0] = -2.0                   # drone 0 now stands behind the wall
    idx = np.ones((1, 6), dtype=np.int32); idx[0, 2] = -1
    ref = sg.sight_brute(pos, rel, idx, wall, 3, offsets=off)
    assert ref["visible"][0].tolist() == [1, 1, 0, 1, 0, 1] and ref["cast"][0].tolist() == [True, True, False, True, True, True]
    assert ref["blocker"][0, 2] == -1 and np.isinf(ref["frac"][0, 2])
    r32 = sg.restated_sight(pos, rel, idx, wall, offsets=off)
    assert np.array_equal(np.isfinite(r32), np.isfinite(ref["frac"]))


# ---- ABI -----------------------------------------------------------------------------------------------------------------------------
def test_header_declares_library_exports_and_mirror_matches(nat, tmp_path):
    hdr = open(os.path.join(ROOT, "include", "dronesim_amd.h")).read()
    lib = nat.load()
    minor = hdr[hdr.index("#define DSIM_ABI_MINOR"):hdr.index("#define DSIM_MAX_ACT")]
    m = re.search(r"^int\s+dsim_line_of_sight\s*\(([^;]*)\);", hdr, flags=re.M | re.S)
    assert m and m.group(1).count(",") + 1 == 6 == len(lib.dsim_line_of_sight.argtypes)
    assert lib.dsim_line_of_sight.argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, nat.View, ctypes.c_void_p,
                                               ctypes.POINTER(nat.SightArgs)]
    for name in ("dsim_line_of_sight", "dsim_sight_args", "DSIM_SIGHT_GROUND"):
        assert name in minor, name
    assert "dsim_line_of_sight" in nat.EXPORTS
    assert re.search(r"#define DSIM_ABI_VERSION 11\b", hdr) and re.search(r"#define DSIM_ABI_MINOR 1\b", hdr)
    assert lib.dsim_abi_version() == 11 and lib.dsim_abi_minor() == 1
    assert os.path.join(ROOT, "dronesim_amd", "csrc", "dsim_sight.hip") in graft.HIP_DEPS and len(graft.HIP_SRCS) == 6
    fields = [f for f, _ in nat.SightArgs._fields_]
    assert fields == ["rel", "index", "k", "flags", "offset", "scenes", "scene_id", "visible_out", "blocker_out", "frac_out"]
    lines = ['printf("size %zu\\n", sizeof(dsim_sight_args));', 'printf("GROUND %u\\n", (unsigned)DSIM_SIGHT_GROUND);']
    lines += [f'printf("{f} %zu\\n", offsetof(dsim_sight_args, {f}));' for f in fields]
    src = tmp_path / "sight.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dronesim_amd.h"\nint main(void) {\n' + "\n".join(lines)
                   + "\nreturn 0; }\n")
    exe = tmp_path / "sight"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(nat.SightArgs) and int(got["GROUND"]) == nat.SIGHT_GROUND == 1
    for f in fields:
        assert int(got[f]) == getattr(nat.SightArgs, f).offset, f
    assert nat.SIGHT_MAX_K == 32


def test_library_refuses_null_arguments_before_it_touches_a_device(nat):
    lib = nat.load()
    v = nat.View()
    a = nat.SightArgs()
    assert lib.dsim_line_of_sight(None, None, 1, v, None, None) == -1
    assert lib.dsim_line_of_sight(None, None, 1, v, None, ctypes.byref(a)) == -1


# ---- the Python class, through a recording stand-in for the library ----------------------------------------------------------------------
class _Lib:
    def __init__(self, log):
        self._log = log

    def __getattr__(self, name):
        def call(*a):
            arg = a[-1]._obj                                   # (the byref'd struct: copy what it holds now)
            self._log.append((name, a[:-1], {f: getattr(arg, f) for f, _ in type(arg)._fields_}))
            return 0
        return call


def _fake(n=5, n_pad=8):
    import torch
    log = []
    ctx = types.SimpleNamespace(lib=_Lib(log), handle=11, stream_ptr=lambda: 22, device=torch.device("cpu"), types=[])
    state = types.SimpleNamespace(n=n, n_pad=n_pad, view=lambda: "view")
    return ctx, state, log


def test_query_hands_the_library_what_it_was_given():
    import torch
    from dronesim_amd import _native as nat
    from dronesim_amd.sight import LineOfSight, Sight
    ctx, state, log = _fake()
    off = np.arange(15, dtype=np.float64).reshape(5, 3)
    los = LineOfSight(ctx, state, None, 3, ground=True, offsets=off)
    assert tuple(los.visible_out.shape) == tuple(los.blocker_out.shape) == tuple(los.frac_out.shape) == (3, 8)
    assert los._off.shape == (3, 8) and np.array_equal(los._off[:, :5].numpy(), off.T.astype(np.float32)) and not los._off[:, 5:].any()
    rel = torch.zeros((3, 3, 8))
    idx = torch.zeros((3, 8), dtype=torch.int32)
    s = los.query(rel, idx)
    assert isinstance(s, Sight) and all(tuple(t.shape) == (3, 5) for t in s)
    assert s.visible.data_ptr() == los.visible_out.data_ptr() and s.frac.data_ptr() == los.frac_out.data_ptr()
    assert log[0][:2] == ("dsim_line_of_sight", (11, 22, 5, "view", None))
    assert log[0][2] == dict(rel=rel.data_ptr(), index=idx.data_ptr(), k=3, flags=nat.SIGHT_GROUND, offset=los._off.data_ptr(), scenes=None,
                             scene_id=None, visible_out=los.visible_out.data_ptr(), blocker_out=los.blocker_out.data_ptr(),
                             frac_out=los.frac_out.data_ptr())
    s = los.query(rel[:, :, :5], None, blocker=False, frac=False)          # (a record cut to its first n drones: the same storage)
    assert s.blocker is None and s.frac is None
    assert log[1][2]["rel"] == rel.data_ptr() and log[1][2]["index"] is None and log[1][2]["blocker_out"] is None and log[1][2]["frac_out"] is None
    from dronesim_amd.downwash import Neighbors
    s = los.query_neighbors(Neighbors(idx[:, :5], None, rel[:, :, :5], None, None))
    assert log[2][2]["rel"] == rel.data_ptr() and log[2][2]["index"] == idx.data_ptr() and len(log) == 3
    with pytest.raises(ValueError, match="rel_pos"):
        los.query_neighbors(Neighbors(idx, None, None, None, None))
    los.close()


def test_host_validation():
    import torch
    from dronesim_amd.sight import LineOfSight
    ctx, state, log = _fake()
    for k in (0, 33, 2.5, True):
        with pytest.raises(ValueError, match="1 .. 32"):
            LineOfSight(ctx, state, None, k, ground=True)
    with pytest.raises(ValueError, match="no world"):
        LineOfSight(ctx, state, None, 4)
    with pytest.raises(TypeError, match="world takes"):
        LineOfSight(ctx, state, "gate", 4)
    with pytest.raises(ValueError, match="scene_id without"):
        LineOfSight(ctx, state, None, 4, ground=True, scene_id=np.zeros(5, dtype=int))
    with pytest.raises(ValueError, match="scene_id is required"):
        LineOfSight(ctx, state, sr.case_ragged()["scenes"], 4)
    with pytest.raises(ValueError, match=r"offsets must be \[5, 3\]"):
        LineOfSight(ctx, state, None, 4, ground=True, offsets=np.zeros((4, 3)))
    los = LineOfSight(ctx, state, None, 32, ground=True)
    ok = torch.zeros((32, 3, 8))
    for bad in (torch.zeros((31, 3, 8)), torch.zeros((32, 3, 7)), torch.zeros((32, 3, 8), dtype=torch.float64), torch.zeros((32, 8, 3)).transpose(1, 2),
                torch.zeros((32, 3, 5)), np.zeros((32, 3, 8), dtype=np.float32)):
        with pytest.raises(ValueError, match="rel must be"):
            los.query(bad)
    for bad in (torch.zeros((32, 8)), torch.zeros((32, 5), dtype=torch.int32), torch.zeros((8, 32), dtype=torch.int32).t()):
        with pytest.raises(ValueError, match="index must be"):
            los.query(ok, bad)
    assert not log
    los.query(ok, torch.zeros((32, 8), dtype=torch.int32)[:, :5])
    assert len(log) == 1 and log[0][2]["k"] == 32


def test_mask_packs_the_slots():
    import torch
    from dronesim_amd.sight import Sight
    vis = torch.tensor([[1, 0, 1], [0, 0, 1], [1, 0, 0]], dtype=torch.int32)
    assert Sight(vis, None, None).mask().tolist() == [5, 0, 3]
    full = Sight(torch.ones((32, 2), dtype=torch.int32), None, None).mask()
    assert full.dtype == torch.int32 and full.tolist() == [-1, -1]


# ---- the env's keywords ----------------------------------------------------------------------------------------------------------------
def _options(**kw):
    from dronesim_amd.envs.watches import StepWatches
    base = dict(num_drones=4, freq=240, aggregate_phy_steps=1, dist=None, drone_watch=False, drone_watch_margin=1.0,
                obstacle_watch=None, obstacle_margin=1.0, obstacle_sweep=False, obstacle_sweep_sag=0.0, obstacle_sweep_travel=None,
                vision_attributes=False, vision_scene=None, vision_drones=None, vision_res=(64, 48), vision_ground=True,
                vision_see_drones=False, vision_drone_range=None)
    base.update(kw)
    w = StepWatches()
    w._watch_options(**base)
    return w


def test_keywords_have_defaults_and_are_checked():
    from dronesim_amd.envs.watches import StepWatches
    assert StepWatches._sight_on is False and StepWatches._sight is None and StepWatches().last_neighbor_sight is None
    w = _options()
    assert w._sight_on is False and w.last_neighbor_sight is None
    assert _options(neighbor_obs=4, neighbor_radius=2.0)._sight_on is False
    gate = sr.gate()
    w = _options(neighbor_obs=4, neighbor_radius=2.0, neighbor_sight=True, obstacle_watch=gate)
    assert w._sight_on is True and w._sight_scene is None
    w = _options(neighbor_obs=4, neighbor_radius=2.0, neighbor_sight=True, neighbor_sight_scene=gate)
    assert w._sight_on is True and w._sight_scene is gate
    with pytest.raises(ValueError, match="neighbor_sight=True without neighbor_obs"):
        _options(neighbor_sight=True, obstacle_watch=gate)
    with pytest.raises(ValueError, match="needs a world to look at"):
        _options(neighbor_obs=4, neighbor_radius=2.0, neighbor_sight=True)
    with pytest.raises(ValueError, match="neighbor_sight_scene without neighbor_sight"):
        _options(neighbor_obs=4, neighbor_radius=2.0, neighbor_sight_scene=gate)
    scenes = sr.case_ragged()["scenes"]
    with pytest.raises(ValueError, match="obstacle_scene_id .* is required"):
        _options(neighbor_obs=4, neighbor_radius=2.0, neighbor_sight=True, neighbor_sight_scene=scenes)
    w = _options(neighbor_obs=4, neighbor_radius=2.0, neighbor_sight=True, neighbor_sight_scene=scenes, obstacle_scene_id=np.zeros(4, dtype=int))
    assert w._sight_scene is scenes
    with pytest.raises(ValueError, match="neighbor_sight_scene="):
        _options(obstacle_scene_id=np.zeros(4, dtype=int))
    with pytest.raises(ValueError, match="neighbor_sight\\(\\) needs an env made with neighbor_sight=True"):
        _options().neighbor_sight()


def test_env_refusals_before_a_context_is_made():
    from dronesim_amd.envs import CtrlAviary, VelocityAviary
    kw = dict(initial_xyzs=np.zeros((4, 3)), dict_io=False)
    for cls in (CtrlAviary, VelocityAviary):
        with pytest.raises(ValueError, match="neighbor_sight=True without neighbor_obs"):
            cls(["tello"], 4, neighbor_sight=True, obstacle_watch=sr.gate(), **kw)
        with pytest.raises(ValueError, match="needs a world to look at"):
            cls(["tello"], 4, neighbor_obs=2, neighbor_radius=1.0, neighbor_sight=True, **kw)
        with pytest.raises(ValueError, match="neighbor_sight_scene without neighbor_sight"):
            cls(["tello"], 4, neighbor_obs=2, neighbor_radius=1.0, neighbor_sight_scene=sr.gate(), **kw)
