"""CPU-side checks of the obstacle witness (dsim_obstacle_witness, dsim_obstacle_witness_scenes, obstacles.witness /
witness_scenes, CtrlAviary(obstacle_witness=...)): the fp64 reference against obstacle_ref.tri_dist, the recorded float32 errors
the GPU tolerances come from, the caps of the two masks on every GPU case's reference, the ABI names and the struct mirror, the
Python calls through a recording stand-in for the library, and the env's keyword checks (tests/README_witness.md)."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

import __graft_entry__ as graft
from tests import scenes_ref as sr
from tests import witness_ref as wr
from tests.obstacle_ref import brute, tri_dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nat():
    graft.build()
    from dronesim_amd import _native
    return _native


def _plain_cases():
    return (("one triangle", wr.case_one_triangle()), ("gate", wr.case_gate(False)), ("gate, offsets", wr.case_gate(True)),
            ("soup", wr.case_soup()))


def _scene_cases():
    return (("gates", False), ("gates", True), ("ragged", False), ("soup", False))


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def test_reference_distance_is_tri_dist():
    """The region walk's distance against the edge-and-plane brute force of obstacle_ref, on the GPU cases' own points: 1e-12."""
    worst = 0.0
    for _, d in _plain_cases():
        q = sr._task_points(d["pos"], d["off"])
        W, D = wr.closest(q, d["set"].triangles)
        worst = max(worst, float(np.abs(D - tri_dist(q, d["set"].triangles)).max()))
        a = d["set"].triangles.astype(np.float64)
        # ... and the point lies in the triangle's plane, inside it: barycentric coordinates in [0, 1]
        n = np.cross(a[:, 1] - a[:, 0], a[:, 2] - a[:, 0])
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        assert np.abs(np.einsum("ptk,tk->pt", W - a[None, :, 0], n)).max() < 1e-12
    print(f"closest() against tri_dist: {worst:.3e} m")
    assert worst <= 1e-12


def test_reference_agrees_with_the_point_watch_references():
    """clearance, nearest and contacts of the witness references are those of obstacle_ref.brute and scenes_ref.brute_scenes."""
    for _, d in _plain_cases():
        s, ref = d["set"], d["ref"]
        b = brute(d["pos"], s.triangles, s.body, d["rad"], d["margin"], d["off"])
        assert np.abs(ref["clr"] - b[0]).max() <= 1e-12 and ref["contacts"] == b[3]
        sure = ~((b[1] >= 0) & (b[2] < 1e-9))
        assert np.array_equal(ref["near"][sure], b[1][sure])
    for name, off in _scene_cases():
        d, ref = wr.scene_ref(name, off)
        assert np.abs(ref["clr"] - d["ref"]["clr"]).max() <= 1e-12 and ref["contacts"] == d["ref"]["contacts"]
        sure = ~((d["ref"]["near"] >= 0) & (d["ref"]["gap"] < 1e-9))
        assert np.array_equal(ref["near"][sure], d["ref"]["near"][sure])
        # |rel| is the distance: to 1e-7 of itself, because the vector went back through a float32 R that is orthonormal to 6e-8
        m = ref["in"]
        assert (np.abs(np.linalg.norm(ref["rel"][m], axis=1) - ref["d"][m]) / ref["d"][m]).max() <= 1e-7 and np.all(ref["rel"][~m] == 0.0)
    for _, d in _plain_cases():                                  # ... and exactly so on a plain set
        ref, m = d["ref"], d["ref"]["in"]
        assert np.abs(np.linalg.norm(ref["rel"][m], axis=1) - ref["d"][m]).max() <= 1e-12 and np.all(ref["rel"][~m] == 0.0)


def test_one_triangle_by_hand():
    """A point over the face, beside an edge and beyond a vertex of the unit right triangle in z = 0."""
    tri = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]])
    p = np.array([[0.25, 0.25, 2.0], [0.5, -3.0, 0.0], [-1.0, -1.0, 1.0], [1.0, 1.0, 0.0]])
    W, D = wr.closest(p, tri)
    np.testing.assert_allclose(W[:, 0], [[0.25, 0.25, 0.0], [0.5, 0.0, 0.0], [0.0, 0.0, 0.0], [0.5, 0.5, 0.0]], atol=1e-15)
    np.testing.assert_allclose(D[:, 0], [2.0, 3.0, np.sqrt(3.0), np.sqrt(0.5)], atol=1e-15)


# ---- the recorded errors and the masks -------------------------------------------------------------------------------------------------
def test_restated_errors_are_what_is_recorded():
    """The float32 restatement of the kernel's arithmetic against the fp64 reference over the GPU cases' own inputs: the worst
    on-surface, optimality and position error are the recorded constants (not above them, and the records not padded), it has a
    witness exactly where the reference has, and it stays inside the tie bound; the kernel is granted 4 x each record."""
    worst = [0.0, 0.0, 0.0, 0.0]
    for name, d in _plain_cases():
        rel, tri, inr = wr.restated_witness(d["pos"], d["set"], d["rad"], d["margin"], d["off"])
        assert np.array_equal(inr, d["ref"]["in"]), name
        e = wr.errors(rel, tri, d["ref"], d["set"])
        print(f"restated {name}: on {e[0]:.3e}, opt {e[1]:.3e}, pos {e[2]:.3e}, pos / tie bound {e[3]:.3e}")
        worst = [max(a, b) for a, b in zip(worst, e)]
    for name, off in _scene_cases():
        d, ref = wr.scene_ref(name, off)
        rel, tri, inr = wr.restated_witness_scenes(d["pos"], d["scenes"], d["scene_id"], d["rad"], d["margin"], d["off"])
        assert np.array_equal(inr, ref["in"]), name
        e = wr.errors(rel, tri, ref, None, d["scenes"], d["scene_id"])
        print(f"restated scenes {name} offsets={off}: on {e[0]:.3e}, opt {e[1]:.3e}, pos {e[2]:.3e}, pos / tie bound {e[3]:.3e}")
        worst = [max(a, b) for a, b in zip(worst, e)]
    print(f"restated worst: on {worst[0]:.4e}, opt {worst[1]:.4e}, pos {worst[2]:.4e}, pos / tie bound {worst[3]:.3e}")
    assert worst[0] <= wr.RESTATED_ON <= 1.02 * worst[0]
    assert worst[1] <= wr.RESTATED_OPT <= 1.02 * worst[1]
    assert worst[2] <= wr.RESTATED_POS <= 1.02 * worst[2]
    assert worst[3] <= 1.0
    assert (wr.TOL_ON, wr.TOL_OPT, wr.TOL_POS) == (4.0 * wr.RESTATED_ON, 4.0 * wr.RESTATED_OPT, 4.0 * wr.RESTATED_POS)
    assert wr.E == wr.TOL_ON + wr.TOL_OPT and wr.TOL_OPT <= sr.GUARD / 4       # (the input rule's guard band decides in / out)


def test_mask_caps_hold_on_every_gpu_case():
    """On the reference alone: the tie mask holds at most 1 % of the drones, the strict mask at most 15 % of those in reach."""
    seen = {}
    for name, d in _plain_cases():
        seen[name] = wr.mask_shares(d["ref"]) + (int(d["ref"]["in"].sum()),)
    for name, off in _scene_cases():
        d, ref = wr.scene_ref(name, off)
        seen[f"scenes {name} offsets={off}"] = wr.mask_shares(ref) + (int(ref["in"].sum()),)
    for k, (tie, strict, inr) in seen.items():
        print(f"{k}: tie mask {tie:.4f} of all, strict mask {strict:.4f} of the {inr} in reach")
        assert tie <= wr.TIE_CAP and strict <= wr.STRICT_CAP and inr >= 30, k
    assert wr.TIE_CAP == 0.01 and wr.STRICT_CAP == 0.15 and wr.STRICT_DIST == 1e-4 and wr.STRICT_SEP == 1e-5
    assert seen["one triangle"][:2] == (0.0, 0.0)
    # the one triangle's drones meet all seven regions on both sides of the plane, within reach
    from tests.obstacle_ref import region
    d = wr.case_one_triangle()
    reg, side = region(d["pos"].astype(np.float64), d["set"].triangles[0])
    for k in range(7):
        for sg in (-1.0, 1.0):
            assert ((reg == k) & (side == sg) & d["ref"]["in"]).sum() >= 3, (k, sg)
    # what the issue counted on the inputs of scenes_ref.py: 49 of 489, 1 of 36, 0 of 421
    for name, off, want in (("gates", False, (49, 489)), ("ragged", False, (1, 36)), ("soup", False, (0, 421))):
        ref = wr.scene_ref(name, off)[1]
        assert (int(ref["strict"].sum()), int(ref["in"].sum())) == want, name


def test_masks_catch_a_rival_on_a_flat_face():
    """Two coplanar unit squares of two triangles each, a slit of 2 cm between them.  A point over a square's diagonal: both
    triangles hold the witness at the same point, no mask.  A point over the middle of the slit: two witnesses 2 cm apart at the
    same distance, both masks.  A point well inside one triangle: the rival is 5 cm farther, no mask."""
    from dronesim_amd.obstacles import ObstacleSet
    from tests.util import f32
    sq = lambda x0: np.array([[[x0, 0, 0], [x0 + 1, 0, 0], [x0 + 1, 1, 0]], [[x0, 0, 0], [x0 + 1, 1, 0], [x0, 1, 0]]], dtype=np.float64)
    s = ObstacleSet(np.concatenate([sq(0.0), sq(1.0 + 2e-2)]), 0)
    p = f32(np.array([[0.5, 0.5, 0.3], [1.0 + 1e-2, 0.5, 0.3], [0.25, 0.5, 0.3]]))
    ref = wr.brute_witness(p, s, np.full(3, np.float32(0.1)), 1.0)
    assert ref["in"].all() and ref["tie"].tolist() == [False, True, False] and ref["strict"].tolist() == [False, True, False]


# ---- ABI -----------------------------------------------------------------------------------------------------------------------------
NEW = {"dsim_obstacle_witness": 6, "dsim_obstacle_witness_scenes": 7}


def test_header_declares_library_exports_and_mirror_matches(nat, tmp_path):
    hdr = open(os.path.join(ROOT, "include", "dronesim_amd.h")).read()
    lib = nat.load()
    minor = hdr[hdr.index("#define DSIM_ABI_MINOR"):hdr.index("#define DSIM_MAX_ACT")]
    for f, n_args in NEW.items():
        m = re.search(rf"^int\s+{f}\s*\(([^;]*)\);", hdr, flags=re.M | re.S)
        assert m, f
        assert m.group(1).count(",") + 1 == n_args == len(getattr(lib, f).argtypes), f
        assert f in nat.EXPORTS and f in minor
    assert "dsim_witness_args" in minor and "DSIM_WITNESS_BODY_FRAME" in minor
    assert re.search(r"#define DSIM_ABI_VERSION 11\b", hdr) and re.search(r"#define DSIM_ABI_MINOR 1\b", hdr)
    assert lib.dsim_abi_version() == 11 and lib.dsim_abi_minor() == 1
    assert os.path.join(ROOT, "dronesim_amd", "csrc", "dsim_witness.hip") in graft.HIP_DEPS and len(graft.HIP_SRCS) == 6
    fields = [f for f, _ in nat.WitnessArgs._fields_]
    assert fields == ["offset", "type_id", "margin", "flags", "clearance_out", "nearest_out", "rel_out", "triangle_out", "contacts_out"]
    lines = ['printf("size %zu\\n", sizeof(dsim_witness_args));', 'printf("body %d\\n", (int)DSIM_WITNESS_BODY_FRAME);']
    lines += [f'printf("{f} %zu\\n", offsetof(dsim_witness_args, {f}));' for f in fields]
    src = tmp_path / "witness.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dronesim_amd.h"\nint main(void) {\n' + "\n".join(lines)
                   + "\nreturn 0; }\n")
    exe = tmp_path / "witness"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(nat.WitnessArgs) and int(got["body"]) == nat.WITNESS_BODY_FRAME == 1
    for f in fields:
        assert int(got[f]) == getattr(nat.WitnessArgs, f).offset, f


def test_library_refuses_null_arguments_before_it_touches_a_device(nat):
    lib = nat.load()
    v = nat.View()
    a = nat.WitnessArgs()
    assert lib.dsim_obstacle_witness(None, None, 1, v, None, None) == -1
    assert lib.dsim_obstacle_witness(None, None, 1, v, None, ctypes.byref(a)) == -1
    assert lib.dsim_obstacle_witness_scenes(None, None, 1, v, None, None, None) == -1
    assert lib.dsim_obstacle_witness_scenes(None, None, 1, v, None, None, ctypes.byref(a)) == -1


# ---- the Python calls, through a recording stand-in for the library ----------------------------------------------------------------------
class _Lib:
    def __init__(self, log):
        self._log = log

    def __getattr__(self, name):
        def call(*a):
            arg = a[-1]._obj                                   # (the byref'd struct: copy what it holds now)
            self._log.append((name, a[:-1], {f: getattr(arg, f) for f, _ in type(arg)._fields_}))
            return 0
        return call


def test_witness_calls_hand_the_library_what_they_were_given():
    import torch
    from dronesim_amd import _native as nat
    from dronesim_amd import obstacles as obs
    log = []
    ctx = types.SimpleNamespace(lib=_Lib(log), handle=11, stream_ptr=lambda: 22)
    state = types.SimpleNamespace(n=5, view=lambda: "view")
    dev = types.SimpleNamespace(handle=33)
    clr, near, tri, ids = torch.zeros(8), torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.int32)
    rel, off = torch.zeros((3, 8)), torch.zeros((3, 8))
    tid, cnt = torch.zeros(8, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64)
    obs.witness(ctx, state, dev, 0.5, clr, near, rel, tri, off, tid, cnt, body_frame=True)
    obs.witness(ctx, state, dev, 0.25, clr, None, rel)
    obs.witness_scenes(ctx, state, dev, ids, 0.5, clr, near, rel, tri, off, tid, cnt)
    assert log[0][:2] == ("dsim_obstacle_witness", (11, 22, 5, "view", 33))
    assert log[0][2] == dict(offset=off.data_ptr(), type_id=tid.data_ptr(), margin=0.5, flags=nat.WITNESS_BODY_FRAME,
                             clearance_out=clr.data_ptr(), nearest_out=near.data_ptr(), rel_out=rel.data_ptr(),
                             triangle_out=tri.data_ptr(), contacts_out=cnt.data_ptr())
    assert log[1][2] == dict(offset=None, type_id=None, margin=0.25, flags=0, clearance_out=clr.data_ptr(), nearest_out=None,
                             rel_out=rel.data_ptr(), triangle_out=None, contacts_out=None)
    assert log[2][:2] == ("dsim_obstacle_witness_scenes", (11, 22, 5, "view", 33, ids.data_ptr())) and log[2][2]["flags"] == 0
    with pytest.raises(ValueError, match="scene_id"):
        obs.witness_scenes(ctx, state, dev, None, 0.5, clr, near, rel)
    with pytest.raises(ValueError, match="rel"):
        obs.witness(ctx, state, dev, 0.5, clr, near, None)
    with pytest.raises(ValueError, match="rel"):
        obs.witness_scenes(ctx, state, dev, ids, 0.5, clr, near, None)
    assert len(log) == 3


# ---- the env's keyword -----------------------------------------------------------------------------------------------------------------
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


def test_keyword_has_a_default_and_is_checked():
    assert _options()._obst_wit is None and _options(obstacle_watch=sr.gate())._obst_wit is None
    for frame in ("world", "body"):
        assert _options(obstacle_watch=sr.gate(), obstacle_witness=frame)._obst_wit == frame
    with pytest.raises(ValueError, match="'world' or 'body'"):
        _options(obstacle_watch=sr.gate(), obstacle_witness=True)
    with pytest.raises(ValueError, match="obstacle_witness without obstacle_watch"):
        _options(obstacle_witness="world")
    with pytest.raises(NotImplementedError, match="witness of a chord"):
        _options(obstacle_watch=sr.gate(), obstacle_sweep=True, obstacle_witness="world")
    from dronesim_amd.envs.watches import StepWatches
    assert StepWatches._obst_wit is None and StepWatches._obst_rel is None and StepWatches().last_obstacle_witness is None


def test_env_refusals_before_a_context_is_made():
    from dronesim_amd.envs import CtrlAviary, VelocityAviary
    kw = dict(initial_xyzs=np.zeros((4, 3)), dict_io=False)
    for cls in (CtrlAviary, VelocityAviary):
        with pytest.raises(ValueError, match="obstacle_witness without obstacle_watch"):
            cls(["tello"], 4, obstacle_witness="world", **kw)
        with pytest.raises(NotImplementedError, match="witness of a chord"):
            cls(["tello"], 4, obstacle_watch=sr.gate(), obstacle_sweep=True, obstacle_witness="body", **kw)
        with pytest.raises(ValueError, match="'world' or 'body'"):
            cls(["tello"], 4, obstacle_watch=sr.gate(), obstacle_witness="task", **kw)
    # the pinned refusal of the swept watch on scenes stays what it was, with or without the keyword
    s = sr.case_ragged()["scenes"]
    with pytest.raises(NotImplementedError, match="chord in the placement's frame"):
        CtrlAviary(["tello"], 4, obstacle_watch=s, obstacle_scene_id=np.zeros(4, dtype=int), obstacle_sweep=True,
                   obstacle_witness="world", **kw)
