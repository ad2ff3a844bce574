"""CPU-side checks of the obstacle witnesses (dsim_obstacle_witnesses, dsim_obstacle_witnesses_scenes, obstacles.witnesses /
witnesses_scenes, CtrlAviary(obstacle_witnesses=m)): the fp64 reference against the witness's and the point watch's references in
slot 0 and by hand, the float32 restatement against witness_ref's records, the caps of the re-draw rule and of the masks on every
GPU case's reference, the ABI names and the struct mirror, the Python calls through a recording stand-in for the library, and the
env's keyword checks (tests/README_witnesses.md)."""
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
from tests import witnesses_ref as ws
from tests.obstacle_ref import brute

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nat():
    graft.build()
    from dronesim_amd import _native
    return _native


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def test_slot_0_of_the_reference_is_the_witness_reference():
    """On the GPU cases' own inputs: slot 0 is witness_ref.brute_witness (_scenes) — clearance, body, triangle, vector, contacts —
    and obstacle_ref.brute's clearance and contacts."""
    for case in (("five", 3, False), ("five", 5, True), ("soup", 8), ("scene", 3, "gates"), ("scene", 4, "ragged"), ("evict", 8)):
        d, ref = ws.reference(*case)
        if "scenes" in d:
            one = wr.brute_witness_scenes(d["pos"], d["scenes"], d["scene_id"], d["rad"], d["margin"], d["off"])
        else:
            one = wr.brute_witness(d["pos"], d["set"], d["rad"], d["margin"], d["off"])
            b = brute(d["pos"], d["set"].triangles, d["set"].body, d["rad"], d["margin"], d["off"])
            assert np.abs(ref["clr"][0] - b[0]).max() <= 1e-12 and ref["contacts"] == b[3]
        assert np.array_equal(ref["in"][0], one["in"]) and np.array_equal(ref["clr"][0], one["clr"]), case
        assert np.array_equal(ref["body"][0], one["near"]) and np.array_equal(ref["tri"][0], one["tri"]), case
        assert np.array_equal(ref["rel"][0], one["rel"]) and ref["contacts"] == one["contacts"], case
        # the slots ascend, the filled ones are a prefix, and count counts them
        with np.errstate(invalid="ignore"):                    # (inf - inf between two unfilled slots)
            assert np.all(np.diff(ref["d"], axis=0)[ref["in"][1:]] >= 0) and np.all(ref["in"][1:] <= ref["in"][:-1])
        assert np.array_equal(ref["count"], np.minimum(ref["n_within"], ref["m"]))
        # no body twice
        for i in range(ref["body"].shape[1]):
            b = ref["body"][:, i][ref["in"][:, i]]
            assert len(set(b)) == len(b)


def test_three_triangles_by_hand():
    """Three unit right triangles in z = 0, at x = 0, 2 and 5: a point over the first at height 0.5."""
    from dronesim_amd.obstacles import ObstacleSet
    tri = np.array([[[x, 0.0, 0.0], [x + 1.0, 0.0, 0.0], [x, 1.0, 0.0]] for x in (0.0, 2.0, 5.0)])
    s = ObstacleSet(tri, np.arange(3))
    p = np.array([[0.25, 0.25, 0.5]], dtype=np.float32)
    rad = np.array([0.1], dtype=np.float32)
    ref = ws.brute_witnesses(p, s, rad, 3.0, 4)
    d1 = np.sqrt(1.75 ** 2 + 0.5 ** 2)                         # to (2, 0.25, 0) on the second's edge x = 2
    r = float(np.float32(0.1))
    assert ref["body"][:, 0].tolist() == [0, 1, -1, -1] and ref["count"][0] == 2 and ref["n_within"][0] == 2
    np.testing.assert_allclose(ref["clr"][:, 0], [0.5 - r, d1 - r, 3.0, 3.0], atol=1e-15)
    np.testing.assert_allclose(ref["rel"][:, 0], [[0, 0, -0.5], [1.75, 0, -0.5], [0, 0, 0], [0, 0, 0]], atol=1e-15)
    far = ws.brute_witnesses(p, s, rad, 5.0, 2)                # all three within 5 m, two slots: the two closest, count == m
    assert far["body"][:, 0].tolist() == [0, 1] and far["count"][0] == 2 and far["n_within"][0] == 3
    # an exact tie between two bodies keeps the lower body (the first met); the order mask flags it
    mid = ws.brute_witnesses(np.array([[1.5, 0.0, 0.0]], dtype=np.float32), s, rad, 3.0, 2)
    assert mid["body"][:, 0].tolist() == [0, 1] and mid["order"][0] and mid["clr"][0, 0] == mid["clr"][1, 0]


# ---- the input rule, the masks and the restatement on every GPU case -----------------------------------------------------------------
@pytest.mark.parametrize("case", ws.GPU_CASES, ids=lambda c: "-".join(map(str, c)))
def test_caps_and_restatement_on_a_gpu_case(case):
    """On the reference alone: at most 2 % of the case re-drawn and nobody left to re-draw; the order mask at most 1 %, the tie mask
    at most 1 % of the drones, the strict mask at most 15 % of the filled slots.  The float32 restatement of the kernel's arithmetic
    fills the reference's slots with the reference's bodies outside the order mask and stays below witness_ref's three records, so
    the tolerances are witness_ref's."""
    kind, m, *key = case
    d, ref = ws.reference(kind, m, *key)
    order, tie, strict = ws.mask_shares(ref)
    print(f"{case}: re-drawn {d['redrawn']:.4f}, order mask {order:.4f}, tie mask {tie:.4f}, strict mask {strict:.4f}, filled per slot "
          f"{ref['in'].sum(1).tolist()} of {ref['in'].shape[1]}, more bodies than slots {(ref['n_within'] > m).mean():.3f}")
    assert d["redrawn"] <= ws.REDRAW_CAP and not ref["redraw"].any()
    assert order <= ws.ORDER_CAP and tie <= wr.TIE_CAP and strict <= wr.STRICT_CAP
    assert (ws.REDRAW_CAP, ws.ORDER_CAP, ws.GUARD) == (0.02, 0.01, 1e-4)
    if "scenes" in d:
        rel, tri, inr, body = ws.restated_witnesses_scenes(d["pos"], d["scenes"], d["scene_id"], d["rad"], d["margin"], m, d["off"])
    else:
        rel, tri, inr, body = ws.restated_witnesses(d["pos"], d["set"], d["rad"], d["margin"], m, d["off"])
    keep = ~ref["order"]
    assert np.array_equal(inr, ref["in"]) and np.array_equal(body[:, keep], ref["body"][:, keep])
    on, opt, pos, ratio = ws.errors(rel, tri, ref, d.get("set"), d.get("scenes"), d.get("scene_id"))
    print(f"{case}: restated on {on:.3e} (record {wr.RESTATED_ON:.3e}), opt {opt:.3e} ({wr.RESTATED_OPT:.3e}), pos {pos:.3e} "
          f"({wr.RESTATED_POS:.3e}), pos / tie bound {ratio:.3f}")
    assert on <= wr.RESTATED_ON and opt <= wr.RESTATED_OPT and pos <= wr.RESTATED_POS and ratio <= 1.0


def test_what_the_cases_are_there_for():
    """Case 1: every permutation of the three bodies occurs; case 4: at least 10 % of the drones have more than 8 bodies within the
    margin and at least half more than 4; the soup leaves slots 4 .. 7 empty; case_gates fills every slot for somebody."""
    from itertools import permutations
    _, ref = ws.reference("three", 3)
    full = ref["in"].all(0)
    for p in permutations(range(3)):
        assert (full & (ref["body"][0] == p[0]) & (ref["body"][1] == p[1]) & (ref["body"][2] == p[2])).sum() >= 3, p
    assert set(ref["count"]) == {0, 1, 2, 3}
    _, ref = ws.reference("evict", 8)
    assert (ref["n_within"] > 8).mean() >= 0.10 and (ref["n_within"] > 4).mean() >= 0.5
    assert ws.evict_world().K == 4 and ws.evict_world().G == 32 and ws.evict_world().prototype.n_bodies == 2 and len(ref["count"]) == 1024
    _, ref = ws.reference("soup", 8)
    assert ref["in"][3].sum() >= 10 and not ref["in"][4:].any()
    _, ref = ws.reference("scene", 3, "gates")
    assert ref["in"].any(1).all()
    assert ws.five_bodies().n_tri == 144 and ws.five_bodies().n_bodies == 5


@pytest.mark.parametrize("clock", ws.MOVING_CLOCKS)
def test_caps_on_the_moving_case(clock):
    """The moving gates as the host's fp64 law places them at the three clocks, m = 3: the same caps."""
    d, motion, now = ws.moving_case(clock)
    ref = ws.brute_witnesses_scenes(d["pos"], now, d["scene_id"], d["rad"], d["margin"], ws.MOVING_M)
    order, tie, strict = ws.mask_shares(ref)
    slot = np.where(ref["in"], ref["tri"] // now.prototype.n_tri, 0)
    static = ref["in"] & ~motion.moving[d["scene_id"][None, :], slot]
    print(f"moving gates clock {clock}: re-drawn {d['redrawn']:.4f}, order {order:.4f}, tie {tie:.4f}, strict {strict:.4f}, filled "
          f"{ref['in'].sum(1).tolist()}, on a static placement {static.sum(1).tolist()}")
    assert d["redrawn"] <= ws.REDRAW_CAP and not ref["redraw"].any()
    assert order <= ws.ORDER_CAP and tie <= wr.TIE_CAP and strict <= wr.STRICT_CAP
    assert static[0].sum() >= 3 and (ref["in"][1] & ~static[1]).sum() >= 5


# ---- ABI -----------------------------------------------------------------------------------------------------------------------------
NEW = {"dsim_obstacle_witnesses": 6, "dsim_obstacle_witnesses_scenes": 7}
FIELDS = ["offset", "type_id", "margin", "m", "flags", "clearance_out", "body_out", "rel_out", "triangle_out", "count_out",
          "contacts_out", "twist", "vel_out"]


def test_header_declares_library_exports_and_mirror_matches(nat, tmp_path):
    hdr = open(os.path.join(ROOT, "include", "dronesim_amd.h")).read()
    lib = nat.load()
    minor = hdr[hdr.index("#define DSIM_ABI_MINOR"):hdr.index("#define DSIM_MAX_ACT")]
    for f, n_args in NEW.items():
        m = re.search(rf"^int\s+{f}\s*\(([^;]*)\);", hdr, flags=re.M | re.S)
        assert m, f
        assert m.group(1).count(",") + 1 == n_args == len(getattr(lib, f).argtypes), f
        assert f in nat.EXPORTS and f in minor
    assert "dsim_witnesses_args" in minor and "DSIM_WITNESSES_MAX" in minor
    assert re.search(r"#define DSIM_ABI_VERSION 11\b", hdr) and re.search(r"#define DSIM_ABI_MINOR 1\b", hdr)
    assert lib.dsim_abi_version() == 11 and lib.dsim_abi_minor() == 1 and (nat.ABI_VERSION, nat.ABI_MINOR) == (11, 1)
    assert os.path.join(ROOT, "dronesim_amd", "csrc", "dsim_witnesses.hip") in graft.HIP_DEPS and len(graft.HIP_SRCS) == 6
    assert '#include "dsim_witnesses.hip"' in open(os.path.join(ROOT, "dronesim_amd", "csrc", "dsim_obstacles.hip")).read()
    assert [f for f, _ in nat.WitnessesArgs._fields_] == FIELDS
    lines = ['printf("size %zu\\n", sizeof(dsim_witnesses_args));', 'printf("max %d\\n", (int)DSIM_WITNESSES_MAX);']
    lines += [f'printf("{f} %zu\\n", offsetof(dsim_witnesses_args, {f}));' for f in FIELDS]
    src = tmp_path / "witnesses.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dronesim_amd.h"\nint main(void) {\n' + "\n".join(lines)
                   + "\nreturn 0; }\n")
    exe = tmp_path / "witnesses"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(nat.WitnessesArgs) == 96 and int(got["max"]) == nat.WITNESSES_MAX == 8
    for f in FIELDS:
        assert int(got[f]) == getattr(nat.WitnessesArgs, f).offset, f


def test_library_refuses_null_arguments_before_it_touches_a_device(nat):
    lib = nat.load()
    v = nat.View()
    a = nat.WitnessesArgs()
    a.m = 3
    assert lib.dsim_obstacle_witnesses(None, None, 1, v, None, None) == -1
    assert lib.dsim_obstacle_witnesses(None, None, 1, v, None, ctypes.byref(a)) == -1
    assert lib.dsim_obstacle_witnesses_scenes(None, None, 1, v, None, None, None) == -1
    assert lib.dsim_obstacle_witnesses_scenes(None, None, 1, v, None, None, ctypes.byref(a)) == -1


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


def test_witnesses_calls_hand_the_library_what_they_were_given():
    import torch
    from dronesim_amd import _native as nat
    from dronesim_amd import obstacles as obs
    log = []
    ctx = types.SimpleNamespace(lib=_Lib(log), handle=11, stream_ptr=lambda: 22)
    state = types.SimpleNamespace(n=5, view=lambda: "view")
    dev = types.SimpleNamespace(handle=33)
    scn = obs.DeviceScenes.__new__(obs.DeviceScenes)           # (a DeviceScenes that owns nothing: _h = 0 keeps close() quiet)
    scn.__dict__.update(_h=0, twist=torch.zeros((1, 1, 8)))
    m = 3
    clr, body, tri = torch.zeros((m, 8)), torch.zeros((m, 8), dtype=torch.int32), torch.zeros((m, 8), dtype=torch.int32)
    rel, vel, off = torch.zeros((m, 3, 8)), torch.zeros((m, 3, 8)), torch.zeros((3, 8))
    count, ids = torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.int32)
    tid, cnt = torch.zeros(8, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64)
    obs.witnesses(ctx, state, dev, 0.5, m, clr, body, rel, tri, count, off, tid, cnt, body_frame=True)
    obs.witnesses(ctx, state, dev, 0.25, 8, clr, body, rel)
    assert log[0][:2] == ("dsim_obstacle_witnesses", (11, 22, 5, "view", 33))
    assert log[0][2] == dict(offset=off.data_ptr(), type_id=tid.data_ptr(), margin=0.5, m=3, flags=nat.WITNESS_BODY_FRAME,
                             clearance_out=clr.data_ptr(), body_out=body.data_ptr(), rel_out=rel.data_ptr(),
                             triangle_out=tri.data_ptr(), count_out=count.data_ptr(), contacts_out=cnt.data_ptr(), twist=None,
                             vel_out=None)
    assert log[1][2] == dict(offset=None, type_id=None, margin=0.25, m=8, flags=0, clearance_out=clr.data_ptr(),
                             body_out=body.data_ptr(), rel_out=rel.data_ptr(), triangle_out=None, count_out=None, contacts_out=None,
                             twist=None, vel_out=None)
    obs.witnesses_scenes(ctx, state, scn, ids, 0.5, m, clr, body, rel, vel=vel)
    assert log[2][:2] == ("dsim_obstacle_witnesses_scenes", (11, 22, 5, "view", 0, ids.data_ptr()))
    assert log[2][2]["twist"] == scn.twist.data_ptr() and log[2][2]["vel_out"] == vel.data_ptr() and log[2][2]["m"] == 3
    obs.witnesses_scenes(ctx, state, scn, ids, 0.5, m, clr, body, rel)
    assert log[3][2]["twist"] is None and log[3][2]["vel_out"] is None
    # the route through point_query
    obs.point_query(ctx, state, scn, ids, 0.5, clr, body, rel, off, tid, cnt, body_frame=True, vel=vel, m=m, count=count)
    assert log[4][0] == "dsim_obstacle_witnesses_scenes" and log[4][2]["count_out"] == count.data_ptr() and log[4][2]["flags"] == 1
    assert log[4][2]["vel_out"] == vel.data_ptr() and log[4][2]["triangle_out"] is None
    n_log = len(log)
    obs.point_query(ctx, state, dev, None, 0.5, clr, body, rel, m=2, count=count)
    assert log[n_log][0] == "dsim_obstacle_witnesses" and log[n_log][2]["m"] == 2 and log[n_log][2]["triangle_out"] is None
    n_log = len(log)
    for bad in (0, 9, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="m must be"):
            obs.witnesses(ctx, state, dev, 0.5, bad, clr, body, rel)
    with pytest.raises(ValueError, match="scene_id"):
        obs.witnesses_scenes(ctx, state, dev, None, 0.5, m, clr, body, rel)
    with pytest.raises(ValueError, match="rel"):
        obs.witnesses(ctx, state, dev, 0.5, m, clr, body, None)
    with pytest.raises(ValueError, match="DeviceScenes"):
        obs.point_query(ctx, state, dev, None, 0.5, clr, body, rel, vel=vel, m=m)
    assert len(log) == n_log
    w = obs.ObstacleWitnesses(1, 2, 3, None, 5)
    assert w._fields == ("clearance", "body", "rel", "vel", "count") and w.vel is None


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
    from dronesim_amd.envs.watches import StepWatches
    assert StepWatches._obst_m == 0 and StepWatches._obst_wits is None and StepWatches().last_obstacle_witnesses is None
    assert _options()._obst_m == 0 and _options(obstacle_watch=sr.gate(), obstacle_witness="world")._obst_m == 0
    for m in range(0, 9):
        assert _options(obstacle_watch=sr.gate(), obstacle_witness="body", obstacle_witnesses=m)._obst_m == m
    for bad in (9, -1, 2.0, "2", True, None):
        with pytest.raises(ValueError, match="obstacle_witnesses must be an int in 0..8"):
            _options(obstacle_watch=sr.gate(), obstacle_witness="world", obstacle_witnesses=bad)
    with pytest.raises(ValueError, match="obstacle_witnesses without obstacle_witness"):
        _options(obstacle_watch=sr.gate(), obstacle_witnesses=2)
    with pytest.raises(NotImplementedError, match="witness of a chord"):                 # the existing refusal fires first
        _options(obstacle_watch=sr.gate(), obstacle_sweep=True, obstacle_witness="world", obstacle_witnesses=2)


def test_env_refusals_before_a_context_is_made():
    from dronesim_amd.envs import CtrlAviary, VelocityAviary
    kw = dict(initial_xyzs=np.zeros((4, 3)), dict_io=False)
    for cls in (CtrlAviary, VelocityAviary):
        with pytest.raises(ValueError, match="obstacle_witnesses without obstacle_witness"):
            cls(["tello"], 4, obstacle_watch=sr.gate(), obstacle_witnesses=2, **kw)
        with pytest.raises(ValueError, match="obstacle_witnesses must be an int in 0..8"):
            cls(["tello"], 4, obstacle_watch=sr.gate(), obstacle_witness="world", obstacle_witnesses=9, **kw)
        with pytest.raises(NotImplementedError, match="witness of a chord"):
            cls(["tello"], 4, obstacle_watch=sr.gate(), obstacle_sweep=True, obstacle_witness="body", obstacle_witnesses=2, **kw)
        # the pinned refusals of the parent, unchanged with the keyword
        with pytest.raises(ValueError, match="obstacle_witness without obstacle_watch"):
            cls(["tello"], 4, obstacle_witness="world", obstacle_witnesses=2, **kw)
        with pytest.raises(ValueError, match="'world' or 'body'"):
            cls(["tello"], 4, obstacle_watch=sr.gate(), obstacle_witness="task", obstacle_witnesses=2, **kw)
        with pytest.raises(ValueError, match="obstacle_witness_velocity without obstacle_motion"):
            cls(["tello"], 4, obstacle_watch=sr.gate(), obstacle_witness="world", obstacle_witness_velocity=True,
                obstacle_witnesses=2, **kw)
    s = sr.case_ragged()["scenes"]
    with pytest.raises(NotImplementedError, match="chord in the placement's frame"):
        CtrlAviary(["tello"], 4, obstacle_watch=s, obstacle_scene_id=np.zeros(4, dtype=int), obstacle_sweep=True,
                   obstacle_witness="world", obstacle_witnesses=2, **kw)
