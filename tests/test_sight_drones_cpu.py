"""CPU-side checks of line of sight among the drones (dsim_line_of_sight_drones, LineOfSight(drones=True),
CtrlAviary(neighbor_sight_drones=True)): the recorded float32 error the GPU tolerance comes from, the cap of the ambiguity mask and
the floors on every GPU case's reference, the fp64 reference by hand, the restatement against the shared walker, the ABI names,
the Python class through a recording stand-in for the library, and the env's keyword checks (tests/README_sight_drones.md)."""
import ctypes
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest

import __graft_entry__ as graft
from tests import scan_ref as sf
from tests import scenes_ref as sr
from tests import sight_drones_ref as sd
from tests import sight_ref as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nat():
    graft.build()
    from dronesim_amd import _native
    return _native


# ---- the recorded error, the mask and the floors ---------------------------------------------------------------------------------------
def test_restated_error_is_what_is_recorded():
    """The float32 restatement of the kernel's arithmetic against sight_drones_brute over the inputs of every GPU case: its worst
    camera_ref.t_error is the recorded SIGHT_DRONES_RESTATED_WORST (not above it, and the record not padded by more than 2 %);
    outside the mask the restatement blocks exactly the segments the reference blocks; the kernel is granted 4 x the record."""
    worst = 0.0
    for name, c in sd.gpu_cases():
        r, ref = sd.restated(c), c["ref"]
        err = sd.t_error(r, ref)
        wrong = int((np.isfinite(r) != np.isfinite(ref["t"]))[~ref["ambiguous"]].sum())
        print(f"restated {name}: t_error {err:.3e}, {wrong} blocked / clear differ outside the mask")
        assert wrong == 0, name
        worst = max(worst, err)
    print(f"restated worst: {worst:.4e}")
    assert worst <= sd.SIGHT_DRONES_RESTATED_WORST <= 1.02 * worst, worst
    assert sd.SIGHT_DRONES_TOL == 4.0 * sd.SIGHT_DRONES_RESTATED_WORST
    readme = open(os.path.join(ROOT, "tests", "README_sight_drones.md")).read()
    assert f"SIGHT_DRONES_RESTATED_WORST = {sd.SIGHT_DRONES_RESTATED_WORST:.2e}" in readme


def test_mask_cap_holds_on_every_gpu_case():
    """On the reference alone: the ambiguity mask covers at most 1 % of a case's cast segments."""
    for name, c in sd.gpu_cases():
        share = sd.mask_share(c["ref"])
        print(f"{name}: mask {share:.4f} of {int(c['ref']['cast'].sum())} cast segments")
        assert share <= sd.MASK_CAP, name
    assert sd.MASK_CAP == 0.01
    # the chunk cases' small fleet too
    rel, index = sd.chunk_record()
    sc = sg.case_main(0)["sc"]
    ref = sd.sight_drones_brute(sd.main_pos(), rel, index, sd.main_radii(), tri=sc.triangles, body=sc.body)
    assert sd.mask_share(ref) <= sd.MASK_CAP


def test_cases_hold_what_the_gpu_tests_need():
    """The floors: what each case must contain to be worth running."""
    for w, (kind, subdiv, offsets) in enumerate(sd.MAIN):
        c = sd.case_main(w)
        ref = c["ref"]
        drones, tris = ref["blocker"] <= -3, ref["blocker"] >= 0
        got = (int(drones.sum()), int(tris.sum()), int((tris & ref["both"]).sum()), int((drones & ref["both"]).sum()))
        print(f"main {sd.MAIN[w]}: drones block {got[0]}, triangles {got[1]}, a triangle before a drone {got[2]}, a drone before a triangle {got[3]}")
        assert all(g >= f for g, f in zip(got, sd.FLOORS[kind])) and c["pos"].shape[0] == 300
        assert c["rel"].shape[0] == {"knn16": 16, "knn1": 1, "goal32": 32}[kind] and (c["index"] is None) == (kind == "goal32")
        assert len(c["tri"]) == (108 if subdiv == 0 else 1548)
        assert ("offsets" in c) == offsets
        who = -3 - ref["blocker"][drones]
        assert not (who[None, :] == np.nonzero(drones)[1][None, :]).all() or who.size == 0        # nobody hides a neighbour from itself
        assert not (ref["blocker"] == -3 - np.arange(300)[None, :]).any()
        if c["index"] is not None:
            assert not (ref["blocker"] == -3 - c["index"])[c["index"] >= 0].any()        # ... nor does the slot's own target
    # the goal segments end at the centre of a drone: without offsets none is clear
    assert not sd.case_main(3)["ref"]["visible"].any()
    # offsets move the triangles' frame, not the spheres: the world's answers are those of the fleet without offsets
    a, b = sd.case_main(0), sd.case_main(1)
    base = lambda c: sg.sight_brute(c["pos"], c["rel"], c["index"], c["tri"], c["body"], offsets=c.get("offsets"))
    assert np.array_equal(base(a)["blocker"], base(b)["blocker"]) and not np.array_equal(a["ref"]["blocker"], b["ref"]["blocker"])
    # the edges: zero components, both tiles, the lost drone, the type of radius 0
    for zero in (False, True):
        c = sd.case_edges(zero)
        ref, rel = c["ref"], c["rel"]
        assert ((rel[:, 0] == 0) & (rel[:, 1] != 0)).any() and ((rel[:, 1] == 0) & (rel[:, 0] != 0)).any()
        assert ((rel[:, 0] == 0) & (rel[:, 1] == 0)).any()
        assert not ref["cast"][:, sd.EDGE_LOST].any() and not (ref["blocker"] == -3 - sd.EDGE_LOST).any()
        assert int((ref["blocker"][:, 256:] <= -3).sum()) >= 100
        if zero:
            assert ((-3 - ref["blocker"][ref["blocker"] <= -3]) % 2 == 1).all() and int((ref["blocker"][:, 0::2] <= -3).sum()) >= 300
    # the pinned box leaves rows on the outside list
    box = sf.stack_pinned_box()
    st = sf.case_stack()["st"]
    assert int((st[:, 1] > box[3] + 0.5).sum()) >= 20
    for s in (None, 0, 2):
        ref = sd.case_scenes(s)["ref"]
        assert int((ref["blocker"] <= -3).sum()) >= 1000 and int((ref["blocker"] >= 0).sum()) >= 30
    ref = sd.case_plane()["ref"]
    assert int((ref["blocker"] == sd.SEG_GROUND).sum()) >= 500 and int((ref["blocker"] <= -3).sum()) >= 500
    # the chunk layout: exact shifts, indices inside their copy
    pos, off, rel, idx, j = sd.chunk_layout(1000)
    assert np.array_equal(pos - off.astype(np.float32), sd.main_pos()[j]) and idx.max() < 1000
    assert ((idx < 0) | (idx // 300 == (np.arange(1000) // 300)[None, :])).all()


def test_reference_by_hand():
    """The column of three and the drone that stands inside a ball."""
    c = sd.case_column(False)
    ref, R = c["ref"], float(c["rad"][1])
    assert ref["visible"][0, 0] == 1                                             # A -> B: the target is left out
    assert ref["blocker"][1, 0] == -3 - 1 and abs(ref["frac"][1, 0] - (1.0 - R) / 2.5) < 1e-12      # A -> C: B, where its ball begins
    assert ref["blocker"][1, 2] == -3 - 1 and abs(ref["frac"][1, 2] - (1.5 - R) / 2.5) < 1e-12      # C -> A: B from the other side
    assert not ref["visible"][:, 3].any() and np.all(ref["frac"][:, 3] == 0.0) and np.all(ref["blocker"][:, 3] == -3 - 1)
    assert not ref["cast"][1:, 4].any() and ref["visible"][0, 4] == 1
    goal = sd.sight_drones_brute(c["pos"], c["rel"], None, c["rad"])             # no index: B hides itself
    assert goal["blocker"][0, 0] == -3 - 1 and abs(goal["frac"][0, 0] - (1.0 - R)) < 1e-12
    # a label table renames the blocker; a range of 0.25 cuts the balls beyond a quarter of the segment
    lab = np.array([10, 11, 12, 13, 14])
    assert sd.sight_drones_brute(c["pos"], c["rel"], c["index"], c["rad"], label=lab)["blocker"][1, 0] == -3 - 11
    short = sd.sight_drones_brute(c["pos"], c["rel"], c["index"], c["rad"], rng=0.25)
    assert short["visible"][1, 0] == 1 and not short["visible"][:, 3].any()
    # the plane and a ball share s
    g = sd.case_column(True)["ref"]
    assert g["blocker"][1, 4] == sd.SEG_GROUND and g["frac"][1, 4] == 0.5
    # a radius of 0 is no target, a position that is not finite neither
    rad = c["rad"].copy()
    rad[1] = 0.0
    assert sd.sight_drones_brute(c["pos"], c["rel"], c["index"], rad)["visible"][1, 0] == 1
    pos = c["pos"].copy()
    pos[1, 2] = np.nan
    r = sd.sight_drones_brute(pos, c["rel"], c["index"], c["rad"])
    assert r["visible"][1, 0] == 1 and not r["cast"][:, 1].any()


def test_the_walk_loses_no_ball():
    """The float32 restatement without a grid and the one through camera_drones_ref.walk_rays (the binning, the 2-D walk, the
    early stop, the outside list) are bit-equal on the edge cases, on the measured and on the pinned box, for every drone that
    stands in nobody's ball (there the walker's surface rule and the solid ball are one rule) — and on the main fleet's goal
    segments for a sample of drones."""
    for zero in (False, True):
        c = sd.case_edges(zero)
        clear = np.nonzero(sd.starts_clear(c["pos"], c["rad"]))[0]
        assert clear.size >= 290
        who = clear[::7]
        flat = sd.restated_balls(c["pos"], c["rel"], None, c["rad"])[:, who]
        st = sf.case_stack()["st"].copy()
        st[:, :3] = c["pos"]
        for box in (None, sf.stack_pinned_box()):
            w = sd.walked(c["pos"], c["rel"], None, c["rad"], sf.scan_grid(st, box), who)
            assert np.array_equal(w, flat), (zero, box)
        assert int(np.isfinite(flat).sum()) >= 100
    c = sd.case_main(0)
    clear = np.nonzero(sd.starts_clear(c["pos"], c["rad"]))[0]
    who = clear[::11]
    flat = sd.restated_balls(c["pos"], c["rel"], c["index"], c["rad"])[:, who]
    st = np.zeros((300, 7), np.float32)
    st[:, :3] = c["pos"]
    w = sd.walked(c["pos"], c["rel"], c["index"], c["rad"], sf.scan_grid(st), who)
    assert np.array_equal(w, flat) and int(np.isfinite(flat).sum()) >= 20


# ---- ABI -----------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_export_and_the_struct_is_unchanged(nat, tmp_path):
    hdr = open(os.path.join(ROOT, "include", "dronesim_amd.h")).read()
    lib = nat.load()
    minor = hdr[hdr.index("#define DSIM_ABI_MINOR"):hdr.index("#define DSIM_MAX_ACT")]
    m = re.search(r"^int\s+dsim_line_of_sight_drones\s*\(([^;]*)\);", hdr, flags=re.M | re.S)
    assert m and m.group(1).count(",") + 1 == 8 == len(lib.dsim_line_of_sight_drones.argtypes)
    assert lib.dsim_line_of_sight_drones.argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, nat.View, ctypes.c_void_p,
                                                      ctypes.POINTER(nat.SightArgs), ctypes.c_void_p, ctypes.POINTER(nat.CameraDrones)]
    assert "dsim_line_of_sight_drones" in minor and "dsim_line_of_sight_drones" in nat.EXPORTS
    assert re.search(r"#define DSIM_ABI_VERSION 11\b", hdr) and re.search(r"#define DSIM_ABI_MINOR 1\b", hdr)
    assert lib.dsim_abi_version() == 11 and lib.dsim_abi_minor() == 1
    # the argument order against a C compiler: a call with every argument of its own type compiles without a warning
    fields = ["rel", "index", "k", "flags", "offset", "scenes", "scene_id", "visible_out", "blocker_out", "frac_out"]
    assert [f for f, _ in nat.SightArgs._fields_] == fields
    lines = ['printf("size %zu\\n", sizeof(dsim_sight_args));']
    lines += [f'printf("{f} %zu\\n", offsetof(dsim_sight_args, {f}));' for f in fields]
    src = tmp_path / "sight_drones.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dronesim_amd.h"\n'
                   "typedef int (*fn)(dsim_ctx*, void*, int64_t, dsim_view, const dsim_obstacles*, const dsim_sight_args*, const uint8_t*,\n"
                   "                  const dsim_camera_drones*);\n"
                   "int main(void) {\nfn f = dsim_line_of_sight_drones;\n"
                   "int (*g)(dsim_ctx*, void*, int64_t, dsim_view, const dsim_obstacles*, const dsim_sight_args*) = dsim_line_of_sight;\n"
                   + "\n".join(lines) + "\nreturn (f != 0 && g != 0) ? 0 : 1; }\n")
    obj = tmp_path / "sight_drones.o"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o", str(obj), str(src)])
    exe = tmp_path / "sight_drones"
    subprocess.check_call(["gcc", "-o", str(exe), str(obj), nat.LIB_PATH, f"-Wl,-rpath,{os.path.dirname(nat.LIB_PATH)}",
                           "-Wl,--unresolved-symbols=ignore-in-shared-libs"])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(nat.SightArgs) == 72
    for f in fields:
        assert int(got[f]) == getattr(nat.SightArgs, f).offset, f


def test_library_refuses_null_arguments_before_it_touches_a_device(nat):
    lib = nat.load()
    v = nat.View()
    a = nat.SightArgs()
    d = nat.CameraDrones()
    assert lib.dsim_line_of_sight_drones(None, None, 1, v, None, None, None, None) == -1
    assert lib.dsim_line_of_sight_drones(None, None, 1, v, None, ctypes.byref(a), None, ctypes.byref(d)) == -1


# ---- the Python class, through a recording stand-in for the library ----------------------------------------------------------------------
class _Lib:
    def __init__(self, log):
        self._log = log

    def __getattr__(self, name):
        def call(*a):
            self._log.append((name, a))
            return 0
        return call


class _Targets:
    """What LineOfSight asks of a DroneTargets."""

    def __init__(self):
        from dronesim_amd import _native as nat
        self.dr, self.planned, self.fresh = nat.CameraDrones(), 0, 0
        self.dr.range = 1.0

    def grid_args(self):
        self.planned += 1
        return "grid"

    def refresh_box(self):
        self.fresh += 1

    def outside(self):
        return 7

    def keepalive(self):
        return ["ws", "label", "count"]


def _fake(n=5, n_pad=8, n_types=1):
    import torch
    log = []
    ctx = types.SimpleNamespace(lib=_Lib(log), handle=11, stream_ptr=lambda: 22, device=torch.device("cpu"), types=[None] * n_types)
    state = types.SimpleNamespace(n=n, n_pad=n_pad, view=lambda: "view")
    return ctx, state, log


def test_query_calls_the_old_symbol_without_drones_and_the_new_one_with():
    import torch
    from dronesim_amd.sight import LineOfSight
    ctx, state, log = _fake()
    rel = torch.zeros((3, 3, 8))
    idx = torch.zeros((3, 8), dtype=torch.int32)
    plain = LineOfSight(ctx, state, None, 3, ground=True)
    assert plain.drones is False and plain._targets is None
    plain.query(rel, idx)
    assert log[0][0] == "dsim_line_of_sight" and len(log[0][1]) == 6 and log[0][1][:5] == (11, 22, 5, "view", None)
    for call in (plain.drones_outside, plain.refresh_drone_box):
        with pytest.raises(ValueError, match="drones=True"):
            call()
    tg = _Targets()
    tid = torch.zeros((8,), dtype=torch.uint8)
    los = LineOfSight(ctx, state, None, 3, drones=True, type_id=tid, targets=tg)          # no world but the drones
    assert los.drones is True and los.args.flags == 0
    s = los.query(rel, idx)
    name, a = log[1]
    assert name == "dsim_line_of_sight_drones" and len(a) == 8 and a[:5] == (11, 22, 5, "view", None)
    assert a[5]._obj is los.args and a[6] == tid.data_ptr() and a[7]._obj is tg.dr and tg.planned == 1
    assert los.args.rel == rel.data_ptr() and los.args.index == idx.data_ptr() and tuple(s.visible.shape) == (3, 5)
    los.query(rel, None, blocker=False)
    assert log[2][0] == "dsim_line_of_sight_drones" and los.args.index is None and los.args.blocker_out is None and tg.planned == 2
    assert los.drones_outside() == 7
    los.refresh_drone_box()
    assert tg.fresh == 1
    keep = los.graph_keepalive()
    assert all(x in keep for x in ("ws", "label", "count")) and any(x is tid for x in keep) and any(x is los.visible_out for x in keep)
    assert LineOfSight.seg_drone(np.array([-1, -2, -3, -10, 4])).tolist() == [-1, -1, 0, 7, -1]
    assert len(log) == 3


def test_host_validation():
    from dronesim_amd.sight import LineOfSight
    ctx, state, log = _fake()
    sig = inspect.signature(LineOfSight.__init__).parameters
    assert sig["drones"].default is False and sig["drone_box"].default is None and sig["type_id"].default is None
    with pytest.raises(ValueError, match="no world"):
        LineOfSight(ctx, state, None, 4)
    with pytest.raises(ValueError, match="without drones=True"):
        LineOfSight(ctx, state, None, 4, ground=True, drone_box=(0, 0, 1, 1))
    with pytest.raises(ValueError, match="drone_box must be"):
        LineOfSight(ctx, state, None, 4, drones=True, drone_box=(0, 0, 1), targets=_Targets())
    with pytest.raises(ValueError, match="drone_box must be"):
        LineOfSight(ctx, state, None, 4, drones=True, drone_box=(2, 0, 1, 1), targets=_Targets())
    with pytest.raises(ValueError, match="targets without"):
        LineOfSight(ctx, state, None, 4, ground=True, targets=_Targets())
    ctx2, state2, _ = _fake(n_types=2)
    with pytest.raises(ValueError, match="type_id is required"):
        LineOfSight(ctx2, state2, None, 4, drones=True, targets=_Targets())
    LineOfSight(ctx2, state2, None, 4, ground=True)                              # (without drones the types play no part)
    assert not log


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
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.envs.watches import StepWatches
    assert StepWatches._sight_drones is False and StepWatches._sight_box is None
    sig = inspect.signature(CtrlAviary.__init__).parameters
    assert sig["neighbor_sight_drones"].default is False and sig["neighbor_sight_drone_box"].default is None
    w = _options()
    assert w._sight_drones is False and w._sight_box is None
    knn = dict(neighbor_obs=4, neighbor_radius=2.0)
    w = _options(neighbor_sight=True, neighbor_sight_drones=True, **knn)         # open air: no world needed
    assert w._sight_on is True and w._sight_drones is True and w._sight_scene is None and w._sight_box is None
    w = _options(neighbor_sight=True, neighbor_sight_drones=True, neighbor_sight_drone_box=(0, -1, 2, 3), **knn)
    assert w._sight_box == (0.0, -1.0, 2.0, 3.0)
    gate = sr.gate()
    assert _options(neighbor_sight=True, neighbor_sight_drones=True, obstacle_watch=gate, **knn)._sight_drones is True
    with pytest.raises(ValueError, match="needs a world to look at"):            # the default keeps its refusal
        _options(neighbor_sight=True, **knn)
    with pytest.raises(ValueError, match="neighbor_sight_drones / neighbor_sight_drone_box without neighbor_sight=True"):
        _options(neighbor_sight_drones=True, **knn)
    with pytest.raises(ValueError, match="without neighbor_sight=True"):
        _options(neighbor_sight_drone_box=(0, 0, 1, 1), **knn)
    with pytest.raises(ValueError, match="neighbor_sight_drone_box without neighbor_sight_drones"):
        _options(neighbor_sight=True, obstacle_watch=gate, neighbor_sight_drone_box=(0, 0, 1, 1), **knn)
    with pytest.raises(ValueError, match="drone_box must be"):
        _options(neighbor_sight=True, neighbor_sight_drones=True, neighbor_sight_drone_box=(0, 0, np.inf, 1), **knn)
    with pytest.raises(ValueError, match="neighbor_sight=True without neighbor_obs"):
        _options(neighbor_sight=True, neighbor_sight_drones=True)


def test_env_refusals_before_a_context_is_made():
    from dronesim_amd.envs import CtrlAviary, VelocityAviary
    kw = dict(initial_xyzs=np.zeros((4, 3)), dict_io=False)
    for cls in (CtrlAviary, VelocityAviary):
        with pytest.raises(ValueError, match="without neighbor_sight=True"):
            cls(["tello"], 4, neighbor_obs=2, neighbor_radius=1.0, neighbor_sight_drones=True, **kw)
        with pytest.raises(ValueError, match="neighbor_sight=True without neighbor_obs"):
            cls(["tello"], 4, neighbor_sight=True, neighbor_sight_drones=True, **kw)
        with pytest.raises(ValueError, match="neighbor_sight_drone_box without neighbor_sight_drones"):
            cls(["tello"], 4, neighbor_obs=2, neighbor_radius=1.0, neighbor_sight=True, obstacle_watch=sr.gate(),
                neighbor_sight_drone_box=(0, 0, 1, 1), **kw)


def test_the_walks_hook_leaves_the_camera_and_the_scanner_their_sphere_test():
    """dsim_camera_drones.inc calls its sphere test through CD_SPHERE, which is cam_sphere on the walk's own names unless the
    includer says otherwise; only line of sight does, and the camera and the scanner define nothing of the kind."""
    src = lambda f: open(os.path.join(ROOT, "dronesim_amd", "csrc", f)).read()
    inc = src("dsim_camera_drones.inc")
    assert "#define CD_SPHERE(p, idx, k) cam_sphere(p, idx, k, own, wx, wy, wz, dx, dy, dz, inv_a, near, tmax, best, body)" in inc
    assert inc.count("CD_SPHERE(g.sorted[k], g.sidx, k);") == 1 and inc.count("CD_SPHERE(g.outside[k], g.outside_idx, k);") == 1
    assert "#undef CD_SPHERE" in inc and inc.count("cam_sphere(") == 1
    assert "CD_SPHERE" not in src("dsim_camera.hip") and "CD_SPHERE" not in src("dsim_scan.hip")
    assert src("dsim_sight.hip").count("#define CD_SPHERE(p, idx, k) sight_sphere(") == 1
