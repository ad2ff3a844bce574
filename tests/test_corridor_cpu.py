"""CPU-side checks of corridor clearance (dsim_corridor_clearance, corridor.Corridor, the env's corridor keyword): the ABI surface,
corridor_reach, the Python class through a recording stand-in for the library, the tests' own fp64 reference (tests/corridor_ref.py)
against dense sampling of the segment, and the env's validation.  tests/README_corridor.md."""
import ctypes
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest

import __graft_entry__ as graft
from dronesim_amd import params
from tests import scenes_ref as sr
from tests.corridor_ref import GROUND, corridor_brute, ground_dist, pieces
from tests.obstacle_ref import tri_dist
from tests.sweep_ref import chords, sweep_brute

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
    minor = hdr[hdr.index("#define DSIM_ABI_MINOR"):hdr.index("#define DSIM_MAX_ACT")]
    m = re.search(r"^int\s+dsim_corridor_clearance\s*\(([^;]*)\);", hdr, flags=re.M | re.S)
    assert m and m.group(1).count(",") + 1 == 6 == len(lib.dsim_corridor_clearance.argtypes)
    assert lib.dsim_corridor_clearance.argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, nat.View, ctypes.c_void_p,
                                                    ctypes.POINTER(nat.CorridorArgs)]
    assert "dsim_corridor_clearance" in minor and "dsim_corridor_clearance" in nat.EXPORTS
    assert lib.dsim_abi_version() == 11 and lib.dsim_abi_minor() == 1          # only new functions: the number stands
    assert nat.CORRIDOR_GROUND == 1 and nat.CORRIDOR_MAX_K == 32 and nat.CORRIDOR_MAX_PIECES == 32
    assert os.path.join(ROOT, "dronesim_amd", "csrc", "dsim_corridor.hip") in graft.HIP_DEPS and len(graft.HIP_SRCS) == 6
    fields = ["rel", "index", "k", "flags", "offset", "type_id", "scenes", "scene_id", "margin", "sag", "clearance_out", "body_out",
              "unserved_out"]
    assert [f for f, _ in nat.CorridorArgs._fields_] == fields
    lines = ['printf("size %zu\\n", sizeof(dsim_corridor_args));', 'printf("ground %d\\n", (int)DSIM_CORRIDOR_GROUND);',
             'printf("seg_ground %d\\n", (int)DSIM_SEG_GROUND);']
    lines += [f'printf("{f} %zu\\n", offsetof(dsim_corridor_args, {f}));' for f in fields]
    src = tmp_path / "corridor.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dronesim_amd.h"\n'
                   "int main(void) {\n"
                   "int (*f)(dsim_ctx*, void*, int64_t, dsim_view, const dsim_obstacles*, const dsim_corridor_args*) = dsim_corridor_clearance;\n"
                   + "\n".join(lines) + "\nreturn f != 0 ? 0 : 1; }\n")
    obj = tmp_path / "corridor.o"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o", str(obj), str(src)])
    exe = tmp_path / "corridor"
    subprocess.check_call(["gcc", "-o", str(exe), str(obj), nat.LIB_PATH, f"-Wl,-rpath,{os.path.dirname(nat.LIB_PATH)}",
                           "-Wl,--unresolved-symbols=ignore-in-shared-libs"])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(nat.CorridorArgs) == 88
    assert int(got["ground"]) == nat.CORRIDOR_GROUND and int(got["seg_ground"]) == GROUND == nat.SEG_GROUND
    for f in fields:
        assert int(got[f]) == getattr(nat.CorridorArgs, f).offset, f


def test_library_refuses_null_arguments_before_it_touches_a_device(nat):
    lib = nat.load()
    a = nat.CorridorArgs()
    assert lib.dsim_corridor_clearance(None, None, 1, nat.View(), None, None) == -1
    assert lib.dsim_corridor_clearance(None, None, 1, nat.View(), None, ctypes.byref(a)) == -1


# ---- host arithmetic ---------------------------------------------------------------------------------------------------------------
def test_corridor_reach_is_sweep_reach():
    from dronesim_amd.obstacles import corridor_reach, sweep_reach
    types_ = [params.builtin_type(k) for k in ("robobee", "tello", "hexa_6DOF")]
    for margin, sag, piece in ((1.0, 0.0, 0.25), (0.6, 0.01, 0.5), (0.25, 5e-4, 3.0)):
        assert corridor_reach(types_, margin, sag, piece) == sweep_reach(types_, margin, sag, piece)
        assert corridor_reach(types_[:1], margin, sag, piece) == sweep_reach(types_[:1], margin, sag, piece)


# ---- the Python class, through a recording stand-in for the library ----------------------------------------------------------------------
class _Lib:
    def __init__(self, log):
        self._log = log

    def __getattr__(self, name):
        def call(*a):
            self._log.append((name, a))
            return 0
        return call


def _fake(n=5, n_pad=8, n_types=1):
    import torch
    log = []
    ctx = types.SimpleNamespace(lib=_Lib(log), handle=11, stream_ptr=lambda: 22, device=torch.device("cpu"),
                                types=[params.builtin_type("robobee")] * n_types)
    state = types.SimpleNamespace(n=n, n_pad=n_pad, view=lambda: "view")
    return ctx, state, log


def test_fan_shapes_and_the_query_call():
    import torch
    from dronesim_amd.corridor import Corridor, CorridorClearance
    ctx, state, log = _fake()
    cor = Corridor(ctx, state, None, 3, 0.5, sag=0.01, ground=True)
    assert cor.max_length == float("inf") and cor.args.flags == 1 and cor.args.k == 3
    assert cor.args.margin == np.float32(0.5) and cor.args.sag == np.float32(0.01)
    dirs = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.6, -0.8]])
    rel = cor.fan(dirs, 2.0)
    assert tuple(rel.shape) == (3, 3, 8) and rel.dtype == torch.float32 and rel.is_contiguous()
    assert np.array_equal(rel[:, :, 0].numpy(), (2.0 * dirs).astype(np.float32)) and bool((rel == rel[:, :, :1]).all())
    assert float(cor.fan(dirs, 0.0).abs().max()) == 0.0
    for bad in (dirs[:2], np.full((3, 3), np.nan)):
        with pytest.raises(ValueError, match="directions"):
            cor.fan(bad, 1.0)
    with pytest.raises(ValueError, match="length"):
        cor.fan(dirs, -1.0)
    out = cor.query(rel)
    name, a = log[0]
    assert name == "dsim_corridor_clearance" and len(a) == 6 and a[:5] == (11, 22, 5, "view", None) and a[5]._obj is cor.args
    assert isinstance(out, CorridorClearance) and tuple(out.clearance.shape) == (3, 5) == tuple(out.body.shape)
    assert cor.args.rel == rel.data_ptr() and cor.args.index is None and cor.args.body_out == cor.body_out.data_ptr()
    idx = torch.zeros((3, 8), dtype=torch.int32)
    out = cor.query(rel[:, :, :5], idx, body=False)                  # (the first n drones, cut from a padded tensor)
    assert out.body is None and cor.args.body_out is None and cor.args.index == idx.data_ptr()
    with pytest.raises(ValueError, match="rel must be"):
        cor.query(torch.zeros((3, 3, 5)))                            # (not cut from a padded tensor: another stride)
    with pytest.raises(ValueError, match="index must be"):
        cor.query(rel, idx.long())
    assert cor.unserved() == 0 and len(log) == 2
    assert any(x is cor.clearance_out for x in cor.graph_keepalive())
    cor.close()
    assert cor.clearance_out is None


def test_host_validation():
    from dronesim_amd.corridor import Corridor
    ctx, state, log = _fake()
    for k in (0, 33, 2.5, True):
        with pytest.raises(ValueError, match="k must be"):
            Corridor(ctx, state, None, k, 0.5, ground=True)
    for margin in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="margin"):
            Corridor(ctx, state, None, 4, margin, ground=True)
    for sag in (-0.1, np.inf, np.nan):
        with pytest.raises(ValueError, match="sag"):
            Corridor(ctx, state, None, 4, 0.5, sag=sag, ground=True)
    with pytest.raises(ValueError, match="no world at all"):
        Corridor(ctx, state, None, 4, 0.5)
    with pytest.raises(TypeError, match="world takes"):
        Corridor(ctx, state, sr.gate(), 4, 0.5)                      # (a host set: it must already be on the device)
    with pytest.raises(ValueError, match="scene_id without"):
        Corridor(ctx, state, None, 4, 0.5, ground=True, scene_id=np.zeros(5, dtype=np.int64))
    ctx2, state2, _ = _fake(n_types=2)
    with pytest.raises(ValueError, match="type_id is required"):
        Corridor(ctx2, state2, None, 4, 0.5, ground=True)
    assert not log


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def test_reference_against_dense_sampling():
    """200 gate segments, 401 samples each: the reference is never above the sampled minimum and within one sample spacing of it;
    and it is the swept watch's reference read the other way round."""
    s = sr.gate()
    rng = np.random.default_rng(171)
    q0, q1 = chords(rng, 200, [-0.55, -1.05, -0.9], [0.55, 1.05, 0.9], 0.0, 0.8)
    pos, rel = q0.astype(np.float32), (q1 - q0).astype(np.float32)
    R = np.float32(params.builtin_type("robobee").collision_sphere)
    rad = np.full(200, R)
    ref = corridor_brute(pos, rel.T[None], rad, 9.0, tri32=s.triangles, body=s.body)
    assert ref["served"].all() and ref["clr"].shape == (1, 200)
    c = ref["raw"][0] + float(R)
    e, d = pos.astype(np.float64), rel.astype(np.float64)
    w = np.linspace(0.0, 1.0, 401)
    pts = e[:, None, :] + w[None, :, None] * d[:, None, :]
    sampled = tri_dist(pts.reshape(-1, 3), s.triangles).min(1).reshape(200, 401).min(1)
    length = np.linalg.norm(d, axis=1)
    print(f"reference vs 401 samples per segment: {int((c == 0).sum())} segments pierce, worst sampled - reference "
          f"{(sampled - c).max():.3e} m, worst reference - sampled {(c - sampled).max():.3e} m")
    assert (c == 0).sum() >= 5
    assert np.all(c <= sampled + 1e-12)                            # never above the sampled minimum
    assert np.all(sampled - c <= length / 400 + 1e-12)             # and within one sample spacing of it
    far = (e + d).astype(np.float32)                               # the swept watch's reference on the chord far end -> pos
    sw = sweep_brute(far, pos, s.triangles, s.body, rad, 9.0)
    assert np.abs(sw[4] - ref["raw"][0]).max() < 1e-6              # (e + d is rounded to float32 there, not here)


def test_reference_half_space_statuses_and_bodies():
    e = np.array([[0.0, 0.0, 0.5], [0.0, 0.0, 0.5], [0.0, 0.0, 0.5], [0.0, 0.0, -0.2], [0.0, 0.0, 2.0]])
    d = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -0.3], [0.0, 1.0, -0.9], [0.0, 0.0, 1.0], [1.0, 0.0, 0.5]])
    assert np.allclose(ground_dist(e, d), [0.5, 0.2, 0.0, 0.0, 2.0])
    pos, rel = e.astype(np.float32), d.astype(np.float32).T[None]
    rad = np.full(5, np.float32(0.1))
    ref = corridor_brute(pos, rel, rad, 1.0, sag=0.05, ground=True)
    rs = float(np.float32(0.1)) + float(np.float32(0.05))
    assert np.allclose(ref["clr"][0], [0.5 - rs, 0.2 - rs, -rs, -rs, 1.0], atol=1e-7)
    assert ref["body"][0].tolist() == [GROUND, GROUND, GROUND, GROUND, -1]
    # statuses: a negative index, a NaN in the position or in rel, and a slot that needs more than 32 pieces
    rel2 = np.repeat(rel, 2, 0).copy()
    rel2[1, 0, 0] = np.nan
    pos2 = pos.copy()
    pos2[4, 1] = np.nan
    idx = np.zeros((2, 5), dtype=np.int32)
    idx[0, 1] = -1
    rel2[0, :, 2] = [0.0, 33 * 2 * 0.25, 0.0]
    ref = corridor_brute(pos2, rel2, rad, 1.0, ground=True, index=idx, half=0.25)
    assert ref["evaluated"].tolist() == [[True, False, True, True, False], [False, True, True, True, False]]
    assert ref["served"].tolist() == [[True, False, False, True, False], [False, True, True, True, False]]
    assert np.all(np.isneginf(ref["clr"][~ref["served"]])) and np.all(ref["body"][~ref["served"]] == -1)
    assert pieces(np.array([0.0, 0.4, 0.5, 16.0, 16.1]), 0.25).tolist() == [1, 1, 2, 33, 33]
    assert pieces(np.array([1e9]), np.inf).tolist() == [1]
    # two bodies: the nearer wins, the gap is the difference of their minima
    tri = np.array([[[0, -1, 1], [0, 1, 1], [0, 0, 3]], [[2, -1, 1], [2, 1, 1], [2, 0, 3]]], dtype=np.float32)
    ref = corridor_brute(np.array([[0.5, 0.0, 1.5]], dtype=np.float32), np.array([[[0.25], [0.0], [0.0]]], dtype=np.float32),
                         np.array([np.float32(0.1)]), 5.0, tri32=tri, body=np.array([0, 1]), ground=True)
    assert ref["body"][0, 0] == 0 and abs(ref["raw"][0, 0] - (0.5 - float(np.float32(0.1)))) < 1e-12
    assert abs(ref["gap"][0, 0] - 0.75) < 1e-12


# ---- the env's keyword ------------------------------------------------------------------------------------------------------------------
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


def test_env_keyword_has_a_default_and_is_checked():
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.envs.watches import StepWatches
    assert StepWatches._corr_opts is None and StepWatches._corr is None
    assert inspect.signature(CtrlAviary.__init__).parameters["corridor"].default is None
    gate = sr.gate()
    # an env without corridor constructs exactly the keywords it did: nothing of the corridor's is set
    for w in (_options(), _options(obstacle_watch=gate)):
        assert w._corr_opts is None and "_corr_opts" not in vars(w) and "_corr" not in vars(w)
    w = _options(obstacle_watch=gate, obstacle_margin=0.75, corridor=dict(k=4, piece=0.5))
    assert w._corr_opts == dict(k=4, piece=0.5, sag=0.0, margin=0.75, ground=False)
    w = _options(obstacle_watch=gate, corridor=dict(k=32, piece=1, sag=0.01, margin=2.0, ground=True))
    assert w._corr_opts == dict(k=32, piece=1.0, sag=0.01, margin=2.0, ground=True)
    with pytest.raises(ValueError, match="corridor without obstacle_watch"):
        _options(corridor=dict(k=4, piece=0.5))
    for bad in (dict(k=0, piece=0.5), dict(k=33, piece=0.5), dict(k=2.5, piece=0.5), dict(k=True, piece=0.5)):
        with pytest.raises(ValueError, match="k must be"):
            _options(obstacle_watch=gate, corridor=bad)
    for piece in (0.0, -1.0, np.inf, np.nan, 1e-4):
        with pytest.raises(ValueError, match="piece must be"):
            _options(obstacle_watch=gate, corridor=dict(k=4, piece=piece))
    for sag in (-0.01, np.inf, np.nan):
        with pytest.raises(ValueError, match="sag must be"):
            _options(obstacle_watch=gate, corridor=dict(k=4, piece=0.5, sag=sag))
    with pytest.raises(ValueError, match="margin must be"):
        _options(obstacle_watch=gate, corridor=dict(k=4, piece=0.5, margin=0.0))
    with pytest.raises(ValueError, match="unknown keys"):
        _options(obstacle_watch=gate, corridor=dict(k=4, piece=0.5, length=3.0))
    for bad in (4, dict(k=4), dict(piece=0.5)):
        with pytest.raises(ValueError, match="corridor takes a dict"):
            _options(obstacle_watch=gate, corridor=bad)


def test_env_refusals_before_a_context_is_made():
    from dronesim_amd.envs import CtrlAviary, VelocityAviary
    kw = dict(initial_xyzs=np.zeros((4, 3)), dict_io=False)
    for cls in (CtrlAviary, VelocityAviary):
        with pytest.raises(ValueError, match="corridor without obstacle_watch"):
            cls(["robobee"], 4, corridor=dict(k=4, piece=0.5), **kw)
        with pytest.raises(ValueError, match="k must be"):
            cls(["robobee"], 4, obstacle_watch=sr.gate(), corridor=dict(k=40, piece=0.5), **kw)
