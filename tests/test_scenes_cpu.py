"""CPU-side checks of obstacle scenes (ObstacleScenes, dsim_scenes_create, dsim_obstacle_clearance_scenes, dsim_depth_image_scenes):
the host data model and its limits, the records against obstacles._rot, flatten, the two routes of the reference, the recorded
float32 errors the GPU tolerances come from, the input conditions of the GPU cases, the ABI names, and every refusal that needs no
device (tests/README_scenes.md)."""
import os
import re
import types

import numpy as np
import pytest

import __graft_entry__ as graft
from tests import camera_ref as cr
from tests import scenes_ref as sr
from tests.obstacle_ref import brute

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nat():
    graft.build()
    from dronesim_amd import _native
    return _native


def _scenes(K=4, G=3, count=None, seed=0):
    from dronesim_amd.obstacles import ObstacleScenes
    pos, rpy = sr.random_placements(np.random.default_rng(seed), K, G)
    return ObstacleScenes(sr.gate(), pos, rpy, count)


# ---- the data model --------------------------------------------------------------------------------------------------------------
def test_validation_and_limits():
    from dronesim_amd.obstacles import ObstacleScenes
    g = sr.gate()
    z = lambda K, G: np.zeros((K, G, 3))
    s = ObstacleScenes(g, z(2, 32), z(2, 32))
    assert (s.K, s.G, s.n_bodies) == (2, 32, 1) and s.count.tolist() == [32, 32]
    with pytest.raises(ValueError, match="G"):
        ObstacleScenes(g, z(2, 33), z(2, 33))
    with pytest.raises(ValueError):
        ObstacleScenes(g, np.zeros((2, 0, 3)), np.zeros((2, 0, 3)))
    with pytest.raises(ValueError, match=r"2\^22"):
        ObstacleScenes(g, z((1 << 22) // 32 + 1, 32), z((1 << 22) // 32 + 1, 32))
    assert ObstacleScenes(g, z(1 << 20, 4), z(1 << 20, 4)).K == 1 << 20          # K G = 2^22 itself is served
    with pytest.raises(ValueError, match="K, G, 3"):
        ObstacleScenes(g, z(2, 3), np.zeros((2, 3)))
    with pytest.raises(ValueError, match="K, G, 3"):
        ObstacleScenes(g, np.zeros((6, 3)), np.zeros((6, 3)))
    for bad in (np.nan, np.inf):
        p = z(2, 3)
        p[1, 2, 0] = bad
        with pytest.raises(ValueError, match="finite"):
            ObstacleScenes(g, p, z(2, 3))
        with pytest.raises(ValueError, match="finite"):
            ObstacleScenes(g, z(2, 3), p)
        assert ObstacleScenes(g, p, z(2, 3), [3, 2]).count.tolist() == [3, 2]    # ... unless the slot is not used
    for count in ([3], [3, 4], [-1, 0], [1.0, 2.0], [[1, 2]]):
        with pytest.raises(ValueError, match="count"):
            ObstacleScenes(g, z(2, 3), z(2, 3), count)
    assert ObstacleScenes(g, z(2, 3), z(2, 3), [0, 0]).count.tolist() == [0, 0]  # a scene may be empty
    with pytest.raises(TypeError):
        ObstacleScenes(g.triangles, z(2, 3), z(2, 3))
    with pytest.raises(ValueError, match="float32"):
        ObstacleScenes(g, np.full((1, 1, 3), 1e39), z(1, 1))


def test_records_are_rot_row_major_then_position():
    from dronesim_amd.obstacles import ObstacleSet, _rot
    s = _scenes(K=5, G=4, count=[4, 0, 1, 3, 2], seed=3)
    assert s.place.shape == (5, 4, 12) and s.place.dtype == np.float32
    for k in range(5):
        for g in range(4):
            if g < s.count[k]:
                # (one float32 ulp of 1: the constructor takes the sines and cosines of all slots at once)
                assert np.abs(s.place[k, g, :9] - _rot(s.rpy[k, g]).ravel()).max() <= 2.0 ** -24
                assert np.array_equal(s.place[k, g, 9:], s.position[k, g].astype(np.float32))
            else:
                assert np.isnan(s.place[k, g]).all()
    # the convention of ObstacleSet.from_urdf(path, position, rpy): the placed gate is the gate loaded at that pose
    urdf = os.path.join(sr.GOLDEN, "gate_50_curved.urdf")
    want = ObstacleSet.from_urdf(urdf, s.position[3, 1], s.rpy[3, 1]).triangles.astype(np.float64)
    R, t = sr.placement64(s, 3, 1)
    got = sr.gate().triangles.astype(np.float64) @ R.T + t
    assert np.abs(got - want).max() < 1e-6                         # (float32 R, t and vertices against fp64 ones, rounded once)


def test_flatten_is_the_placed_union_instance_major():
    from dronesim_amd.obstacles import ObstacleScenes
    two = sr.gate() + sr.gate().__class__.box((0.0, 0.0, 1.0), (0.2, 0.2, 0.2))
    assert two.n_bodies == 2
    pos, rpy = sr.random_placements(np.random.default_rng(5), 3, 3)
    s = ObstacleScenes(two, pos, rpy, [3, 0, 2])
    f = s.flatten(2)
    assert f.n_tri == 2 * two.n_tri and f.n_bodies == 4
    assert f.body.tolist() == two.body.tolist() + (two.body + 2).tolist()
    tri, body = sr.placed_triangles(s, 2)
    assert np.array_equal(f.triangles, tri.astype(np.float32)) and np.array_equal(f.body, body)
    assert s.flatten(0).n_tri == 3 * two.n_tri
    with pytest.raises(ValueError, match="empty"):
        s.flatten(1)
    with pytest.raises(ValueError):
        s.flatten(3)


# ---- the reference -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["gates", "ragged", "soup"])
def test_the_two_routes_of_the_reference_agree(case):
    """Transform the point into the placement's frame, or the triangles into the task's: with an orthonormal R (the fp64 rotation of
    the scene's rpy) the clearances agree to 1e-12 and the nearest instances are the same.  With the device's float32 R, orthonormal
    to 6e-8 only, placing triangles is not quite an isometry: the routes then differ by that relative amount."""
    d = {"gates": lambda: sr.case_gates(True), "ragged": sr.case_ragged, "soup": sr.case_soup}[case]()
    args = (d["pos"], d["scenes"], d["scene_id"], d["rad"], d["margin"], d["off"])
    a, b = sr.brute_scenes(*args, exact=True), sr.brute_scenes_by_triangles(*args, exact=True)
    fin = np.isfinite(a["raw"])
    assert np.array_equal(fin, np.isfinite(b["raw"])) and fin.sum() > 0.5 * len(fin)
    assert np.abs(a["raw"][fin] - b["raw"][fin]).max() <= 1e-12
    assert np.array_equal(a["near"], b["near"]) and a["contacts"] == b["contacts"]
    # R32 = Q + E with Q orthonormal and |E| <= 9 x 2^-25 (nine entries rounded to float32): a distance between a placed vertex
    # R32 x + t and q differs from the one between x and R32^T (q - t) by at most 2 |E| (|x| + |q - t|)
    b32 = sr.brute_scenes_by_triangles(*args)
    scale = np.abs(d["scenes"].prototype.triangles).sum(-1).max() + 2.0 * 16.0 * np.sqrt(3.0)
    assert np.abs(d["ref"]["raw"][fin] - b32["raw"][fin]).max() <= 2.0 * 9.0 * 2.0 ** -25 * scale


def test_identity_scene_is_the_unplaced_reference():
    from dronesim_amd.obstacles import ObstacleScenes
    s = ObstacleScenes(sr.gate(), np.zeros((1, 1, 3)), np.zeros((1, 1, 3)))
    assert np.array_equal(s.place[0, 0], np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=np.float32))
    p = np.random.default_rng(1).uniform(-1.0, 1.0, (300, 3)).astype(np.float32)
    rad = np.full(300, np.float32(0.06))
    a = sr.brute_scenes(p, s, np.zeros(300, dtype=int), rad, 1.0)
    b = brute(p, sr.gate().triangles, sr.gate().body, rad, 1.0)
    assert np.array_equal(a["clr"], b[0]) and np.array_equal(a["near"], b[1]) and a["contacts"] == b[3]


def test_restated_clearance_error_is_what_is_recorded():
    """The float32 restatement of the placed query against the fp64 reference on the GPU cases' own inputs, over the drones whose
    clearance the device reports (c < margin): its worst |c32 - c64| is the recorded RESTATED_WORST (not above it, and the record is
    not padded); the kernel is granted 4 x it, which stays below GUARD / 4."""
    worst = 0.0
    for d in (sr.case_gates(False), sr.case_gates(True), sr.case_ragged(), sr.case_soup()):
        c32 = sr.restated_scenes(d["pos"], d["scenes"], d["scene_id"], d["rad"], d["off"])
        m = d["ref"]["raw"] < d["margin"]
        assert np.array_equal(c32[m] < d["margin"], np.ones(int(m.sum()), bool))        # (the guard band: the same side of the margin)
        assert np.array_equal(c32[m] < 0, d["ref"]["raw"][m] < 0)
        worst = max(worst, float(np.abs(c32[m] - d["ref"]["raw"][m]).max()))
    print(f"restated worst {worst:.3e} m")
    assert worst <= sr.RESTATED_WORST <= 1.02 * worst, worst
    assert sr.ATOL == 4.0 * sr.RESTATED_WORST and sr.ATOL <= sr.GUARD / 4 and sr.GUARD == 1e-4


def test_float32_transform_moves_the_local_point_little():
    """Subtract, then rotate, in float32 against fp64: at |q| <= 8 m the local point moves by a few 1e-6 m (the issue measured
    1.9e-6); with offsets of 128 m subtracted first nothing more is lost, whereas R^T q - R^T t at the stored magnitudes would be."""
    rng = np.random.default_rng(9)
    s = _scenes(K=64, G=3, seed=9)
    q = rng.uniform(-8.0, 8.0, (4096, 3)).astype(np.float32)
    P = s.place[np.arange(4096) % 64, 0]
    d = q - P[:, 9:]
    l32 = np.stack([P[:, k] * d[:, 0] + P[:, 3 + k] * d[:, 1] + P[:, 6 + k] * d[:, 2] for k in range(3)], 1)
    assert l32.dtype == np.float32
    P64 = P.astype(np.float64)
    l64 = np.einsum("nji,nj->ni", P64[:, :9].reshape(-1, 3, 3), q.astype(np.float64) - P64[:, 9:])
    assert np.linalg.norm(l32 - l64, axis=1).max() < 4e-6


# ---- the input conditions of the GPU cases, on the reference alone ---------------------------------------------------------------
@pytest.mark.parametrize("offsets", [False, True])
def test_conditions_of_the_placed_gates_case(offsets):
    d = sr.case_gates(offsets)
    r, n = d["ref"], len(d["scene_id"])
    s = d["scenes"]
    assert (s.K, s.G, n, s.prototype.n_tri, s.n_bodies, d["margin"]) == (64, 3, 2048, 96, 1, 0.5)
    assert np.array_equal(d["scene_id"], np.arange(n) % 64)
    assert d["redrawn"] <= 0.01 and sr.tie_fraction(r) <= 0.01
    assert int((r["n_near"] >= 2).sum()) >= 20                     # drones within the margin of two or more placements
    assert r["contacts"] >= 0.01 * n
    assert 0.1 < (r["near"] >= 0).mean() < 0.5 and set(r["near"][r["near"] >= 0]) == {0, 1, 2}
    c = r["raw"]
    assert not ((np.abs(c) < sr.GUARD) | (np.abs(c - d["margin"]) < sr.GUARD)).any()
    if offsets:
        assert np.abs(d["off"]).max() > 100.0 and np.abs(d["pos"] - d["off"]).max() < 8.0


def test_conditions_of_the_ragged_case():
    d = sr.case_ragged()
    r, sid, s = d["ref"], d["scene_id"], d["scenes"]
    assert s.count.tolist() == [0, 1, 2, 3, 8] and s.G == 8 and len(sid) == 300
    assert set(sid) == {-1, 0, 1, 2, 3, 4, 5}
    none = (sid < 1) | (sid >= 5)                                  # out of range, or the empty scene
    assert none.sum() > 60 and np.all(r["near"][none] == -1) and np.all(r["clr"][none] == d["margin"])
    assert d["redrawn"] <= 0.01 and sr.tie_fraction(r) <= 0.01
    assert (r["near"] >= 0).sum() >= 20 and r["contacts"] >= 3 and r["near"].max() >= 4      # a slot beyond G = 3 of the others
    for k in range(1, 5):                                          # nobody names a slot at or above its scene's count
        assert r["near"][sid == k].max() < s.count[k]


def test_conditions_of_the_soup_case():
    d = sr.case_soup()
    r, s = d["ref"], d["scenes"]
    assert (s.prototype.n_tri, s.n_bodies, s.K, s.G, len(d["scene_id"])) == (3000, 4, 4, 2, 512)
    assert d["redrawn"] <= 0.01 and sr.tie_fraction(r) <= 0.01
    assert r["contacts"] > 10 and set(r["near"][r["near"] >= 0]) == set(range(8))            # both slots, all four bodies
    assert int((r["n_near"] >= 2).sum()) >= 20


def test_conditions_of_the_camera_case():
    st, (pos, quat), off, arms, sid = sr.camera_fleet()
    assert len(sr.CAMERAS) == 6 and [sid[c] for c in sr.CAMERAS] == list(sr.CAMERA_SCENE) and (sid >= 0).sum() == 6
    for subdiv, n_tri in ((0, 108), (2, 1548)):
        s = sr.camera_scenes(subdiv)
        assert (s.K, s.G, s.prototype.n_tri, s.n_bodies) == (3, 3, n_tri, 2)
    for res in ((64, 48), (17, 17)):
        seen = set()
        for k, pair in enumerate(sr.reference_images(0, res)):
            for ref in pair:
                assert ref["ambiguous"].mean() <= 0.01, (res, k)
                seen |= set(np.unique(ref["seg"]))
        assert seen >= {-2, -1, 0, 1, 2, 3, 4, 5}                  # every instance of G = 3 x two bodies is in view somewhere
    first_behind, last_behind = sr.carry_pixels()
    assert first_behind.sum() >= 20 and last_behind.sum() >= 10    # `best` must carry both ways across placements


def test_restated_image_error_is_what_is_recorded():
    """The float32 restatement of the placed image against camera_ref.cast on the placed union, over the GPU case's own images
    (both sets, both resolutions, the six cameras): its worst |t - t_ref| max(|n . d|, 0.05) / t_ref is the recorded
    IMAGE_RESTATED_WORST; outside the ambiguity mask it hits exactly the pixels the reference hits."""
    _, (pos, quat), _, arms, _ = sr.camera_fleet()
    worst = 0.0
    for subdiv in (0, 2):
        s = sr.camera_scenes(subdiv)
        for res in ((64, 48), (17, 17)):
            for k, L in enumerate(arms):
                ref = sr.reference_images(subdiv, res)[k][0]
                t32 = sr.restated_placed_image(s, sr.CAMERA_SCENE[k], pos[k], quat[k], L, res[0], res[1])
                assert not ((np.isfinite(t32) != np.isfinite(ref["t"])) & ~ref["ambiguous"]).any()
                worst = max(worst, cr.t_error(t32, ref))
    print(f"restated image worst {worst:.3e}")
    assert worst <= sr.IMAGE_RESTATED_WORST <= 1.02 * worst, worst
    assert sr.IMAGE_TOL == 4.0 * sr.IMAGE_RESTATED_WORST


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
NEW = {"dsim_scenes_create": 7, "dsim_scenes_destroy": 2, "dsim_obstacle_clearance_scenes": 12, "dsim_depth_image_scenes": 12}


def test_header_declares_and_library_exports_the_scenes(nat):
    hdr = open(os.path.join(ROOT, "include", "dronesim_amd.h")).read()
    lib = nat.load()
    for f, n_args in NEW.items():
        m = re.search(rf"^int\s+{f}\s*\(([^;]*)\);", hdr, flags=re.M | re.S)
        assert m, f
        assert m.group(1).count(",") + 1 == n_args == len(getattr(lib, f).argtypes), f
        assert f in nat.EXPORTS
        assert f.replace("dsim_scenes_destroy", "_destroy") in hdr[hdr.index("#define DSIM_ABI_MINOR"):hdr.index("#define DSIM_MAX_ACT")]
    assert re.search(r"typedef struct dsim_scenes dsim_scenes;", hdr)
    assert re.search(r"#define DSIM_ABI_VERSION 11\b", hdr) and re.search(r"#define DSIM_ABI_MINOR 1\b", hdr)
    assert lib.dsim_abi_version() == 11 and lib.dsim_abi_minor() == 1
    for f in ("dsim_scenes.hip", "dsim_camera_walk.inc"):
        assert os.path.join(ROOT, "dronesim_amd", "csrc", f) in graft.HIP_DEPS


def test_library_refuses_null_arguments_before_it_touches_a_device(nat):
    """Every new entry point checks its pointers first: DSIM_E_ARG with nothing dereferenced (no context exists on this machine)."""
    import ctypes
    lib = nat.load()
    h = ctypes.c_void_p()
    place = np.zeros((1, 1, 12), dtype=np.float32)
    assert lib.dsim_scenes_create(None, None, place.ctypes.data, None, 1, 1, ctypes.byref(h)) == -1 and not h
    assert lib.dsim_scenes_destroy(None, None) == 0
    v = nat.View()
    assert lib.dsim_obstacle_clearance_scenes(None, None, 1, v, None, None, None, None, 0.5, None, None, None) == -1
    assert lib.dsim_depth_image_scenes(None, None, v, None, None, None, 1, None, None, None, None, None) == -1


# ---- argument validation of the Python surfaces, through a stub ---------------------------------------------------------------------
class _Lib:
    def __init__(self, log):
        self._log = log

    def __getattr__(self, name):
        def call(*a):
            self._log.append((name, a))
            return 0
        return call


def test_query_scenes_hands_the_library_what_it_was_given():
    import torch
    from dronesim_amd import obstacles as obs
    log = []
    ctx = types.SimpleNamespace(lib=_Lib(log), handle=11, stream_ptr=lambda: 22)
    state = types.SimpleNamespace(n=5, view=lambda: "view")
    dev = types.SimpleNamespace(handle=33)
    clr, near, ids = torch.zeros(8), torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.int32)
    off, tid, cnt = torch.zeros((3, 8)), torch.zeros(8, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64)
    obs.query_scenes(ctx, state, dev, ids, 0.5, clr, near, off, tid, cnt)
    obs.query_scenes(ctx, state, dev, ids, 0.25, clr, None)
    assert log[0] == ("dsim_obstacle_clearance_scenes", (11, 22, 5, "view", 33, ids.data_ptr(), off.data_ptr(), tid.data_ptr(), 0.5,
                                                         clr.data_ptr(), near.data_ptr(), cnt.data_ptr()))
    assert log[1] == ("dsim_obstacle_clearance_scenes", (11, 22, 5, "view", 33, ids.data_ptr(), None, None, 0.25, clr.data_ptr(), None, None))
    with pytest.raises(ValueError, match="scene_id"):
        obs.query_scenes(ctx, state, dev, None, 0.5, clr, near)
    assert len(log) == 2


def test_scene_ids_go_into_storage_order():
    import torch
    from dronesim_amd import obstacles as obs
    ids = np.array([5, -1, 7, 2, 9])
    t = obs.scene_ids_tensor(ids, 5, 8, torch.device("cpu"))
    assert t.dtype == torch.int32 and t.tolist() == [5, -1, 7, 2, 9, -1, -1, -1]
    order = types.SimpleNamespace(to_storage_np=lambda a: np.take(a, [3, 0, 4, 1, 2], axis=0))
    assert obs.scene_ids_tensor(ids, 5, 8, torch.device("cpu"), order).tolist() == [2, 5, 9, -1, 7, -1, -1, -1]
    assert obs.scene_ids_tensor(np.array([2 ** 40, -(2 ** 40)]), 2, 2, torch.device("cpu")).tolist() == [2 ** 31 - 1, -1]
    for bad in (np.zeros(4, dtype=int), np.zeros((5, 1), dtype=int), np.zeros(5)):
        with pytest.raises(ValueError, match="scene ids"):
            obs.scene_ids_tensor(bad, 5, 8, torch.device("cpu"))


def test_depth_camera_refusals_with_scenes():
    from dronesim_amd.camera import DepthCamera
    from dronesim_amd.params import builtin_type
    ctx = types.SimpleNamespace(types=[builtin_type("tello")])
    s = _scenes()
    with pytest.raises(NotImplementedError, match="drones=True"):
        DepthCamera(ctx, None, s, drones=True, scene_id=np.zeros(2, dtype=int))
    with pytest.raises(ValueError, match="scene_id is required"):
        DepthCamera(ctx, None, s)
    with pytest.raises(ValueError, match="scene_id without"):
        DepthCamera(ctx, None, sr.gate(), scene_id=np.zeros(2, dtype=int))


def test_env_refusals_with_scenes():
    """All before a context is made: ids missing, misshapen or given without scenes; the two deliberate cuts."""
    from dronesim_amd.envs import CtrlAviary
    s, xyz, ids = _scenes(), np.zeros((4, 3)), np.zeros(4, dtype=int)
    kw = dict(initial_xyzs=xyz, dict_io=False)
    with pytest.raises(ValueError, match="obstacle_scene_id .* is required"):
        CtrlAviary(["tello"], 4, obstacle_watch=s, **kw)
    with pytest.raises(ValueError, match="obstacle_scene_id .* is required"):
        CtrlAviary(["tello"], 4, vision_attributes=True, vision_scene=s, **kw)
    for bad in (np.zeros(3, dtype=int), np.zeros((4, 1), dtype=int), np.zeros(4), [0, 1]):
        with pytest.raises(ValueError, match=r"obstacle_scene_id must be \[4\] ints"):
            CtrlAviary(["tello"], 4, obstacle_watch=s, obstacle_scene_id=bad, **kw)
    with pytest.raises(ValueError, match="obstacle_scene_id without"):
        CtrlAviary(["tello"], 4, obstacle_watch=sr.gate(), obstacle_scene_id=ids, **kw)
    with pytest.raises(ValueError, match="obstacle_scene_id without"):
        CtrlAviary(["tello"], 4, obstacle_scene_id=ids, **kw)
    with pytest.raises(NotImplementedError, match="chord in the placement's frame"):
        CtrlAviary(["tello"], 4, obstacle_watch=s, obstacle_scene_id=ids, obstacle_sweep=True, **kw)
    for world in (dict(obstacle_watch=s), dict(vision_scene=s)):
        with pytest.raises(NotImplementedError, match="vision_see_drones"):
            CtrlAviary(["tello"], 4, obstacle_scene_id=ids, vision_attributes=True, vision_see_drones=True, **world, **kw)
