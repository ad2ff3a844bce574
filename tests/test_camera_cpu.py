"""CPU-side checks of the depth camera: the fp64 reference caster against closed forms, the ray grid's lists against the
triangles' bounding boxes, the watch grid's outputs against what the library gave before the ray grid came in, the ABI surface,
argument validation, and the float32 figure the GPU tests' tolerance is made from."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

import __graft_entry__ as graft
from tests import camera_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nat():
    graft.build()
    from dronesim_amd import _native
    return _native


# ---- the reference caster against closed forms --------------------------------------------------------------------------------------
def test_reference_box_face_head_on():
    """A level camera (L = 0: f = (1, 0, 0) exactly) in front of an axis-aligned box: every pixel on the near face has t = the
    face distance, the centre pixel included — t is eye-space depth, not the distance along the ray (which is t |d|)."""
    from dronesim_amd.obstacles import ObstacleSet
    box = ObstacleSet.box((3.0, 0.0, 1.0), (2.0, 2.0, 2.0))
    W, H = 33, 25
    eye, d = cr.camera_rays((0.0, 0.0, 1.0), (0, 0, 0, 1), 0.0, W, H)
    np.testing.assert_allclose(d[H // 2, W // 2], [1.0, 0.0, 0.0], atol=1e-15)
    r = cr.cast(box.triangles, box.body, eye, d, 0.1, 1000.0)
    on_face = (np.abs(d[..., 1]) * 2.0 < 0.999) & (np.abs(d[..., 2]) * 2.0 < 0.999)          # the face spans +-1 m at x = 2
    off_face = (np.abs(d[..., 1]) * 2.0 > 1.001) | (np.abs(d[..., 2]) * 2.0 > 1.001)
    assert on_face.sum() > 300 and off_face.sum() > 100 and on_face[H // 2, W // 2]
    np.testing.assert_allclose(r["t"][on_face], 2.0, rtol=1e-12)
    assert (r["seg"][on_face] == 0).all() and np.isinf(r["t"][off_face]).all() and (r["seg"][off_face] == -1).all()
    # the distance along the ray is t |d| = 2 / cos: what t is NOT
    assert np.abs(r["t"][on_face] * np.linalg.norm(d[on_face], axis=1) - 2.0).max() > 0.2
    np.testing.assert_allclose(r["ndot"][on_face], 1.0 / np.linalg.norm(d[on_face], axis=1), rtol=1e-12)
    # inside the box the far face is seen from behind (both faces of a triangle are hit); near clips the near one away
    r2 = cr.cast(box.triangles, box.body, eye, d, 2.5, 1000.0)
    assert abs(r2["t"][H // 2, W // 2] - 4.0) < 1e-12


def test_reference_ground_plane_of_a_level_camera():
    """eye at height h, level: the pixel of row r sees the plane at t = h / -b(r) below the horizon and nothing above it; the
    top row of the image is row 0."""
    W, H, h = 16, 12, 1.5
    eye, d = cr.camera_rays((0.0, 0.0, h), (0, 0, 0, 1), 0.0, W, H)
    none = np.zeros((1, 3, 3), dtype=np.float32) + np.array([[[0, 0, 0], [1e-3, 0, 0], [0, 1e-3, 0]]], dtype=np.float32) + 500.0
    r = cr.cast(none, 0, eye, d, 0.05, 1000.0, ground=True)
    b = (1.0 - (np.arange(H) + 0.5) / H * 2.0) * np.tan(np.radians(30.0))
    assert (b[: H // 2] > 0).all() and np.isinf(r["t"][: H // 2]).all() and (r["seg"][: H // 2] == -1).all()
    np.testing.assert_allclose(r["t"][H // 2:], np.repeat((h / -b[H // 2:])[:, None], W, 1), rtol=1e-12)
    assert (r["seg"][H // 2:] == cr.SEG_GROUND).all()
    np.testing.assert_allclose(cr.depth_buffer_to_t(cr.depth_buffer(r["t"], 0.05, 1000.0), 0.05, 1000.0)[H // 2:], r["t"][H // 2:], rtol=1e-9)
    assert (cr.depth_buffer(r["t"], 0.05, 1000.0)[: H // 2] == 1.0).all()
    off, on = cr.cast(none, 0, eye, d, 0.05, 1000.0, ground="both")
    assert np.isinf(off["t"]).all() and np.array_equal(on["t"], r["t"])


def test_reference_degenerate_cameras_have_no_image():
    for pos, quat in (((np.nan, 0, 1), (0, 0, 0, 1)), ((0, 0, 1), (0, np.nan, 0, 1)), ((0, 0, 1), cr.quat_from_rpy(0, np.pi / 2, 0)),
                      ((0, 0, 1), cr.quat_from_rpy(0, -np.pi / 2, 0.3))):
        assert cr.camera_rays(pos, np.asarray(quat, np.float32), 0.0635, 8, 8) is None
    assert cr.camera_rays((0, 0, 1), cr.quat_from_rpy(0.3, 0.3, 0.1), 0.0635, 8, 8) is not None


def test_ambiguous_share_of_the_reference_is_small():
    """The mask the GPU tests leave out is at most 1 % of any of their images (it is asserted there too)."""
    sc = cr.scene(0)
    pos, quat = cr.camera_poses()
    worst = 0.0
    for k, L in enumerate(cr.camera_arms()):
        a, b = cr.reference_image(sc.triangles, sc.body, pos[k], quat[k], L, 64, 48, ground="both")
        worst = max(worst, a["ambiguous"].mean(), b["ambiguous"].mean())
    assert worst <= 0.01, worst


def test_restated_error_is_what_is_recorded():
    """The float32 restatement of the kernel's arithmetic against the fp64 caster over the GPU tests' own scenes: its worst
    |t - t_ref| max(|n . d|, 0.05) / t_ref is the recorded RESTATED_WORST (not above it, and the record is not padded); the
    restatement hits exactly the pixels the reference hits outside the ambiguity mask."""
    pos, quat = cr.camera_poses()
    worst = 0.0
    for sd, res in ((0, ((64, 48), (20, 12))), (2, ((64, 48), (20, 12)))):
        sc = cr.scene(sd)
        for W, H in res:
            for k, L in enumerate(cr.camera_arms()):
                ref = cr.reference_image(sc.triangles, sc.body, pos[k], quat[k], L, W, H)
                t32 = cr.restated_image(sc.triangles, pos[k], quat[k], L, W, H)
                assert not ((np.isfinite(t32) != np.isfinite(ref["t"])) & ~ref["ambiguous"]).any()
                worst = max(worst, cr.t_error(t32, ref))
    print(f"restated worst {worst:.3e}")
    assert worst <= cr.RESTATED_WORST <= 1.02 * worst, worst
    assert cr.KERNEL_TOL == 4.0 * cr.RESTATED_WORST


def test_the_walk_finds_what_brute_force_finds():
    """The kernel's route restated in float32 (grid box, cell walk, lists, early stop) gives, pixel for pixel, the very t of the
    float32 brute force over all triangles: the walk and the ray grid lose no triangle.  Both sets, the five poses, 20 x 12."""
    pos, quat = cr.camera_poses()
    hits = 0
    for sd in (0, 2):
        sc = cr.scene(sd)
        for k, L in enumerate(cr.camera_arms()):
            t, steps, tests = cr.walked_image(sc, pos[k], quat[k], L, 20, 12)
            b = cr.restated_image(sc.triangles, pos[k], quat[k], L, 20, 12)
            assert np.array_equal(t, b), (sd, k)
            assert tests < sc.n_tri / 4                    # ... and tests a fraction of the set per ray
            hits += int(np.isfinite(b).sum())
    assert hits > 400


# ---- the edge table: what tests/test_gpu_camera_edges.py takes for granted ------------------------------------------------------------
_EDGE_REF = {}


def edge_refs(sd):
    """{(pose number, res): (without ground, with ground)} of a set's edge table over EDGE_RES, plus the two strips of EDGE_STRIP;
    computed once."""
    if sd not in _EDGE_REF:
        sc = cr.scene(sd)
        out = {}
        for k, p in enumerate(cr.edge_poses(sc)):
            for res in cr.EDGE_RES + (cr.EDGE_STRIP_RES if (p["eye"], p["cam"]) == cr.EDGE_STRIP else ()):
                out[k, res] = cr.reference_image(sc.triangles, sc.body, p["pos"], p["quat"], p["L"], res[0], res[1], ground="both")
        _EDGE_REF[sd] = (sc, cr.edge_poses(sc), out)
    return _EDGE_REF[sd]


def test_edge_table_is_the_table():
    """22 poses: the five eyes x the four axis cameras, yaw pi / 4 from the corner and the low x face; both arms among them, on
    distinct drones of the fleet that carry none of the five old poses; the fleet holds them as given."""
    for sd in (0, 2):
        sc = cr.scene(sd)
        st, table = cr.edge_fleet(sc)
        assert [(p["eye"], p["cam"]) for p in table] == [(e, q[0]) for e in cr.EDGE_EYES for q in cr.EDGE_QUATS] + [("corner", "diag"), ("lo_x", "diag")]
        drones = [p["drone"] for p in table]
        assert len(set(drones)) == 22 and not set(drones) & set(cr.CAMERAS) and max(drones) < cr.FLEET_N
        assert {p["L"] for p in table if p["zero"] is not None} == {0.0635, 1.0635}
        for e in cr.EDGE_EYES:
            assert len({p["L"] for p in table if p["eye"] == e and p["zero"] is not None}) == 2
        for p in table:
            assert np.array_equal(st[p["drone"], :3], p["pos"]) and np.array_equal(st[p["drone"], 3:], p["quat"])
            assert p["L"] == cr.ARM[cr.FLEET_MODELS[p["drone"] % 2]]


def test_edge_eyes_lie_exactly_where_they_claim():
    """In float32, as the kernel forms them: the corner eye's x, y and z = fl(pz + L) equal interior faces fl(origin + fl(j) cell) of
    the set's ray grid; lo_x has ex == origin[0], hi_y has ey == hi[1]; off_y lies 0.5 m beyond hi[1] and off_corner a cell outside in
    x and y; every other coordinate is strictly inside the box."""
    f32 = np.float32
    for sd, dims in ((0, (7, 6, 4)), (2, (17, 14, 10))):
        sc = cr.scene(sd)
        g = sc.ray_grid()[0]
        assert (g.nx, g.ny, g.nz) == dims                      # (what the poses were looked at with; they follow the grid if it changes)
        o, hi, cell = np.array(list(g.origin), f32), np.array(list(g.hi), f32), f32(g.cell)
        faces = [np.array([f32(o[k] + f32(j) * cell) for j in range(1, n)], f32) for k, n in enumerate(dims)]
        for p in cr.edge_poses(sc):
            e = np.array([p["pos"][0], p["pos"][1], f32(p["pos"][2] + f32(p["L"]))], f32)      # the kernel's eye
            assert e.dtype == np.float32 and np.array_equal(e, p["eye_xyz"])
            inside = (e > o) & (e < hi)
            if p["eye"] == "corner":
                assert all(e[k] in faces[k] for k in range(3)) and inside.all()
            elif p["eye"] == "lo_x":
                assert e[0] == o[0] and e[1] in faces[1] and inside[1:].all()
            elif p["eye"] == "hi_y":
                assert e[1] == hi[1] and inside[0] and inside[2]
            elif p["eye"] == "off_y":
                assert e[1] == f32(hi[1] + f32(0.5)) and e[1] > hi[1] and inside[2]         # (in front of the box in x as well)
            else:
                assert e[0] == f32(o[0] - cell) and e[1] == f32(o[1] - cell) and e[0] < o[0] and e[1] < o[1] and inside[2]


def test_edge_zero_components_are_exactly_zero():
    """The float32 restatement of the rays (camera_drones_ref.rays32, operation by operation): on the centre column of the
    odd-width images the claimed component of d is == 0.0 for every axis pose, at every height; no other column has a zero there,
    and the yaw pi / 4 cameras have none at all."""
    from tests import camera_drones_ref as dr
    for p in cr.edge_poses(cr.scene(0)):
        for W, H in cr.EDGE_RES + cr.EDGE_STRIP_RES:
            _, d = dr.rays32(p["pos"], p["quat"], p["L"], W, H)
            if p["zero"] is None:
                assert (d[..., :2] != 0.0).all()
                continue
            z = d[..., p["zero"]] == 0.0
            want = np.zeros((H, W), bool)
            if W % 2:
                want[:, W // 2] = True
            assert np.array_equal(z, want), (p["eye"], p["cam"], W, H)
            assert (d[..., 1 - p["zero"]] != 0.0).all()


def test_edge_masks_stay_under_the_cap():
    """Every image the GPU test compares: the ambiguity mask is at most 1 % of it, which for an image of fewer than 100 pixels
    means no ambiguous pixel at all."""
    for sd in (0, 2):
        _, table, refs = edge_refs(sd)
        for (k, res), pair in refs.items():
            for ref in pair:
                assert ref["ambiguous"].sum() <= res[0] * res[1] // 100, (sd, table[k]["eye"], table[k]["cam"], res, int(ref["ambiguous"].sum()))


def test_edge_table_is_not_vacuous():
    """Summed over the table (17 x 17 and 1 x 33, both sets): at least 20 triangle hits in zero-component columns, some of them
    from the eye on the cell-plane corner; from off_y the cameras along x (dy = 0, the eye outside the y slab) hit no triangle in
    that column while the plane still answers there."""
    zero_hits = corner_hits = 0
    for sd in (0, 2):
        _, table, refs = edge_refs(sd)
        for k, p in enumerate(table):
            if p["zero"] is None:
                continue
            for res in ((17, 17), (1, 33)):
                bare, gnd = refs[k, res]
                col = bare["seg"][:, res[0] // 2]
                zero_hits += int((col >= 0).sum())
                corner_hits += int((col >= 0).sum()) if p["eye"] == "corner" else 0
                if p["eye"] == "off_y" and p["zero"] == 1:
                    gcol = gnd["seg"][:, res[0] // 2]
                    assert not (col >= 0).any() and np.isinf(bare["t"][:, res[0] // 2]).all()
                    assert (gcol[np.isfinite(gnd["t"][:, res[0] // 2])] == cr.SEG_GROUND).all() and (gcol == cr.SEG_GROUND).sum() >= res[1] // 2 - 1
    print(f"triangle hits in zero-component columns: {zero_hits}, from the cell-plane corner: {corner_hits}")
    assert zero_hits >= 20 and corner_hits >= 1


def test_edge_walk_finds_what_brute_force_finds():
    """The kernel's route restated in float32 (slab clip with its NaN rule, the inside tests, the clamped entry cell, the selects
    for a zero component, the tie rule, the lists with their slack at a face) over the edge table at 17 x 17 and 1 x 33: outside the
    mask it hits what the fp64 caster hits, at the same depth to the recorded float32 error, and it is pixel for pixel the float32
    brute force over all triangles — no triangle is lost at a face or along a cell plane."""
    for sd in (0, 2):
        sc, table, refs = edge_refs(sd)
        for k, p in enumerate(table):
            for res in ((17, 17), (1, 33)):
                ref = refs[k, res][0]
                t = cr.walked_image(sc, p["pos"], p["quat"], p["L"], *res)[0]
                assert not ((np.isfinite(t) != np.isfinite(ref["t"])) & ~ref["ambiguous"]).any(), (sd, p["eye"], p["cam"], res)
                assert cr.t_error(t, ref) <= cr.EDGE_RESTATED_WORST
                assert np.array_equal(t, cr.restated_image(sc.triangles, p["pos"], p["quat"], p["L"], *res)), (sd, p["eye"], p["cam"], res)


def test_edge_restated_error_is_what_is_recorded():
    """test_restated_error_is_what_is_recorded over the edge table: every image the GPU test compares (both sets, the five
    resolutions, the two strips).  The record is not above the worst by more than 2 %, and the bar the edge images get is 4 x the
    larger of the two records."""
    worst = 0.0
    for sd in (0, 2):
        sc, table, refs = edge_refs(sd)
        for (k, res), (ref, _) in refs.items():
            p = table[k]
            t32 = cr.restated_image(sc.triangles, p["pos"], p["quat"], p["L"], *res)
            assert not ((np.isfinite(t32) != np.isfinite(ref["t"])) & ~ref["ambiguous"]).any()
            worst = max(worst, cr.t_error(t32, ref))
    print(f"edge restated worst {worst:.3e}")
    assert worst <= cr.EDGE_RESTATED_WORST <= 1.02 * worst, worst
    assert cr.EDGE_KERNEL_TOL == 4.0 * max(cr.RESTATED_WORST, cr.EDGE_RESTATED_WORST)


# ---- the ray grid -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["scene", "soup"])
def test_ray_grid_lists_every_triangle_where_its_box_lies(nat, what):
    from dronesim_amd.obstacles import ObstacleSet
    s = cr.scene(0) if what == "scene" else ObstacleSet(cr.soup_600(), 0)
    assert (s.n_tri > 512) == (what == "soup")
    g, start, lst = s.ray_grid()
    cells, T = g.nx * g.ny * g.nz, s.n_tri
    assert cells <= 1 << 18 and max(g.nx, g.ny, g.nz) <= 4096 and 0 < g.list_len <= 1 << 26 and g.reach == 0.0
    assert start[0] == 0 and start[-1] == g.list_len == len(lst) and (np.diff(start) >= 0).all() and lst.min() >= 0 and lst.max() < T
    lo, hi, cell = np.array(list(g.lo), np.float64), np.array(list(g.hi), np.float64), float(g.cell)
    v = s.triangles.astype(np.float64)
    vmin, vmax = v.reshape(-1, 3).min(0), v.reshape(-1, 3).max(0)
    assert list(g.origin) == list(g.lo) and (lo < vmin).all() and (hi > vmax).all() and (lo > vmin - 0.02 * cell - 1e-5).all()
    assert (lo + np.array([g.nx, g.ny, g.nz]) * cell > hi).all()
    diag = np.linalg.norm(vmax - vmin)
    k = cell / (diag / (2.0 * np.cbrt(T)))
    assert abs(np.log2(k) - round(np.log2(k))) < 1e-6 and k >= 1.0 - 1e-6           # the planned edge, doubled some times
    key = np.unique(np.repeat(np.arange(cells, dtype=np.int64), np.diff(start)) * T + lst)
    assert len(key) == len(lst)                                                    # no triangle twice in a cell
    nn = np.array([g.nx, g.ny, g.nz])
    c_lo = np.clip(np.floor((v.min(1) - lo) / cell).astype(np.int64), 0, nn - 1)
    c_hi = np.clip(np.floor((v.max(1) - lo) / cell).astype(np.int64), 0, nn - 1)
    need = 0
    for t in range(T):
        zz, yy, xx = np.meshgrid(*(np.arange(c_lo[t, a], c_hi[t, a] + 1) for a in (2, 1, 0)), indexing="ij")
        c = ((zz * g.ny + yy) * g.nx + xx).ravel()
        need += c.size
        assert np.isin(c * T + t, key).all(), t
    # ... and hardly anywhere else: the slack is a hundredth of a cell (the watch grid of the gate lists every triangle everywhere)
    assert need <= len(lst) <= 1.5 * need
    assert len(lst) / cells < T / 8


def test_ray_plan_refusals(nat):
    lib = nat.load()
    tri = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]], dtype=np.float32)
    g = nat.ObstacleGrid()
    untouched = bytes(g)
    assert lib.dsim_obstacle_ray_grid_plan(tri.ctypes.data, 0, ctypes.byref(g)) == -1
    assert lib.dsim_obstacle_ray_grid_plan(None, 1, ctypes.byref(g)) == -1
    bad = tri.copy()
    bad[0, 2] = np.inf
    assert lib.dsim_obstacle_ray_grid_plan(bad.ctypes.data, 1, ctypes.byref(g)) == -1 and bytes(g) == untouched
    assert lib.dsim_obstacle_ray_grid_plan(tri.ctypes.data, 1, ctypes.byref(g)) == 0          # a flat soup: the slack gives it a box
    assert g.nx * g.ny * g.nz >= 1 and g.hi[2] > g.lo[2] and g.list_len >= 1
    start, lst = np.full(g.nx * g.ny * g.nz + 1, -3, np.int32), np.full(int(g.list_len), -3, np.int32)
    g.ny += 1
    assert lib.dsim_obstacle_ray_grid_build(tri.ctypes.data, 1, ctypes.byref(g), start.ctypes.data, lst.ctypes.data) == -1
    assert (start == -3).all() and (lst == -3).all()


def test_watch_grid_is_what_the_parent_commit_gave(nat, golden_dir):
    """dsim_obstacle_grid_plan / _build of the same sets, byte for byte against the record made before the ray grid shared their
    code (tests/golden/obstacle_grid_parent.npz)."""
    from dronesim_amd.obstacles import ObstacleSet
    z = np.load(os.path.join(golden_dir, "obstacle_grid_parent.npz"))
    for name, tri in (("scene", cr.scene(0).triangles), ("soup", cr.soup_600())):
        g, start, lst = ObstacleSet(tri, 0).grid(float(z[name + "_reach"]))
        assert bytes(g) == z[name + "_grid"].tobytes(), name
        assert np.array_equal(start, z[name + "_start"]) and np.array_equal(lst, z[name + "_list"]), name


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------
NEW = {"dsim_obstacle_ray_grid_plan": 3, "dsim_obstacle_ray_grid_build": 5, "dsim_obstacles_enable_rays": 2, "dsim_depth_image": 11}


def test_header_declares_and_library_exports_the_camera(nat):
    hdr = open(os.path.join(ROOT, "include", "dronesim_amd.h")).read()
    lib = nat.load()
    for f, n_args in NEW.items():
        m = re.search(rf"^int\s+{f}\s*\(([^;]*)\);", hdr, flags=re.M | re.S)
        assert m, f
        assert m.group(1).count(",") + 1 == n_args == len(getattr(lib, f).argtypes), f
        assert f in nat.EXPORTS
    assert re.search(r"DSIM_CAM_METRIC\s*=\s*1u << 0", hdr) and re.search(r"DSIM_CAM_GROUND\s*=\s*1u << 1", hdr)
    assert re.search(r"#define DSIM_SEG_GROUND \(-2\)", hdr)
    assert (nat.CAM_METRIC, nat.CAM_GROUND, nat.SEG_GROUND) == (1, 2, -2)
    assert os.path.exists(os.path.join(ROOT, "dronesim_amd", "csrc", "dsim_camera.hip"))
    assert os.path.join(ROOT, "dronesim_amd", "csrc", "dsim_camera.hip") in graft.HIP_DEPS


def test_camera_params_struct_matches_c(nat, tmp_path):
    fields = [f for f, _ in nat.CameraParams._fields_]
    lines = ['printf("size %zu\\n", sizeof(dsim_camera_params));'] + [f'printf("{f} %zu\\n", offsetof(dsim_camera_params, {f}));' for f in fields]
    src = tmp_path / "cam.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dronesim_amd.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "cam"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(nat.CameraParams)
    for f in fields:
        assert int(got[f]) == getattr(nat.CameraParams, f).offset, f


# ---- argument validation (nothing here reaches a device) ----------------------------------------------------------------------------
def test_depth_camera_refuses_bad_arguments(nat):
    from dronesim_amd.camera import DepthCamera
    from dronesim_amd.params import builtin_type
    ctx = types.SimpleNamespace(types=[builtin_type("tello")])
    sc = cr.scene(0)
    for kw, msg in ((dict(res=(0, 48)), "res"), (dict(res=(64, 1025)), "res"), (dict(fov=0.0), "fov"), (dict(fov=180.0), "fov"),
                    (dict(aspect=0.0), "aspect"), (dict(far=0.0), "far"), (dict(far=-1.0), "far"), (dict(far=np.inf), "far")):
        with pytest.raises(ValueError, match=msg):
            DepthCamera(ctx, None, sc, **kw)
    two = types.SimpleNamespace(types=[builtin_type("tello"), builtin_type("hexa_6DOF_simple")])
    with pytest.raises(ValueError, match="type_id"):
        DepthCamera(two, None, sc)
    import dataclasses
    armless = types.SimpleNamespace(types=[dataclasses.replace(builtin_type("tello"), arm=0.0)])
    with pytest.raises(ValueError, match="arm"):
        DepthCamera(armless, None, sc)


def test_env_refuses_bad_vision_keywords(nat):
    from dronesim_amd.envs import CtrlAviary
    sc = cr.scene(0)
    xyz = np.zeros((2, 3))
    with pytest.raises(ValueError, match="IMG_CAPTURE_FREQ"):          # 240 // 24 = 10 physics steps, not a multiple of 4
        CtrlAviary(["tello"], 2, initial_xyzs=xyz, freq=240, aggregate_phy_steps=4, vision_attributes=True, vision_scene=sc)
    with pytest.raises(ValueError, match="IMG_CAPTURE_FREQ"):          # 12 // 24 = 0
        CtrlAviary(["tello"], 2, initial_xyzs=xyz, freq=12, aggregate_phy_steps=1, vision_attributes=True, vision_scene=sc)
    with pytest.raises(ValueError, match="vision_scene"):
        CtrlAviary(["tello"], 2, initial_xyzs=xyz, vision_attributes=True)
    with pytest.raises(ValueError, match="without vision_attributes"):
        CtrlAviary(["tello"], 2, initial_xyzs=xyz, vision_scene=sc)
    with pytest.raises(ValueError, match="without vision_attributes"):
        CtrlAviary(["tello"], 2, initial_xyzs=xyz, vision_drones=[0])
    with pytest.raises(ValueError, match="vision_drones"):
        CtrlAviary(["tello"], 2, initial_xyzs=xyz, vision_attributes=True, vision_scene=sc, vision_drones=[2])
    with pytest.raises(ValueError, match="vision_res"):
        CtrlAviary(["tello"], 2, initial_xyzs=xyz, vision_attributes=True, vision_scene=sc, vision_res=(64, 0))
