"""The drones in the camera's images without a device: the fp64 sphere caster of tests/camera_drones_ref.py against closed forms,
the float32 restatement's error against the record the GPU tolerance is derived from, and the library's host side (symbols, struct
layout, workspace size, refusals that reach no device)."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

import __graft_entry__ as graft
from tests import camera_drones_ref as dr
from tests import camera_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TELLO_R = 0.05173490117899134


@pytest.fixture(scope="module")
def nat():
    graft.build()
    from dronesim_amd import _native
    return _native


# ---- the caster against closed forms ------------------------------------------------------------------------------------------------
def level_rays(W=33, H=25):
    """A level camera with L = 0 at the origin: f = (1, 0, 0) exactly, the centre pixel's ray is f."""
    eye, d = cr.camera_rays((0.0, 0.0, 0.0), (0, 0, 0, 1), 0.0, W, H)
    np.testing.assert_allclose(d[H // 2, W // 2], [1.0, 0.0, 0.0], atol=1e-15)
    return eye, d, (H // 2, W // 2)


def test_centred_sphere():
    """A sphere of radius R on the optical axis at distance D: the centre pixel sees it at t = D - R head on (|n . d| = 1); a ray at
    angle a to the axis at the smaller root of t^2 |d|^2 - 2 t D + D^2 - R^2 = 0, and only while D sin a <= R."""
    eye, d, c = level_rays()
    D, R = 5.0, 0.5
    r = dr.cast_spheres([[D, 0, 0]], [R], eye, d, 0.1, 1000.0)
    assert abs(r["t"][c] - (D - R)) < 1e-12 and r["idx"][c] == 0 and abs(r["ndot"][c] - 1.0) < 1e-12
    aa = (d * d).sum(-1)
    disc = D * D - aa * (D * D - R * R)
    want = np.where(disc >= 0, (D - np.sqrt(np.maximum(disc, 0))) / aa, np.inf)
    np.testing.assert_allclose(r["t"], want, rtol=1e-12)
    assert np.isfinite(want).sum() > 20 and np.isinf(want).sum() > 500
    assert (r["idx"][np.isinf(want)] == -1).all() and (r["ndot"][np.isinf(want)] == 1.0).all()
    # t is eye-space depth: the distance along the ray is t |d|
    off_axis = np.isfinite(want) & (aa > 1.0001)
    assert off_axis.any() and (np.abs(r["t"][off_axis] * np.sqrt(aa[off_axis]) - np.linalg.norm(r["t"][off_axis][:, None] * d[off_axis], axis=1)) < 1e-12).all()


def test_eye_inside_a_sphere_sees_its_far_side():
    eye, d, c = level_rays()
    r = dr.cast_spheres([[0.25, 0, 0]], [1.0], eye, d, 0.1, 1000.0)
    assert np.isfinite(r["t"]).all()                          # every ray leaves through the sphere
    assert abs(r["t"][c] - 1.25) < 1e-12 and abs(r["ndot"][c] - 1.0) < 1e-12
    hp = r["t"][..., None] * d
    np.testing.assert_allclose(np.linalg.norm(hp - [0.25, 0, 0], axis=-1), 1.0, rtol=1e-12)
    # the own drone's case: the eye L above a centre it is inside of, excluded by index
    r2 = dr.cast_spheres([[0.25, 0, 0], [50.0, 0, 0]], [1.0, 0.5], eye, d, 0.1, 1000.0, own=0)
    assert abs(r2["t"][c] - 49.5) < 1e-12 and r2["idx"][c] == 1 and (r2["idx"] != 0).all()


def test_tangent_ray_is_masked_not_decided():
    """The centre ray passes a sphere at exactly rho = R (1 + 1e-4): no hit, and the pixel is ambiguous; at rho = R (1 + 1e-2) it is
    neither."""
    eye, d, c = level_rays()
    for k, masked in ((1e-4, True), (-1e-4, True), (1e-2, False)):
        R = 0.25
        r = dr.cast_spheres([[4.0, R * (1.0 + k), 0]], [R], eye, d, 0.1, 1000.0)
        assert np.isfinite(r["t"][c]) == (k < 0)
        t = np.where(np.isfinite(r["t"]), r["t"], np.inf)
        assert bool(dr.sphere_mask(r, t, 0.1, 1000.0, 1000.0)[c]) == masked


def test_sphere_behind_near_and_straddling_it():
    eye, d, c = level_rays()
    # wholly in front of the near plane: invisible; straddling it: the second root; the first root 1e-4 from near: ambiguous
    assert np.isinf(dr.cast_spheres([[0.5, 0, 0]], [0.25], eye, d, 1.0, 1000.0)["t"]).all()
    r = dr.cast_spheres([[1.0, 0, 0]], [0.25], eye, d, 1.0, 1000.0)
    assert abs(r["t"][c] - 1.25) < 1e-12
    x = np.float32(1.25 + 1e-4)                                # (the caster reads float32 inputs)
    r = dr.cast_spheres([[x, 0, 0]], [0.25], eye, d, 1.0, 1000.0)
    assert abs(r["t"][c] - (float(x) - 0.25)) < 1e-12 and dr.sphere_mask(r, r["t"], 1.0, 1000.0, 1000.0)[c]


def test_sphere_beyond_the_range_and_not_drawn_ones():
    eye, d, c = level_rays()
    ctr, rad = [[30.0, 0, 0], [10.0, 0, 0], [5.0, 0, 0], [np.nan, 0, 0]], [0.5, 0.5, 0.0, 0.5]
    assert dr.cast_spheres(ctr, rad, eye, d, 0.1, 1000.0)["idx"][c] == 1          # R = 0 and the NaN position are not drawn
    assert dr.cast_spheres(ctr, rad, eye, d, 0.1, 9.0)["idx"][c] == -1            # min(far, range) cuts
    assert dr.cast_spheres(ctr[:1], rad[:1], eye, d, 0.1, 29.5)["t"][c] == 29.5   # inclusive
    # merged with the triangles: a wall at x = 20 hides the sphere at 30 and is hidden by the one at 10
    from dronesim_amd.obstacles import ObstacleSet
    wall = ObstacleSet.box((20.5, 0.0, 0.0), (1.0, 40.0, 40.0))
    st = np.array([[0, 0, -0.25], [30.0, 0, 0], [10.0, 0, 0]], dtype=np.float32)
    ref = dr.reference_image(wall.triangles, wall.body, st, [0.1, 0.5, 0.5], 0, (0, 0, 0, 1), 0.25, 33, 25, label=[7, 8, 9])
    assert ref["seg"][12, 16] == dr.seg_drone(9) and abs(ref["t"][12, 16] - 9.5) < 1e-3 and ref["is_drone"][12, 16]
    assert ref["seg"][0, 0] == 0 and abs(ref["t"][0, 0] - 20.0) < 1e-2 and not (ref["seg"] == dr.seg_drone(8)).any()
    assert not (ref["seg"] == dr.seg_drone(7)).any()          # the own drone
    near = dr.reference_image(wall.triangles, wall.body, st, [0.1, 0.5, 0.5], 0, (0, 0, 0, 1), 0.25, 33, 25, rng=5.0)
    assert (near["seg"] == 0).all()


# ---- the float32 restatement --------------------------------------------------------------------------------------------------------
def sphere_error(t32, ref):
    m = ref["is_drone"] & ~ref["ambiguous"]
    assert not ((np.isfinite(t32) != np.isfinite(ref["t"])) & ~ref["ambiguous"]).any()
    return float((np.abs(t32[m] - ref["t"][m]) * np.maximum(ref["ndot"][m], 0.05) / ref["t"][m]).max()) if m.any() else 0.0


def test_restated_sphere_error_is_what_is_recorded():
    """The float32 restatement of the kernel's sphere arithmetic against the fp64 caster over the GPU tests' own scenes, every
    sphere in view (no obstacle set in front): the main scene at both resolutions with and without offsets, the lattice at both
    ranges.  Its worst |t - t_ref| max(|n . d|, 0.05) / t_ref is the recorded SPHERE_RESTATED_WORST (not above it, and the record
    is not padded); it hits exactly the pixels the reference hits outside the mask, and the mask stays below 1 % of every image."""
    worst, pixels = 0.0, 0
    for off in (False, True):
        st, _, _, rad = dr.main_fleet(off)
        for res in ((64, 48), (20, 12)):
            refs = dr.main_reference(None, res, off)
            for k, (c, L) in enumerate(zip(cr.CAMERAS, cr.camera_arms())):
                ref = refs[k][0]
                assert ref["ambiguous"].mean() <= 0.01
                worst = max(worst, sphere_error(dr.restated_spheres(st[:, :3], rad, c, st[c, 3:], L, *res), ref))
                pixels += int(ref["is_drone"].sum())
    st, rad = dr.lattice_fleet(), dr.type_radii(["tello"] * dr.LATTICE_N)
    for rng in (20.0, None):
        for c, ref in zip(dr.LATTICE_CAMERAS, dr.lattice_reference(rng)):
            assert ref["ambiguous"].mean() <= 0.01
            worst = max(worst, sphere_error(dr.restated_spheres(st[:, :3], rad, c, st[c, 3:], cr.ARM["tello"], 64, 48, rng=rng), ref))
            pixels += int(ref["is_drone"].sum())
    print(f"restated sphere worst {worst:.4e} over {pixels} sphere pixels")
    assert pixels > 2000
    assert worst <= dr.SPHERE_RESTATED_WORST <= 1.02 * worst, worst
    assert dr.SPHERE_TOL == 4.0 * dr.SPHERE_RESTATED_WORST


def test_the_walk_finds_what_brute_force_finds():
    """The kernel's route restated in float32 (binning, the outside list, the 2-D walk with its partial blocks, the early stop)
    gives, pixel for pixel, the very t of the float32 brute force over all spheres: the walk loses no sphere.  The main scene on
    the grid the camera would choose and on a pinned box that leaves a dozen drones outside (20 x 12), and the lattice's long
    walks (with and without the range)."""
    from dronesim_amd.downwash import clearance_grid
    st, _, _, rad = dr.main_fleet(False)
    r_max = float(rad.max())
    hits = 0
    for lo, hi in (((float(st[:, 0].min()), float(st[:, 1].min())), (float(st[:, 0].max()), float(st[:, 1].max()))), ((0.0, -2.6), (4.2, 2.6))):
        grid = clearance_grid(lo, hi, r_max, max(0.25 - 2.0 * r_max, 0.0), cr.FLEET_N)
        assert grid[0] >= 2.0 * r_max
        for c, L in zip(cr.CAMERAS, cr.camera_arms()):
            t, steps, tests = dr.walked_spheres(st[:, :3], rad, c, st[c, 3:], L, 20, 12, grid)
            assert np.array_equal(t, dr.restated_spheres(st[:, :3], rad, c, st[c, 3:], L, 20, 12)), c
            hits += int(np.isfinite(t).sum())
    assert hits > 150
    st, rad = dr.lattice_fleet(), dr.type_radii(["tello"] * dr.LATTICE_N)
    grid = clearance_grid((0.0, 0.0), (63.0, 63.0), float(rad.max()), max(0.25 - 2.0 * float(rad.max()), 0.0), dr.LATTICE_N)
    far_hits, longest = 0, 0.0
    for c, res, rng in ((dr.LATTICE_CAMERAS[0], (64, 48), None), (dr.LATTICE_CAMERAS[1], (32, 48), 20.0)):
        t, steps, tests = dr.walked_spheres(st[:, :3], rad, c, st[c, 3:], cr.ARM["tello"], *res, grid, rng=rng)
        assert np.array_equal(t, dr.restated_spheres(st[:, :3], rad, c, st[c, 3:], cr.ARM["tello"], *res, rng=rng)), (c, rng)
        assert tests < dr.LATTICE_N / 8                        # ... and tests a fraction of the fleet per ray
        far_hits += int((t[np.isfinite(t)] > 20.0).sum())
        longest = max(longest, steps)
    assert far_hits > 20 and longest > 10                      # many-cell walks


def test_the_scenes_are_what_the_gpu_tests_need():
    """Main scene, 64 x 48, no offsets: drones in front of triangles and triangles in front of drones; the lattice: hits on both
    sides of the 20 m range; the tello's radius is the one the closed forms above assume for the own-drone geometry."""
    assert abs(float(dr.type_radii(["tello"])[0]) - TELLO_R) < 1e-7 and cr.ARM["tello"] > TELLO_R      # a tello's eye is outside its sphere
    assert float(dr.type_radii(["hexa_6DOF_simple"])[0]) > 0.0
    sc = cr.scene(0)
    st, _, _, rad = dr.main_fleet(False)
    refs = dr.main_reference(0, (64, 48), False)
    bare = dr.main_reference(None, (64, 48), False)
    front = sum(int((refs[k][0]["is_drone"] & (tri["seg"] >= 0)).sum()) for k, tri in enumerate(
        cr.reference_image(sc.triangles, sc.body, st[c, :3], st[c, 3:], L, 64, 48) for c, L in zip(cr.CAMERAS, cr.camera_arms())))
    behind = sum(int((bare[k][0]["is_drone"] & (refs[k][0]["seg"] >= 0)).sum()) for k in range(5))
    assert front > 50 and behind > 50, (front, behind)
    far_hits = [r["t"][r["is_drone"]] for r in dr.lattice_reference(None)]
    assert sum(int((t > 20.0).sum()) for t in far_hits) > 40 and max(float(t.max()) for t in far_hits) > 45.0
    assert all(not (r["t"][r["is_drone"]] > 20.0).any() for r in dr.lattice_reference(20.0))


# ---- the axis fleet: what tests/test_gpu_camera_edges.py takes for granted ----------------------------------------------------------
def test_axis_fleet_is_laid_out_as_described():
    """32 hexas on odd numbers (type-major storage differs from the caller's order), the camera a tello; per depth the first drone
    exactly on the ray's line in xy and the others within a sphere's radius of it or a pixel column off; the chosen grid has cells
    of 2 R_max or more, a few metres; the pinned box's grid has a border 0.1 m beyond the 41 m drones of the +x line, which lie in
    its outermost cell, a border along y = 0 to float32 rounding, and leaves the lines along y outside."""
    st, models, rad, info = dr.axis_fleet()
    assert models[dr.AXIS_CAMERA] == "tello" and sum(m == "hexa_6DOF_simple" for m in models) == 32 and len(models) == dr.AXIS_N
    assert np.array_equal(st[dr.AXIS_CAMERA, :3], np.array(dr.AXIS_EYE, np.float32))
    R = float(rad[1])
    assert abs(R - 0.2020269) < 1e-6 and (rad[[i for i, m in enumerate(models) if m == "tello"]] < 0.06).all()
    on_line = 0
    for name, _, zero in cr.EDGE_QUATS:
        axis, sign = 1 - zero, (1.0 if name[0] == "+" else -1.0)
        assert set(info[name]) == ({7.0, 19.0, 41.0} if sign > 0 else {7.0, 19.0})
        for D, ids in info[name].items():
            assert abs(sign * st[ids, axis] - D).max() < 0.01          # the depth along the view
            on_line += int((st[ids, zero] == 0.0).sum())
            assert st[ids[0], zero] == 0.0 and abs(st[ids[1], zero]) == 0.125 < R
    assert on_line == 12                                       # one per depth and direction, two in the 41 m groups
    cell, xmin, ymin, nx, ny = dr.axis_grid()
    assert 2.0 * R <= cell < 4.1 and nx * ny <= 4 * dr.AXIS_N                    # 41 m is more than 10 cells
    box = dr.axis_pinned_box()
    pc, px, py, pnx, pny = dr.axis_grid(box)
    f32 = np.float32
    in_cell = lambda j: (int(np.floor((st[j, 0] - f32(px)) * (f32(1.0) / f32(pc)))), int(np.floor((st[j, 1] - f32(py)) * (f32(1.0) / f32(pc)))))
    for j in (info["+x"][41.0][0], info["+x"][41.0][2]):
        cx, cy = in_cell(j)
        assert cx == pnx - 1 and 0 <= cy < pny                 # the outermost cell ...
        assert 0.0 < float(f32(px) + f32(pnx) * f32(pc)) - float(st[j, 0]) < R     # ... and the sphere reaches out of it
    border = f32(f32(f32(py) - f32(pc)) + f32(4.0) * f32(pc))                     # the walk's face: gy0 + 4 cell
    assert abs(float(border)) < 1e-6
    for name in ("+y", "-y"):
        for ids in info[name].values():
            assert all(not 0 <= in_cell(j)[1] < pny for j in ids)


_AXIS_REF = {}


def axis_ref(name, q, res, rng, sd):
    key = (name, res, rng, sd)
    if key not in _AXIS_REF:
        _AXIS_REF[key] = dr.axis_reference(q, res, rng, sd)
    return _AXIS_REF[key]


def test_axis_fleet_masks_and_what_is_in_view():
    """Every image the GPU test compares (the four axis cameras x 17 x 17 and 1 x 33 x range none / 25 m x no set / scene(0)): the
    union mask is at most 1 % (none at all below 100 pixels).  In the zero-component columns at least 3 drone pixels lie further
    than 10 cells of the chosen sphere grid from the eye with no range, and none beyond the range with it; the 41 m drones of the
    +x line (the pinned grid's outermost cell) and drones of the lines along y (outside the pinned box) win pixels; scene(0)
    stands in front of part of the +x row."""
    st, _, _, info = dr.axis_fleet()
    cell = dr.axis_grid()[0]
    far_px = 0
    winners = set()
    for name, q, zero in cr.EDGE_QUATS:
        for res in dr.AXIS_RES:
            for rng in (None, dr.AXIS_RANGE):
                for sd in (None, 0):
                    ref = axis_ref(name, q, res, rng, sd)
                    assert ref["ambiguous"].sum() <= res[0] * res[1] // 100, (name, res, rng, sd)
                    col = ref["is_drone"][:, res[0] // 2]
                    ids = dr.seg_drone(ref["seg"][:, res[0] // 2][col])
                    dist = np.linalg.norm(st[ids, :2] - st[dr.AXIS_CAMERA, :2], axis=1)
                    if rng is None:
                        far_px += int((dist > 10.0 * cell).sum()) if sd is None else 0
                        winners |= set(ids.tolist())
                    else:
                        assert not (ref["t"][ref["is_drone"]] > rng).any() and not (dist > rng + 1.0).any()
    print(f"drone pixels of zero columns beyond 10 cells ({10 * cell:.1f} m): {far_px}")
    assert far_px >= 3
    assert info["+x"][41.0][0] in winners and winners & set(info["+y"][41.0]) and winners & set(info["-y"][19.0])
    bare, front = axis_ref("+x", cr.EDGE_QUATS[0][1], (17, 17), None, None), axis_ref("+x", cr.EDGE_QUATS[0][1], (17, 17), None, 0)
    assert (front["seg"] >= 0).sum() >= 20 and (bare["is_drone"] & (front["seg"] >= 0)).any() and front["is_drone"].any()


def test_axis_walk_finds_what_brute_force_finds():
    """walked_spheres (the 2-D walk in float32 with the kernel's selects: inf steps for a zero component, the in_x / in_y tests, the
    tie rule along a cell border, the ring, the outside list) on the chosen grid and on the pinned one: outside the mask it hits
    what the fp64 caster hits, within the recorded float32 error, and is pixel for pixel the float32 brute force over all
    spheres."""
    st, _, rad, _ = dr.axis_fleet()
    grids = (dr.axis_grid(), dr.axis_grid(dr.axis_pinned_box()))
    worst, longest = 0.0, 0.0
    for name, q, zero in cr.EDGE_QUATS:
        qa = np.array(q, np.float32)
        for res in dr.AXIS_RES:
            for rng in (None, dr.AXIS_RANGE):
                ref = axis_ref(name, q, res, rng, None)
                t32 = dr.restated_spheres(st[:, :3], rad, dr.AXIS_CAMERA, qa, cr.ARM["tello"], *res, rng=rng)
                worst = max(worst, sphere_error(t32, ref))
                for grid in grids:
                    t, steps, _ = dr.walked_spheres(st[:, :3], rad, dr.AXIS_CAMERA, qa, cr.ARM["tello"], *res, grid, rng=rng)
                    assert np.array_equal(t, t32), (name, res, rng, grid)
                    longest = max(longest, steps)
    print(f"restated sphere worst on the axis fleet {worst:.4e}; longest mean walk {longest:.1f} cells")
    assert worst <= dr.SPHERE_RESTATED_WORST                   # the record covers this fleet: SPHERE_TOL stands
    assert longest > 30


def test_edge_strips_with_the_fleet_drawn_stay_under_the_cap():
    """The 1 x 1024 and 1024 x 1 images of camera_ref.EDGE_STRIP through dsim_depth_image_drones (scene(0), the edge fleet's other
    drones drawn): the union mask is at most 1 %, and drones are in view."""
    sc = cr.scene(0)
    pose = next(p for p in cr.edge_poses(sc) if (p["eye"], p["cam"]) == cr.EDGE_STRIP)
    seen = 0
    for res in cr.EDGE_STRIP_RES:
        ref = dr.edge_fleet_reference(sc, pose, res)
        assert ref["ambiguous"].sum() <= res[0] * res[1] // 100, (res, int(ref["ambiguous"].sum()))
        seen += int(ref["is_drone"].sum())
    assert seen > 0


# ---- the library's host side (nothing here reaches a device) -----------------------------------------------------------------------
def test_header_declares_and_library_exports_the_call(nat):
    hdr = open(os.path.join(ROOT, "include", "dronesim_amd.h")).read()
    lib = nat.load()
    for f, rtype, n_args in (("dsim_depth_image_drones", "int", 12), ("dsim_depth_image_drones_workspace", "int64_t", 3)):
        m = re.search(rf"^{rtype}\s+{f}\s*\(([^;]*)\);", hdr, flags=re.M | re.S)
        assert m, f
        assert m.group(1).count(",") + 1 == n_args == len(getattr(lib, f).argtypes), f
        assert f in nat.EXPORTS
    assert re.search(r"#define DSIM_SEG_DRONE\(k\) \(-3 - \(k\)\)", hdr)
    assert nat.seg_drone(0) == -3 and nat.seg_drone(nat.seg_drone(41)) == 41
    assert re.search(r"#define DSIM_ABI_MINOR 1\b", hdr) and "dsim_depth_image_drones" in hdr.split("#define DSIM_MAX_ACT")[0]
    # the old entry point is declared as it was
    assert re.search(r"^int\s+dsim_depth_image\s*\(([^;]*)\);", hdr, flags=re.M | re.S).group(1).count(",") + 1 == 11


def test_camera_drones_struct_matches_c(nat, tmp_path):
    fields = [f for f, _ in nat.CameraDrones._fields_]
    lines = ['printf("size %zu\\n", sizeof(dsim_camera_drones));'] + [f'printf("{f} %zu\\n", offsetof(dsim_camera_drones, {f}));' for f in fields]
    src = tmp_path / "camdr.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dronesim_amd.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "camdr"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(nat.CameraDrones)
    for f in fields:
        assert int(got[f]) == getattr(nat.CameraDrones, f).offset, f


def test_workspace_holds_the_watch_and_the_outside_list(nat):
    lib = nat.load()
    for m, nx, ny in ((70, 5, 7), (4096, 68, 68), (1, 1, 1), (100000, 300, 200)):
        need, watch = lib.dsim_depth_image_drones_workspace(m, nx, ny), lib.dsim_clearance_workspace(m, nx, ny)
        # behind the watch's pieces: a 16-byte aligned float4 [m] (+ 4 words of slack), an int [m], 4 ints of length
        assert need >= watch and need >= 2 * (nx * ny + 1) + nx * ny + 4 + 4 * m + m + 4 + 4 * m + m + 4
        assert need <= watch + 4 + 4 * m + m + 4
    assert lib.dsim_depth_image_drones_workspace(-1, 5, 5) == -1 and lib.dsim_depth_image_drones_workspace(5, 0, 5) == -1


def test_library_refuses_without_touching_a_device(nat):
    """The refusals that come before the context is used: every missing piece gives DSIM_E_ARG (-1)."""
    lib = nat.load()
    p = nat.CameraParams(64, 48, 60.0, 1.0, 1000.0, 0)
    g = nat.DownwashArgs()
    d = nat.CameraDrones()
    d.grid, d.range = ctypes.addressof(g), 20.0
    out = ctypes.create_string_buffer(16)
    args = lambda dd: (None, None, nat.View(), None, ctypes.byref(p), 1, None, None, None, dd, ctypes.addressof(out), None)
    assert lib.dsim_depth_image_drones(*args(None)) == -1                         # no drones
    assert lib.dsim_depth_image_drones(*args(ctypes.byref(d))) == -1              # no context
    for bad in (0.0, -1.0, float("nan")):
        d.range = bad
        assert lib.dsim_depth_image_drones(*args(ctypes.byref(d))) == -1
    d.range, d.grid = 20.0, None
    assert lib.dsim_depth_image_drones(*args(ctypes.byref(d))) == -1              # no grid


def test_depth_camera_and_env_refuse_bad_drone_keywords(nat):
    from dronesim_amd.camera import DepthCamera
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.params import builtin_type
    ctx = types.SimpleNamespace(types=[builtin_type("tello")])
    sc = cr.scene(0)
    for kw, msg in ((dict(drone_range=5.0), "without drones"), (dict(drone_box=(0, 0, 1, 1)), "without drones"),
                    (dict(drones=True, drone_range=0.0), "drone_range"), (dict(drones=True, drone_box=(0, 0, 1)), "drone_box"),
                    (dict(drones=True, drone_box=(2, 0, 1, 1)), "drone_box")):
        with pytest.raises(ValueError, match=msg):
            DepthCamera(ctx, None, sc, **kw)
    with pytest.raises(TypeError, match="drones=True"):
        DepthCamera(ctx, None, None)
    xyz = np.zeros((2, 3))
    with pytest.raises(ValueError, match="without vision_attributes"):
        CtrlAviary(["tello"], 2, initial_xyzs=xyz, vision_see_drones=True)
    with pytest.raises(ValueError, match="vision_drone_range"):
        CtrlAviary(["tello"], 2, initial_xyzs=xyz, vision_attributes=True, vision_scene=sc, vision_drone_range=5.0)
    with pytest.raises(ValueError, match="vision_drone_range"):
        CtrlAviary(["tello"], 2, initial_xyzs=xyz, vision_attributes=True, vision_see_drones=True, vision_drone_range=-1.0)
    assert DepthCamera.seg_drone(np.array([-1, -2, 0, 5, -3, -44])).tolist() == [-1, -1, -1, -1, 0, 41]
