"""The depth camera's hand-written degenerate cases on the device (k_depth_image behind dsim_depth_image and
dsim_depth_image_drones) against the fp64 brute-force casters of tests/camera_ref.py and tests/camera_drones_ref.py: rays with an
exactly zero component (1 / 0 in the slab clip, 0 x inf at a face, dt = inf, the inside tests), eyes on the faces of the ray grid's
box and on interior cell planes (the clamped entry cell, the tie rule, the lists' slack), images narrower than a wave's 8 x 8 tile
and at the documented maxima (the edge masking), the memory around the outputs, and the cam_index values the library accepts.

The poses (camera_ref.edge_poses) and the fleet of spheres (camera_drones_ref.axis_fleet) are built on the host, and every
condition on them — masks under the cap, zeros that are zeros, faces that are faces, hits where the edges are, the float32 walk
equal to brute force — is asserted without a device by test_camera_cpu.py and test_camera_drones_cpu.py.  The bars: triangles
EDGE_KERNEL_TOL = 4 x max(RESTATED_WORST, EDGE_RESTATED_WORST), spheres SPHERE_TOL (tests/README_camera.md).  On the centre column
of an odd-width image the device may contract ca into an fma and leave ~1e-8 where float32 numpy has 0: the reference is the
same for both, and nothing here asserts which of the two happened."""
import ctypes

import numpy as np
import pytest

import __graft_entry__ as graft
from tests import camera_drones_ref as dr
from tests import camera_ref as cr
from tests.camera_check import check_image

pytestmark = pytest.mark.gpu
FAR = 1000.0
GUARD = 16384                     # sentinel elements in front of and behind an output
DEP_SENTINEL, SEG_SENTINEL = -123.0, -7777       # values no image holds


@pytest.fixture(scope="module")
def torch_mod():
    graft.build()
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch


_REF = {}


def edge_reference(subdiv, res):
    """[(without ground, with ground)] x the edge table, computed once per (set, resolution)."""
    key = (subdiv, res)
    if key not in _REF:
        sc = cr.scene(subdiv)
        _REF[key] = [cr.reference_image(sc.triangles, sc.body, p["pos"], p["quat"], p["L"], res[0], res[1], far=FAR, ground="both")
                     for p in cr.edge_poses(sc)]
    return _REF[key]


def make_env(torch, st, models, n):
    from dronesim_amd.envs import CtrlAviary
    env = CtrlAviary(models, n, initial_xyzs=st[:, :3].astype(np.float64), noise_seed=0, dict_io=False, ground_plane=False)
    assert env.order is not None                              # two types interleaved: stored type-major, not in the caller's order
    env.state.set_fields(0, torch.from_numpy(np.ascontiguousarray(st.T)))
    return env


def edge_env(torch, sc):
    st, table = cr.edge_fleet(sc)
    return make_env(torch, st, [cr.FLEET_MODELS[i % 2] for i in range(cr.FLEET_N)], cr.FLEET_N), table


# ---- 1. the edge poses against the triangles ----------------------------------------------------------------------------------------
# between them the cases launch the four instances <LDS, SEG> at every resolution family, with the plane on and off, metric and
# depth-buffer: 17 x 17 is four 16 x 16 blocks, three of them with one live row or column; the others are narrower than a tile
EDGE_CASES = [
    # subdiv, res, ground, metric, seg
    (0, (17, 17), False, True, True),
    (0, (1, 33), True, False, False),
    (0, (33, 1), True, True, True),
    (0, (1, 1), True, True, False),
    (0, (5, 7), False, False, True),
    (2, (17, 17), True, True, False),
    (2, (1, 33), False, True, True),
    (2, (33, 1), False, False, False),
    (2, (1, 1), True, False, True),
    (2, (5, 7), True, True, True),
]


@pytest.mark.parametrize("subdiv, res, ground, metric, with_seg", EDGE_CASES)
def test_edge_poses_against_the_brute_force_reference(torch_mod, subdiv, res, ground, metric, with_seg):
    torch = torch_mod
    from dronesim_amd.camera import DepthCamera
    sc = cr.scene(subdiv)
    assert (sc.n_tri <= 512) == (subdiv == 0)
    env, table = edge_env(torch, sc)
    cam = DepthCamera(env.ctx, env.state, sc, res=res, far=FAR, ground=ground, metric=metric, cameras=[p["drone"] for p in table],
                      type_id=env._type_id)
    cam.seg.fill_(SEG_SENTINEL)
    dep, seg = cam.capture(seg=with_seg)
    torch.cuda.synchronize()
    assert tuple(dep.shape) == (len(table), res[1], res[0])
    if not with_seg:
        assert seg is None and bool((cam.seg == SEG_SENTINEL).all())
    dep_h, seg_h = dep.cpu().numpy(), (seg.cpu().numpy() if with_seg else None)
    refs = edge_reference(subdiv, res)
    worst, hits = 0.0, 0
    for k, p in enumerate(table):
        ref = refs[k][1 if ground else 0]
        worst = max(worst, check_image(f"{p['eye']} {p['cam']}", dep_h[k], seg_h[k] if with_seg else None, ref, p["L"], metric, FAR,
                                       tol=cr.EDGE_KERNEL_TOL))
        hits += int((ref["seg"] >= 0).sum())
    print(f"set {subdiv} {res[0]} x {res[1]}: {hits} triangle pixels, worst |dt| / bound {worst:.3f}")
    if res == (17, 17):
        assert hits > 500                                     # the set is in view
    cam.close()
    env.close()


# ---- 3. the same rays against the drone spheres -----------------------------------------------------------------------------------
AXIS_CASES = [
    # range, subdiv, pinned box, metric, seg
    (None, None, False, True, True),
    (dr.AXIS_RANGE, None, False, False, False),
    (None, 0, False, True, True),
    (dr.AXIS_RANGE, 0, True, True, False),
    (None, None, True, True, True),
]


@pytest.mark.parametrize("rng, subdiv, pinned, metric, with_seg", AXIS_CASES)
def test_axis_cameras_against_the_spheres(torch_mod, rng, subdiv, pinned, metric, with_seg):
    """The four axis quaternions in turn on one camera drone, 17 x 17 and 1 x 33: no obstacle set (the TRIS = false instances) and
    scene(0) in front of part of the +x row; no range and one that cuts the 41 m group; the grid the camera chooses and a pinned
    box with a drone in its outermost cell, a border along the rays' line and the lines along y on the outside list."""
    torch = torch_mod
    from dronesim_amd.camera import DepthCamera
    st, models, rad, info = dr.axis_fleet()
    env = make_env(torch, st, models, dr.AXIS_N)
    sc = cr.scene(subdiv) if subdiv is not None else None
    box = dr.axis_pinned_box() if pinned else None
    grid = dr.axis_grid(box)
    L = cr.ARM["tello"]
    cams = {res: DepthCamera(env.ctx, env.state, sc, res=res, far=FAR, metric=metric, cameras=[dr.AXIS_CAMERA], type_id=env._type_id,
                             drones=True, drone_range=rng, drone_box=box) for res in dr.AXIS_RES}
    worst, drone_px, far_px, outside_px = 0.0, 0, 0, 0
    outside = set(j for name in ("+y", "-y") for ids in info[name].values() for j in ids)
    for name, q, zero in cr.EDGE_QUATS:
        st[dr.AXIS_CAMERA, 3:] = q
        env.state.set_fields(0, torch.from_numpy(np.ascontiguousarray(st.T)))
        for res, cam in cams.items():
            dep, seg = cam.capture(seg=with_seg)
            torch.cuda.synchronize()
            a = cam._grid_args                                # the grid the conditions of the CPU tests were asserted on
            assert (a.nx, a.ny) == (grid[3], grid[4]) and a.cell == np.float32(grid[0]) and a.xmin == np.float32(grid[1])
            ref = dr.axis_reference(q, res, rng, subdiv)
            worst = max(worst, check_image(f"{name} {res[0]} x {res[1]}", dep[0].cpu().numpy(), seg[0].cpu().numpy() if with_seg else None,
                                           ref, L, metric, FAR, tol=cr.EDGE_KERNEL_TOL))
            drone_px += int(ref["is_drone"].sum())
            far_px += int((ref["t"][ref["is_drone"]] > 30.0).sum())
            outside_px += int(np.isin(dr.seg_drone(ref["seg"][ref["is_drone"]]), list(outside)).sum())
    print(f"range {rng} set {subdiv} pinned {pinned}: {drone_px} drone pixels, {far_px} beyond 30 m, worst |dt| / bound {worst:.3f}")
    assert drone_px >= 30 and (far_px >= 8 if rng is None else far_px == 0)
    if pinned:
        assert outside_px >= 10 and cams[(17, 17)].drones_outside() > 0        # drawn from the outside list
    else:
        assert all(c.drones_outside() == 0 for c in cams.values())
    for c in cams.values():
        c.close()
    env.close()


# ---- 4. image shapes and the memory around the outputs ----------------------------------------------------------------------------
def guarded(torch, dev, numel, dtype, sentinel):
    """A tensor of GUARD + numel + GUARD sentinels and the address of its middle."""
    t = torch.full((GUARD + numel + GUARD,), sentinel, dtype=dtype, device=dev)
    return t, t.data_ptr() + GUARD * t.element_size()


class Caller:
    """The two entry points called as a C caller calls them, on an edge fleet: the set, the storage slots of the cameras and — for
    dsim_depth_image_drones — the grid record come from a DepthCamera that has captured once."""

    def __init__(self, torch, env, sc, drones):
        from dronesim_amd.camera import DepthCamera
        self.torch, self.env, self.drones = torch, env, drones
        self.cam = DepthCamera(env.ctx, env.state, sc, res=(5, 7), far=FAR, metric=True, cameras=[0], type_id=env._type_id, drones=drones)
        self.cam.capture()
        torch.cuda.synchronize()

    def slot(self, drone):
        return int(self.env.order.slot_np[drone])

    def __call__(self, res, index, n_cam, dep_ptr, seg_ptr, flags=None):
        from dronesim_amd import _native as nat
        env = self.env
        p = nat.CameraParams(res[0], res[1], 60.0, 1.0, FAR, nat.CAM_METRIC if flags is None else flags)
        self.index = None if index is None else self.torch.tensor(index, dtype=self.torch.int32, device=env.ctx.device)
        idx = None if index is None else self.index.data_ptr()
        head = (env.ctx.handle, env.ctx.stream_ptr(), env.state.view(), self.cam.set.handle, ctypes.byref(p), n_cam, idx, None,
                env._type_id.data_ptr())
        if self.drones:
            rc = env.ctx.lib.dsim_depth_image_drones(*head, ctypes.byref(self.cam._dr), dep_ptr, seg_ptr)
        else:
            rc = env.ctx.lib.dsim_depth_image(*head, dep_ptr, seg_ptr)
        self.torch.cuda.synchronize()
        return rc

    def close(self):
        self.cam.close()
        self.env.close()


@pytest.mark.parametrize("drones", [False, True])
def test_shapes_and_the_memory_around_the_outputs(torch_mod, drones):
    """1 x 1, 1 x 1024 and 1024 x 1 (the documented maxima: 64 blocks per camera, each with one live row or column) and 17 x 17, two
    cameras, depth_out and seg_out in the middle of larger tensors of sentinels: afterwards every element outside [n_cam][H][W]
    still holds the sentinel and every element inside does not; 1025 wide is refused and writes nothing.  The two strips of
    EDGE_STRIP are compared with the reference (the 1 548-triangle set through dsim_depth_image, scene(0) with the fleet's drones
    drawn through dsim_depth_image_drones)."""
    torch = torch_mod
    sc = cr.scene(0 if drones else 2)
    env, table = edge_env(torch, sc)
    call = Caller(torch, env, sc, drones)
    pose = next(p for p in table if (p["eye"], p["cam"]) == cr.EDGE_STRIP)
    index = [call.slot(pose["drone"]), call.slot(table[0]["drone"])]
    dev = env.ctx.device
    for res in ((1, 1), (17, 17)) + cr.EDGE_STRIP_RES:
        numel = 2 * res[0] * res[1]
        dep, dep_ptr = guarded(torch, dev, numel, torch.float32, DEP_SENTINEL)
        seg, seg_ptr = guarded(torch, dev, numel, torch.int32, SEG_SENTINEL)
        assert call(res, index, 2, dep_ptr, seg_ptr) == 0
        for t, s in ((dep, DEP_SENTINEL), (seg, SEG_SENTINEL)):
            assert bool((t[:GUARD] == s).all()) and bool((t[GUARD + numel:] == s).all()), res      # nothing outside ...
            assert bool((t[GUARD:GUARD + numel] != s).all()), res                                     # ... and every pixel inside
        if res in cr.EDGE_STRIP_RES:
            img = dep[GUARD:GUARD + numel].reshape(2, res[1], res[0])[0].cpu().numpy()
            sg = seg[GUARD:GUARD + numel].reshape(2, res[1], res[0])[0].cpu().numpy()
            ref = (dr.edge_fleet_reference(sc, pose, res) if drones else
                   cr.reference_image(sc.triangles, sc.body, pose["pos"], pose["quat"], pose["L"], res[0], res[1], far=FAR))
            assert np.isfinite(ref["t"]).sum() > 250
            check_image(f"strip {res[0]} x {res[1]}", img, sg, ref, pose["L"], True, FAR, tol=cr.EDGE_KERNEL_TOL)
    for res in ((1025, 1), (1, 1025)):
        dep, dep_ptr = guarded(torch, dev, 2 * 1025, torch.float32, DEP_SENTINEL)
        assert call(res, index, 2, dep_ptr, None) == -1 and bool((dep == DEP_SENTINEL).all())
    call.close()


# ---- 5. cam_index values the library accepts --------------------------------------------------------------------------------------
@pytest.mark.parametrize("drones", [False, True])
@pytest.mark.parametrize("metric", [True, False])
def test_cam_index_out_of_range_and_repeated(torch_mod, drones, metric):
    """cam_index = [-1, n_pad, c, c] (the Python class refuses all three): DSIM_OK; images 0 and 1 are all background (inf / 1.0, seg
    -1), images 2 and 3 are bit-identical to each other and to a one-camera call on c.  cam_index NULL: n_cam = n_pad is
    accepted, n_pad + 1 refused."""
    torch = torch_mod
    from dronesim_amd import _native as nat
    sc = cr.scene(0)
    env, table = edge_env(torch, sc)
    call = Caller(torch, env, sc, drones)
    pose = next(p for p in table if (p["eye"], p["cam"]) == cr.EDGE_STRIP)
    c, n_pad, dev = call.slot(pose["drone"]), int(env.state.n_pad), env.ctx.device
    flags = (nat.CAM_METRIC if metric else 0) | nat.CAM_GROUND
    res = (17, 17)
    px = res[0] * res[1]
    dep, dep_ptr = guarded(torch, dev, 4 * px, torch.float32, DEP_SENTINEL)
    seg, seg_ptr = guarded(torch, dev, 4 * px, torch.int32, SEG_SENTINEL)
    assert call(res, [-1, n_pad, c, c], 4, dep_ptr, seg_ptr, flags) == 0
    one_d, one_d_ptr = guarded(torch, dev, px, torch.float32, DEP_SENTINEL)
    one_s, one_s_ptr = guarded(torch, dev, px, torch.int32, SEG_SENTINEL)
    assert call(res, [c], 1, one_d_ptr, one_s_ptr, flags) == 0
    for t, s in ((dep, DEP_SENTINEL), (seg, SEG_SENTINEL), (one_d, DEP_SENTINEL), (one_s, SEG_SENTINEL)):
        assert bool((t[:GUARD] == s).all()) and bool((t[-GUARD:] == s).all())
    d4, s4 = dep[GUARD:GUARD + 4 * px].reshape(4, px), seg[GUARD:GUARD + 4 * px].reshape(4, px)
    assert bool((d4[:2] == (float("inf") if metric else 1.0)).all()) and bool((s4[:2] == -1).all())
    assert torch.equal(d4[2], d4[3]) and torch.equal(s4[2], s4[3])
    assert torch.equal(d4[2], one_d[GUARD:GUARD + px]) and torch.equal(s4[2], one_s[GUARD:GUARD + px])
    assert bool((s4[2] >= 0).any()) and bool((s4[2] == cr.SEG_GROUND).any())       # an image with something in it
    # cam_index NULL: camera k is drone k of the storage, n_pad of them at the most
    small = (5, 7)
    dep, dep_ptr = guarded(torch, dev, (n_pad + 1) * 35, torch.float32, DEP_SENTINEL)
    assert call(small, None, n_pad + 1, dep_ptr, None, flags) == -1 and bool((dep == DEP_SENTINEL).all())
    assert call(small, None, n_pad, dep_ptr, None, flags) == 0
    assert bool((dep[GUARD:GUARD + n_pad * 35] != DEP_SENTINEL).all()) and bool((dep[GUARD + n_pad * 35:] == DEP_SENTINEL).all())
    assert bool((dep[:GUARD] == DEP_SENTINEL).all())
    one, one_ptr = guarded(torch, dev, 35, torch.float32, DEP_SENTINEL)
    assert call(small, [c], 1, one_ptr, None, flags) == 0
    assert torch.equal(dep[GUARD:GUARD + n_pad * 35].reshape(n_pad, 35)[c], one[GUARD:GUARD + 35])     # image k is drone k of the storage
    call.close()
