"""The drones in the camera's images on the device (dsim_depth_image_drones, DepthCamera(drones=True),
CtrlAviary(vision_see_drones=True)) against the fp64 brute-force casters of tests/camera_ref.py and tests/camera_drones_ref.py,
which walk no grid.

Outside the union of the triangle mask and the sphere mask (at most 1 % of an image, asserted) hit / no-hit and seg are equal —
a drone as -3 - its number in the CALLER's numbering — and |t - t_ref| <= tol t_ref / max(|n . d|, 0.05) with tol = SPHERE_TOL where a
sphere wins (4 x the error of the float32 restatement of the kernel's sphere arithmetic) and KERNEL_TOL elsewhere."""
import ctypes

import numpy as np
import pytest

import __graft_entry__ as graft
from tests import camera_drones_ref as dr
from tests import camera_ref as cr
from tests.camera_check import check_image

pytestmark = pytest.mark.gpu
FAR = dr.FAR


@pytest.fixture(scope="module")
def torch_mod():
    graft.build()
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch


_REF = {}


def main_ref(subdiv, res, with_offsets, **kw):
    key = (subdiv, res, with_offsets, tuple(sorted(kw)))
    if kw or key not in _REF:
        r = dr.main_reference(subdiv, res, with_offsets, **kw)
        if kw:
            return r
        _REF[key] = r
    return _REF[key]


def make_env(torch, with_offsets, stored=None, models=None, **kw):
    from dronesim_amd.envs import CtrlAviary
    st, off, mixed_models, _ = dr.main_fleet(with_offsets)
    st = st if stored is None else stored
    models = mixed_models if models is None else models
    env = CtrlAviary(models, cr.FLEET_N, initial_xyzs=np.nan_to_num(st[:, :3]).astype(np.float64), noise_seed=0, dict_io=False,
                     ground_plane=False, **kw)
    env.state.set_fields(0, torch.from_numpy(np.ascontiguousarray(st.T)))
    return env, off


# between them the cases launch the six instances <LDS, SEG, DRONES, TRIS>: (108 triangles | 1548 | no set) x (seg_out | NULL)
CASES = [
    # subdiv, res, offsets, ground, metric, seg
    (0, (64, 48), False, False, True, True),
    (0, (20, 12), True, True, False, False),
    (2, (64, 48), True, True, True, True),
    (2, (20, 12), False, False, False, False),
    (None, (64, 48), False, True, True, True),
    (None, (20, 12), True, False, False, False),
    (0, (64, 48), True, True, False, True),
]


@pytest.mark.parametrize("subdiv, res, with_offsets, ground, metric, with_seg", CASES)
def test_images_against_the_brute_force_reference(torch_mod, subdiv, res, with_offsets, ground, metric, with_seg):
    torch = torch_mod
    from dronesim_amd.camera import DepthCamera
    env, off = make_env(torch, with_offsets)
    assert env.order is not None                              # type-major storage: not the caller's order
    sc = cr.scene(subdiv) if subdiv is not None else None
    cam = DepthCamera(env.ctx, env.state, sc, res=res, far=FAR, ground=ground, metric=metric, cameras=cr.CAMERAS, offsets=off,
                      type_id=env._type_id, drones=True)
    cam.seg.fill_(-77)
    dep, seg = cam.capture(seg=with_seg)
    torch.cuda.synchronize()
    if not with_seg:
        assert seg is None and bool((cam.seg == -77).all())
    dep_h, seg_h = dep.cpu().numpy(), (seg.cpu().numpy() if with_seg else None)
    refs = main_ref(subdiv, res, with_offsets)
    drone_px = front = behind = 0
    for k, L in enumerate(cr.camera_arms()):
        ref = refs[k][1 if ground else 0]
        check_image(k, dep_h[k], seg_h[k] if with_seg else None, ref, L, metric)
        drone_px += int(ref["is_drone"].sum())
    assert drone_px > (100 if res == (64, 48) else 10)        # drones are in view
    assert cam.drones_outside() == 0                          # the measured box holds the fleet
    if with_seg:
        d = DepthCamera.seg_drone(seg_h)
        assert set(np.unique(d[d >= 0])) <= set(range(cr.FLEET_N))
        assert np.array_equal(DepthCamera.seg_drone(seg).cpu().numpy(), d)
        for k, c in enumerate(cr.CAMERAS):
            assert not (d[k] == c).any()                      # nobody sees its own drone
    if subdiv is not None and res == (64, 48) and not with_offsets and with_seg:
        # drone pixels in front of triangles, and triangles in front of drones (against the images without the one or the other)
        plain = DepthCamera(env.ctx, env.state, cam.set, res=res, far=FAR, ground=ground, metric=True, cameras=cr.CAMERAS,
                            type_id=env._type_id)
        bare = DepthCamera(env.ctx, env.state, None, res=res, far=FAR, ground=ground, metric=True, cameras=cr.CAMERAS,
                           type_id=env._type_id, drones=True)
        tri_seg, dr_seg = plain.capture()[1].cpu().numpy(), bare.capture()[1].cpu().numpy()
        front, behind = int(((seg_h <= -3) & (tri_seg >= 0)).sum()), int(((seg_h >= 0) & (dr_seg <= -3)).sum())
        assert front > 50 and behind > 50, (front, behind)
    cam.close()
    env.close()


@pytest.mark.parametrize("rng", [20.0, None])
def test_long_walks_on_a_lattice(torch_mod, rng):
    """4 096 tellos, 1 m pitch: rays that cross tens of cells before they hit, the early exit, the range cut (hits at 20 .. 53 m with
    no range, none beyond 20 m with it); no obstacle set."""
    torch = torch_mod
    from dronesim_amd.camera import DepthCamera
    from dronesim_amd.envs import CtrlAviary
    st = dr.lattice_fleet()
    env = CtrlAviary(["tello"], dr.LATTICE_N, initial_xyzs=st[:, :3].astype(np.float64), noise_seed=0, dict_io=False, ground_plane=False)
    env.state.set_fields(0, torch.from_numpy(np.ascontiguousarray(st.T)))
    cam = DepthCamera(env.ctx, env.state, None, far=FAR, metric=True, cameras=dr.LATTICE_CAMERAS, drones=True, drone_range=rng)
    dep, seg = cam.capture()
    torch.cuda.synchronize()
    a = cam._grid_args
    assert a.nx * a.ny > 1000 and a.cell >= 2.0 * float(dr.type_radii(["tello"])[0])     # many cells to walk
    dep_h, seg_h = dep.cpu().numpy(), seg.cpu().numpy()
    far_px = 0
    for k, ref in enumerate(dr.lattice_reference(rng)):
        check_image(k, dep_h[k], seg_h[k], ref, cr.ARM["tello"], True)
        far_px += int((ref["t"][ref["is_drone"]] > 20.0).sum())
    assert (far_px > 40) if rng is None else (far_px == 0)
    assert cam.drones_outside() == 0
    env.close()


def test_drones_outside_a_pinned_box_are_drawn_all_the_same(torch_mod):
    torch = torch_mod
    from dronesim_amd.camera import DepthCamera
    env, _ = make_env(torch, False)
    st = dr.main_fleet(False)[0]
    box = (0.0, -2.6, 4.2, 2.6)                               # with the grid's margin x > 4.85 m is outside: about a dozen of the
    xy = st[:, :2]                                            # 65, and the camera 60 m off
    cam = DepthCamera(env.ctx, env.state, cr.scene(0), far=FAR, metric=True, cameras=cr.CAMERAS, type_id=env._type_id, drones=True,
                      drone_box=box)
    dep, seg = cam.capture()
    torch.cuda.synchronize()
    a = cam._grid_args
    # the library's box is [xmin, xmin + nx cell] x [ymin, ymin + ny cell]: count against it
    x1, y1 = a.xmin + a.nx * a.cell, a.ymin + a.ny * a.cell
    want = int(((xy[:, 0] < a.xmin) | (xy[:, 0] >= x1) | (xy[:, 1] < a.ymin) | (xy[:, 1] >= y1)).sum())
    assert 5 <= want <= 20 and cam.drones_outside() == want
    dep_h, seg_h = dep.cpu().numpy(), seg.cpu().numpy()
    refs = main_ref(0, (64, 48), False)
    seen_outside = 0
    for k, L in enumerate(cr.camera_arms()):
        check_image(k, dep_h[k], seg_h[k], refs[k][0], L, True)
        ids = DepthCamera.seg_drone(seg_h[k])
        seen_outside += int(np.isin(ids[ids >= 0], np.nonzero((xy[:, 0] >= x1) | (xy[:, 0] < a.xmin))[0]).sum())
    assert seen_outside > 0                                   # some of them are in view
    cam.capture()
    assert cam.drones_outside() == 2 * want                   # += per capture
    cam.close()
    env.close()


def test_exclusions(torch_mod):
    """A type with collision_sphere = 0 is invisible; a NaN position among the drones changes no other pixel; a degenerate camera
    still gets the no-hit image."""
    torch = torch_mod
    import dataclasses
    from dronesim_amd.camera import DepthCamera
    from dronesim_amd.params import builtin_type
    st, _, models, rad = dr.main_fleet(False)
    # the hexas made spheres of radius 0: only tellos are drawn
    hexa0 = dataclasses.replace(builtin_type("hexa_6DOF_simple"), collision_sphere=0.0)
    env, _ = make_env(torch, False, models=[builtin_type("tello") if i % 2 == 0 else hexa0 for i in range(cr.FLEET_N)])
    cam = DepthCamera(env.ctx, env.state, cr.scene(0), far=FAR, metric=True, cameras=cr.CAMERAS, type_id=env._type_id, drones=True)
    dep, seg = cam.capture()
    torch.cuda.synchronize()
    rad0 = np.where(np.arange(cr.FLEET_N) % 2 == 0, rad, 0.0).astype(np.float32)
    refs = main_ref(0, (64, 48), False, radius=rad0)
    ids = DepthCamera.seg_drone(seg.cpu().numpy())
    assert (ids[ids >= 0] % 2 == 0).all() and (ids >= 0).sum() > 50
    for k, L in enumerate(cr.camera_arms()):
        check_image(k, dep[k].cpu().numpy(), seg[k].cpu().numpy(), refs[k][0], L, True)
    cam.close()
    env.close()
    # NaN positions among the drones, a NaN and a vertical camera
    env, _ = make_env(torch, False)
    good = DepthCamera(env.ctx, env.state, cr.scene(0), far=FAR, metric=True, cameras=cr.CAMERAS, type_id=env._type_id, drones=True)
    want_dep, want_seg = (x.clone() for x in good.capture())
    torch.cuda.synchronize()
    lost = [i for i in range(cr.FLEET_N) if i not in cr.CAMERAS][:4]
    unseen = ~np.isin(DepthCamera.seg_drone(want_seg.cpu().numpy()), lost)
    st2 = st.copy()
    st2[lost[0], 0], st2[lost[1], 1], st2[lost[2], 2] = np.nan, np.nan, np.inf
    cams = list(cr.CAMERAS) + lost[:1] + [lost[3]]            # a camera without a position, and one with a position ...
    st2[lost[3], 3:] = cr.quat_from_rpy(0.0, np.pi / 2, 0.0)  # ... whose vehicle is pitched to the vertical
    assert np.isfinite(st2[lost[3]]).all()
    lost = lost[:3]
    env.state.set_fields(0, torch.from_numpy(np.ascontiguousarray(st2.T)))
    cam = DepthCamera(env.ctx, env.state, good.set, far=FAR, metric=True, cameras=cams, type_id=env._type_id, drones=True)
    dep, seg = cam.capture()                                  # (nat.check: DSIM_OK)
    torch.cuda.synchronize()
    assert bool((seg[5:] == -1).all()) and bool(torch.isinf(dep[5:]).all())
    d5, s5 = dep[:5].cpu().numpy(), seg[:5].cpu().numpy()
    assert np.array_equal(d5[unseen], want_dep.cpu().numpy()[unseen]) and np.array_equal(s5[unseen], want_seg.cpu().numpy()[unseen])
    assert not np.isin(DepthCamera.seg_drone(s5), lost).any() and (~unseen).sum() > 0
    refs = main_ref(0, (64, 48), False, stored=st2)
    for k, L in enumerate(cr.camera_arms()):
        check_image(k, d5[k], s5[k], refs[k][0], L, True)
    good.close()
    env.close()


def test_the_default_is_unchanged(torch_mod):
    """DepthCamera(..., drones=False) and dsim_depth_image give the triangle-only images: the reference's, and bit for bit those of
    a second capture through the old entry point, with drones all over the scene."""
    torch = torch_mod
    from dronesim_amd import _native as nat
    from dronesim_amd.camera import DepthCamera
    env, _ = make_env(torch, False)
    sc = cr.scene(0)
    cam = DepthCamera(env.ctx, env.state, sc, far=FAR, ground=True, cameras=cr.CAMERAS, type_id=env._type_id)
    assert cam.drones is False
    dep, seg = (x.clone() for x in cam.capture())
    with_drones = DepthCamera(env.ctx, env.state, cam.set, far=FAR, ground=True, cameras=cr.CAMERAS, type_id=env._type_id, drones=True)
    dd, ds = with_drones.capture()                            # (the new call in between: it disturbs nothing)
    dep2 = torch.empty_like(dep)
    seg2 = torch.empty_like(seg)
    p = nat.CameraParams(64, 48, 60.0, 1.0, FAR, nat.CAM_GROUND)
    nat.check(env.ctx.lib.dsim_depth_image(env.ctx.handle, env.ctx.stream_ptr(), env.state.view(), cam.set.handle, ctypes.byref(p), 5,
                                           cam._index.data_ptr(), None, env._type_id.data_ptr(), dep2.data_ptr(), seg2.data_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(dep, dep2) and torch.equal(seg, seg2)
    assert int(seg.min()) == -2 and not torch.equal(seg, ds) and int(ds.min()) <= -3
    st = dr.main_fleet(False)[0]
    hits = 0
    for k, (c, L) in enumerate(zip(cr.CAMERAS, cr.camera_arms())):
        ref = cr.reference_image(sc.triangles, sc.body, st[c, :3], st[c, 3:], L, 64, 48, far=FAR, ground=True)
        ref["is_drone"] = np.zeros((48, 64), bool)
        check_image(k, dep[k].cpu().numpy(), seg[k].cpu().numpy(), ref, L, False)
        hits += int((ref["seg"] >= 0).sum())
    assert hits > 300
    cam.close()
    env.close()


def test_library_refuses_bad_calls(torch_mod):
    torch = torch_mod
    from dronesim_amd import _native as nat
    from dronesim_amd.camera import DepthCamera
    env, _ = make_env(torch, False)
    cam = DepthCamera(env.ctx, env.state, None, cameras=cr.CAMERAS, type_id=env._type_id, drones=True)
    cam.capture()
    lib, h, a = env.ctx.lib, env.ctx.handle, cam._grid_args
    p = nat.CameraParams(64, 48, 60.0, 1.0, FAR, 0)

    def call(d, params=p, type_id=env._type_id.data_ptr(), out=cam.dep.data_ptr()):
        return lib.dsim_depth_image_drones(h, env.ctx.stream_ptr(), env.state.view(), None, ctypes.byref(params), 5, cam._index.data_ptr(),
                                           None, type_id, ctypes.byref(d), out, None)

    def drones(**kw):
        g = nat.DownwashArgs.from_buffer_copy(a)
        d = nat.CameraDrones()
        d.range = 20.0
        for k, v in kw.items():
            if k in ("range", "radius_all"):
                setattr(d, k, v)
            else:
                setattr(g, k, v)
        d._g = g
        d.grid = ctypes.addressof(g)
        return d
    assert call(drones()) == 0
    for bad in (dict(range=0.0), dict(range=float("nan")), dict(cell=0.0), dict(cell=0.01), dict(nx=0), dict(m=10 ** 6),
                dict(workspace=None), dict(workspace_len=a.workspace_len // 4), dict(type_id=None), dict(radius_all=cam.dep.data_ptr())):
        assert call(drones(**bad)) == -1, bad
    assert call(drones(), params=nat.CameraParams(0, 48, 60.0, 1.0, FAR, 0)) == -1
    assert call(drones(), type_id=None) == -1 and call(drones(), out=None) == -1
    halo = nat.HaloPlan()
    assert call(drones(halo=ctypes.addressof(halo))) == -5    # DSIM_E_UNSUPPORTED
    torch.cuda.synchronize()
    cam.close()
    env.close()


def test_env_sees_drones_in_the_callers_numbering(torch_mod):
    """CtrlAviary(vision_attributes=True, vision_see_drones=True): env.seg holds drone labels of the caller's numbering behind
    env.step; vision_scene=None works; the on-demand images equal a camera of one's own."""
    torch = torch_mod
    from dronesim_amd.camera import DepthCamera
    env, _ = make_env(torch, False, freq=240, aggregate_phy_steps=10, vision_attributes=True, vision_see_drones=True,
                      vision_drones=cr.CAMERAS, vision_ground=False)
    assert env._vision.set is None and env._vision.drones
    dep, seg = env.drone_images()
    torch.cuda.synchronize()
    refs = main_ref(None, (64, 48), False)
    for k, L in enumerate(cr.camera_arms()):
        check_image(k, dep[k].cpu().numpy(), seg[k].cpu().numpy(), refs[k][0], L, False)
    from dronesim_amd.fleet import Targets
    tgt = Targets(env.ctx, cr.FLEET_N)
    tgt.set(pos=dr.main_fleet(False)[0][:, :3].T.astype(np.float64), yaw=np.zeros(cr.FLEET_N))
    env.seg.fill_(-1)
    env.step_fused(tgt)                                       # cadence 1: the step is followed by a capture
    torch.cuda.synchronize()
    assert bool((env.seg <= -3).any())
    env.seg.fill_(-1)
    env.step(np.full((cr.FLEET_N, env.n_act), 0.4, dtype=np.float32))      # BaseAviary.step: the same watch behind it
    torch.cuda.synchronize()
    ids = DepthCamera.seg_drone(env.seg.cpu().numpy())
    seen = set(np.unique(ids[ids >= 0]))
    assert len(seen) > 10 and seen <= set(range(cr.FLEET_N))
    # the labels are the caller's: the drones the reference of the (barely moved) fleet shows are the ones seen
    want = set(np.unique(np.concatenate([DepthCamera.seg_drone(refs[k][0]["seg"]).ravel() for k in range(5)]))) - {-1}
    assert len(seen & want) >= 0.8 * len(want)
    env.close()


def test_env_captured_graph_reproduces_the_eager_images(torch_mod):
    """Cadence 1 (240 Hz, AGGR_PHY_STEPS = 10): the capture is part of the graph, with the box the eager capture in front of it
    measured; the replay leaves the images eager stepping leaves (one type: eager and captured flights are the same bits)."""
    torch = torch_mod
    from dronesim_amd.fleet import Targets
    sc = cr.scene(0)
    out = []
    for graph in (False, True):
        env, _ = make_env(torch, False, models=["tello"], freq=240, aggregate_phy_steps=10, vision_attributes=True, vision_scene=sc,
                          vision_drones=cr.CAMERAS, vision_see_drones=True, vision_drone_range=30.0)
        tgt = Targets(env.ctx, cr.FLEET_N)
        st = dr.main_fleet(False)[0]
        tgt.set(pos=(st[:, :3] + np.array([0.3, 0.0, 0.2])).T.astype(np.float64), yaw=np.zeros(cr.FLEET_N))
        env.step_fused(tgt)
        if graph:
            g = env.capture_fused(tgt, 3)
            g.replay()
            g.replay()
        else:
            for _ in range(6):
                env.step_fused(tgt)
        torch.cuda.synchronize()
        out.append((env.dep.cpu().numpy().copy(), env.seg.cpu().numpy().copy(), env.state.rigid_aos()))
        env.close()
    assert np.array_equal(out[0][2], out[1][2])               # the same flight
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert (out[0][1] <= -3).any() and (out[0][1] >= 0).any()


def test_a_graph_keeps_the_drone_grid_workspace_it_captured(torch_mod):
    """The captured captures bin and scatter into the workspace the drones' grid had at capture time.  An eager capture that
    later needs a larger one (the fleet spread, the box was re-measured) replaces the camera's: the graph holds the old tensor, so
    a replay writes into memory that is still its own, and leaves the images of the state it left."""
    torch = torch_mod
    from dronesim_amd.camera import DepthCamera
    from dronesim_amd.fleet import Targets
    sc = cr.scene(0)
    env, _ = make_env(torch, False, models=["tello"], freq=240, aggregate_phy_steps=10, vision_attributes=True, vision_scene=sc,
                      vision_drones=cr.CAMERAS, vision_see_drones=True)
    tgt = Targets(env.ctx, cr.FLEET_N)
    st = dr.main_fleet(False)[0]
    tgt.set(pos=st[:, :3].T.astype(np.float64), yaw=np.zeros(cr.FLEET_N))
    env.step_fused(tgt)
    g = env.capture_fused(tgt, 2)
    grid = env._vision._grid
    old = grid._ws
    assert any(t is old for t in g._keepalive_vision) and any(t is env._vision._outside for t in g._keepalive_vision)
    ptr, numel = old.data_ptr(), old.numel()
    grid._ws = None                                           # what outgrowing it does: the camera lets go of the tensor
    del old
    env._vision.refresh_drone_box()
    env.drone_images()                                        # eager: a new workspace
    filler = [torch.full((numel,), 7, dtype=torch.int32, device=env.ctx.device) for _ in range(8)]     # takers of a freed block
    torch.cuda.synchronize()
    assert grid._ws is not None and grid._ws.data_ptr() != ptr and all(f.data_ptr() != ptr for f in filler)
    g.replay()
    torch.cuda.synchronize()
    assert all(bool((f == 7).all()) for f in filler)          # nobody's memory was written
    own = DepthCamera(env.ctx, env.state, env._vision.set, ground=True, cameras=cr.CAMERAS, drones=True)
    dep, seg = own.capture()
    torch.cuda.synchronize()
    assert torch.equal(dep, env.dep) and torch.equal(seg, env.seg) and bool((seg <= -3).any())
    env.close()


@pytest.mark.parametrize("graph", [False, True])
def test_env_with_the_downwash_term_and_drones_in_view(torch_mod, graph):
    """Physics.PYB_DW with vision_see_drones: the drones' binning drops the context's downwash bookkeeping behind every step, the
    next query bins the fleet itself.  Eager (240 Hz, ten sub-steps, the term per sub-step) and captured (40 Hz, one sub-step,
    cadence 1): the force is what a fleet without a camera gets, and the images are those of the state the steps left."""
    torch = torch_mod
    from dronesim_amd.camera import DepthCamera
    from dronesim_amd.envs import Physics
    from dronesim_amd.fleet import Targets
    kw = dict(freq=40, aggregate_phy_steps=1) if graph else dict(freq=240, aggregate_phy_steps=10)
    st = dr.main_fleet(False)[0]
    out = []
    for see in (True, False):
        vis = dict(vision_attributes=True, vision_drones=cr.CAMERAS, vision_see_drones=True) if see else {}
        env, _ = make_env(torch, False, models=["tello"], physics=Physics.PYB_DW, **kw, **vis)
        tgt = Targets(env.ctx, cr.FLEET_N)
        tgt.set(pos=st[:, :3].T.astype(np.float64), yaw=np.zeros(cr.FLEET_N))
        env.step_fused(tgt)
        if graph:
            g = env.capture_fused(tgt, 2)
            g.replay()
            g.replay()
        else:
            for _ in range(4):
                env.step_fused(tgt)
        torch.cuda.synchronize()
        out.append((env.state.rigid_aos(), env._downwash.force.cpu().numpy().copy()))
        if see:
            own = DepthCamera(env.ctx, env.state, None, ground=True, cameras=cr.CAMERAS, drones=True)
            dep, seg = own.capture()
            torch.cuda.synchronize()
            assert torch.equal(dep, env.dep) and torch.equal(seg, env.seg) and bool((seg <= -3).any())
        env.close()
    assert np.abs(out[0][1]).max() > 0.0                      # the term acts in this cluster
    # with and without the camera: the same forces and the same flight (the sums' order is not pinned: to rounding)
    np.testing.assert_allclose(out[0][1], out[1][1], rtol=1e-4, atol=1e-9)
    np.testing.assert_allclose(out[0][0], out[1][0], rtol=1e-4, atol=1e-5)
