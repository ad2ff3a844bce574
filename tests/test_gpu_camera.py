"""The depth camera on the device (dsim_depth_image, DepthCamera, CtrlAviary(vision_attributes=True)) against the fp64 brute-force
caster of tests/camera_ref.py, which walks no grid.

Fleet: 70 drones, tello and hexa_6DOF_simple interleaved (arms 0.0635 / 1.0635 m; stored type-major, so storage order differs
from the caller's); cameras on drones 40, 7, 68, 12, 33 in that order: inside the ray grid's box, outside looking in, outside
looking away, 60 m off, rolled and pitched.  Outside the reference's ambiguity mask (at most 1 % of an image, asserted) hit /
no-hit and the body index are equal and |t - t_ref| <= KERNEL_TOL t_ref / max(|n . d|, 0.05), KERNEL_TOL = 4 x the error of the
float32 restatement of the kernel's arithmetic (tests/README_camera.md).  A depth-buffer image is mapped back to t; the float32 depth
value itself is granted 3 ulp of 1.0 (reciprocal, product, store), which the map back to t magnifies by t^2 (far - near) /
(far near)."""
import numpy as np
import pytest

import __graft_entry__ as graft
from tests import camera_ref as cr
from tests.camera_check import check_image

pytestmark = pytest.mark.gpu
FAR = 1000.0


@pytest.fixture(scope="module")
def torch_mod():
    graft.build()
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch


_REF = {}


def reference(subdiv, res):
    """(without ground, with ground) x the five cameras, computed once per (set, resolution): the poses are the same numbers
    with and without offsets (camera_ref.fleet_offsets)."""
    key = (subdiv, res)
    if key not in _REF:
        sc = cr.scene(subdiv)
        pos, quat = cr.camera_poses()
        _REF[key] = [cr.reference_image(sc.triangles, sc.body, pos[k], quat[k], L, res[0], res[1], far=FAR, ground="both")
                     for k, L in enumerate(cr.camera_arms())]
    return _REF[key]


def make_env(torch, with_offsets, models=None, **kw):
    from dronesim_amd.envs import CtrlAviary
    st, _, off = cr.fleet_state(with_offsets)
    mixed = models is None
    models = [cr.FLEET_MODELS[i % 2] for i in range(cr.FLEET_N)] if mixed else models
    env = CtrlAviary(models, cr.FLEET_N, initial_xyzs=st[:, :3].astype(np.float64), noise_seed=0, dict_io=False, ground_plane=False, **kw)
    assert (env.order is not None) == mixed                   # the mixed fleet is stored type-major: not the caller's order
    env.state.set_fields(0, torch.from_numpy(np.ascontiguousarray(st.T)))
    return env, off


# between them the cases launch the four instances <LDS, SEG>: (108 triangles | 1548) x (seg_out | NULL)
CASES = [
    # subdiv, res, offsets, ground, metric, seg
    (0, (64, 48), False, False, True, True),
    (0, (20, 12), True, True, False, True),
    (0, (64, 48), True, True, True, False),
    (2, (64, 48), False, True, True, True),
    (2, (20, 12), True, False, False, False),
    (2, (64, 48), True, False, True, True),
]


@pytest.mark.parametrize("subdiv, res, with_offsets, ground, metric, with_seg", CASES)
def test_images_against_the_brute_force_reference(torch_mod, subdiv, res, with_offsets, ground, metric, with_seg):
    torch = torch_mod
    from dronesim_amd.camera import DepthCamera
    env, off = make_env(torch, with_offsets)
    sc = cr.scene(subdiv)
    assert (sc.n_tri <= 512) == (subdiv == 0)
    cam = DepthCamera(env.ctx, env.state, sc, res=res, far=FAR, ground=ground, metric=metric, cameras=cr.CAMERAS, offsets=off,
                      type_id=env._type_id)
    cam.seg.fill_(-77)
    dep, seg = cam.capture(seg=with_seg)
    torch.cuda.synchronize()
    assert tuple(dep.shape) == (5, res[1], res[0]) and dep.dtype == torch.float32
    if not with_seg:
        assert seg is None and bool((cam.seg == -77).all())  # seg_out NULL: nothing written
    dep_h, seg_h = dep.cpu().numpy(), (seg.cpu().numpy() if with_seg else None)
    refs = reference(subdiv, res)
    hits = 0
    for k, L in enumerate(cr.camera_arms()):
        ref = refs[k][1 if ground else 0]
        check_image(k, dep_h[k], seg_h[k] if with_seg else None, ref, L, metric)
        hits += int(np.isfinite(ref["t"]).sum())
    assert hits > (300 if res == (64, 48) else 30)            # the scene is in view
    if with_seg and not ground:
        assert set(np.unique(seg_h)) == {-1, 0, 1}
    if with_seg and ground:
        assert cr.SEG_GROUND in np.unique(seg_h)
    cam.close()
    env.close()


def test_degenerate_cameras_give_background_and_disturb_nobody(torch_mod):
    """A NaN position, a NaN quaternion and vehicles pitched to exactly +-90 degrees: all-background images, DSIM_OK, and the
    other cameras of the same launch give what they give alone."""
    torch = torch_mod
    from dronesim_amd.camera import DepthCamera
    env, _ = make_env(torch, False)
    sc = cr.scene(0)
    cams = list(cr.CAMERAS) + [2, 3, 4, 5]
    good = DepthCamera(env.ctx, env.state, sc, ground=True, cameras=cr.CAMERAS, type_id=env._type_id)
    want_dep, want_seg = (x.clone() for x in good.capture())
    st = cr.fleet_state(False)[0]
    st[2, 0] = np.nan
    st[3, 4] = np.nan
    st[4, 3:] = cr.quat_from_rpy(0.0, np.pi / 2, 0.0)
    st[5, 3:] = cr.quat_from_rpy(0.0, -np.pi / 2, 0.7)
    env.state.set_fields(0, torch.from_numpy(np.ascontiguousarray(st.T)))
    for metric in (False, True):
        cam = DepthCamera(env.ctx, env.state, good.set, ground=True, metric=metric, cameras=cams, type_id=env._type_id)
        dep, seg = cam.capture()                              # (nat.check: the call returned DSIM_OK)
        torch.cuda.synchronize()
        assert bool((seg[5:] == -1).all())
        assert bool((dep[5:] == (float("inf") if metric else 1.0)).all())
        if not metric:
            assert torch.equal(dep[:5], want_dep) and torch.equal(seg[:5], want_seg)
    assert bool((want_seg == cr.SEG_GROUND).any()) and bool((want_seg >= 0).any())
    good.close()
    env.close()


def test_library_refuses_bad_calls(torch_mod):
    torch = torch_mod
    import ctypes
    from dronesim_amd import _native as nat
    env, _ = make_env(torch, False)
    sc = cr.scene(0)
    from dronesim_amd.camera import camera_reach
    dev = sc.to_device(env.ctx, camera_reach(env.ctx.types))
    lib, h = env.ctx.lib, env.ctx.handle
    dep = torch.empty((2, 48, 64), dtype=torch.float32, device=env.ctx.device)
    tid = env._type_id.data_ptr()

    def call(p, n_cam=2, type_id=tid, out=dep.data_ptr()):
        return lib.dsim_depth_image(h, env.ctx.stream_ptr(), env.state.view(), dev.handle, ctypes.byref(p), n_cam, None, None, type_id,
                                    out, None)
    ok = nat.CameraParams(64, 48, 60.0, 1.0, 1000.0, 0)
    assert call(ok) == -1                                     # no rays enabled yet
    dev.enable_rays()
    dev.enable_rays()                                         # DSIM_OK when it already has them
    assert call(ok) == 0
    for bad in (nat.CameraParams(0, 48, 60.0, 1.0, 1000.0, 0), nat.CameraParams(64, 1025, 60.0, 1.0, 1000.0, 0),
                nat.CameraParams(64, 48, 60.0, 1.0, 0.0, 0), nat.CameraParams(64, 48, 60.0, 1.0, -5.0, 0)):
        assert call(bad) == -1
    assert call(ok, n_cam=0) == -1 and call(ok, type_id=None) == -1 and call(ok, out=None) == -1
    torch.cuda.synchronize()
    dev.close()
    env.close()


def test_env_cadence_on_demand_and_stream(torch_mod):
    """240 Hz, AGGR_PHY_STEPS = 5: IMG_CAPTURE_FREQ = 10 physics steps, so env.dep is refreshed behind every second Env.step and
    untouched behind the others; drone_images() equals a direct DepthCamera on the same state; the capture is on the env's
    stream (a step enqueued right behind it, with no synchronisation, does not disturb the image)."""
    torch = torch_mod
    from dronesim_amd.camera import DepthCamera
    from dronesim_amd.fleet import Targets
    sc = cr.scene(0)
    env, _ = make_env(torch, False, freq=240, aggregate_phy_steps=5, vision_attributes=True, vision_scene=sc, vision_drones=cr.CAMERAS)
    assert env.IMG_CAPTURE_FREQ == 10 and tuple(env.dep.shape) == (5, 48, 64) and tuple(env.seg.shape) == (5, 48, 64)
    assert bool((env.dep == 1.0).all()) and bool((env.seg == -1).all())
    tgt = Targets(env.ctx, cr.FLEET_N)
    st = cr.fleet_state(False)[0]
    tgt.set(pos=(st[:, :3] + np.array([0.3, 0.0, 0.2])).T.astype(np.float64), yaw=np.zeros(cr.FLEET_N))
    ptr = env.dep.data_ptr()
    changed = []
    for k in range(6):
        before = env.dep.clone()
        env.step_fused(tgt)
        changed.append(not torch.equal(before, env.dep))
        assert env.dep.data_ptr() == ptr
    assert changed == [False, True, False, True, False, True], changed
    # on demand, against a camera of its own on the same state; then a step right behind the capture, no sync in between
    own = DepthCamera(env.ctx, env.state, sc, ground=True, cameras=cr.CAMERAS, type_id=env._type_id)
    want_dep, want_seg = (x.clone() for x in own.capture())
    dep, seg = env.drone_images()
    keep_dep, keep_seg = dep.clone(), seg.clone()             # (stream-ordered copies, enqueued before the step below)
    env.step_fused(tgt)                                       # step_counter 35: no capture falls due
    torch.cuda.synchronize()
    assert dep is env.dep and seg is env.seg
    assert torch.equal(keep_dep, want_dep) and torch.equal(keep_seg, want_seg)
    assert torch.equal(env.dep, want_dep)                     # ... and the step behind it left the image alone
    assert bool((want_seg >= 0).any())
    # a launch of several Env.steps captures once, at its end, when a capture fell due inside it
    before = env.dep.clone()
    env.step_fused(tgt, n_steps=3)                            # 35 -> 50: 40 and 50 lie inside
    direct = tuple(x.clone() for x in own.capture())
    torch.cuda.synchronize()
    assert not torch.equal(before, env.dep) and torch.equal(env.dep, direct[0]) and torch.equal(env.seg, direct[1])
    with pytest.raises(NotImplementedError, match="cadence"):
        env.capture_fused(tgt, 2)
    own.close()
    env.close()


def test_env_captured_graph_at_cadence_one(torch_mod):
    """240 Hz, AGGR_PHY_STEPS = 10: a capture behind every Env.step, part of the captured graph; the replay leaves the images
    eager stepping leaves (a fleet of one type, whose eager and captured flights are the same bits), and they are the images of
    the state the replay left."""
    torch = torch_mod
    from dronesim_amd.camera import DepthCamera
    from dronesim_amd.fleet import Targets
    sc = cr.scene(0)
    out = []
    for graph in (False, True):
        env, _ = make_env(torch, False, models=["tello"], freq=240, aggregate_phy_steps=10, vision_attributes=True, vision_scene=sc,
                          vision_drones=cr.CAMERAS, obstacle_watch=sc)
        assert env._vision.set is env._obst                   # one device set for the watch and the camera
        tgt = Targets(env.ctx, cr.FLEET_N)
        st = cr.fleet_state(False)[0]
        tgt.set(pos=(st[:, :3] + np.array([0.3, 0.0, 0.2])).T.astype(np.float64), yaw=np.zeros(cr.FLEET_N))
        env.step_fused(tgt)
        if graph:
            g = env.capture_fused(tgt, 3)
            g.replay()
        else:
            for _ in range(3):
                env.step_fused(tgt)
        torch.cuda.synchronize()
        out.append((env.dep.cpu().numpy().copy(), env.seg.cpu().numpy().copy(), env.state.rigid_aos()))
        own = DepthCamera(env.ctx, env.state, env._obst, ground=True, cameras=cr.CAMERAS)
        dep, seg = own.capture()
        assert torch.equal(dep, env.dep) and torch.equal(seg, env.seg)
        env.close()
    assert np.array_equal(out[0][2], out[1][2])               # the same flight
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert (out[0][1] >= 0).any()


def test_env_without_the_keywords_has_no_camera(torch_mod):
    torch = torch_mod
    env, _ = make_env(torch, False)
    assert not hasattr(env, "dep") and not hasattr(env, "seg") and env._vision is None and not hasattr(env, "IMG_CAPTURE_FREQ")
    with pytest.raises(ValueError, match="vision_attributes"):
        env.drone_images()
    env.close()
