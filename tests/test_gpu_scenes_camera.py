"""The placed depth camera on the device (dsim_depth_image_scenes, DepthCamera(scenes, scene_id=...), CtrlAviary(vision_scene=scenes))
against camera_ref.cast on the union of the placed triangles with instance-major bodies (tests/scenes_ref.py).

Fleet: camera_ref's 70 drones (tello and hexa_6DOF_simple interleaved, stored type-major, with task offsets) with a sixth camera on
drone 21; K = 3 scenes of G = 3 placements of camera_ref.scene (108 triangles: records in LDS; 1548: through L2), cameras on scenes
0, 2, 1, 0, 1, 1, every other drone without a scene.  Scene 2 is built so that the nearest hit of camera 1 lies in the LAST placement
in front of a hit in the first one, and the reverse: `best` must carry across placements.  Outside the reference's ambiguity mask (at
most 1 % of every image, asserted) hit / no-hit and the instance-major body are equal and |t - t_ref| <= IMAGE_TOL t_ref /
max(|n . d|, 0.05), IMAGE_TOL = 4 x the float32 restatement's recorded error (tests/README_scenes.md)."""
import numpy as np
import pytest

import __graft_entry__ as graft
from tests import camera_ref as cr
from tests import scenes_ref as sr
from tests.camera_check import check_image

pytestmark = pytest.mark.gpu
FAR = 1000.0


@pytest.fixture(scope="module")
def torch_mod():
    graft.build()
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product has no CPU fallback")
    return torch


def make_env(torch, models=None, **kw):
    from dronesim_amd.envs import CtrlAviary
    st, _, off, _, sid = sr.camera_fleet()
    mixed = models is None
    models = [cr.FLEET_MODELS[i % 2] for i in range(cr.FLEET_N)] if mixed else models
    env = CtrlAviary(models, cr.FLEET_N, initial_xyzs=st[:, :3].astype(np.float64), noise_seed=0, dict_io=False, ground_plane=False, **kw)
    assert (env.order is not None) == mixed
    env.state.set_fields(0, torch.from_numpy(np.ascontiguousarray(st.T)))
    return env, off, sid


# between them the cases launch the four PLACED instances <LDS, SEG>: (108 triangles | 1548) x (seg_out | NULL)
CASES = [
    # subdiv, res, ground, metric, seg
    (0, (64, 48), False, True, True),
    (0, (17, 17), True, False, True),
    (0, (64, 48), True, True, False),
    (2, (64, 48), True, True, True),
    (2, (17, 17), False, False, False),
    (2, (17, 17), True, False, True),
]


@pytest.mark.parametrize("subdiv, res, ground, metric, with_seg", CASES)
def test_placed_images_against_the_brute_force_reference(torch_mod, subdiv, res, ground, metric, with_seg):
    torch = torch_mod
    from dronesim_amd.camera import DepthCamera
    env, off, sid = make_env(torch)
    scenes = sr.camera_scenes(subdiv)
    assert (scenes.prototype.n_tri <= 512) == (subdiv == 0)
    cam = DepthCamera(env.ctx, env.state, scenes, res=res, far=FAR, ground=ground, metric=metric, cameras=sr.CAMERAS, offsets=off,
                      type_id=env._type_id, scene_id=sid)
    cam.seg.fill_(-77)
    dep, seg = cam.capture(seg=with_seg)
    torch.cuda.synchronize()
    assert tuple(dep.shape) == (6, res[1], res[0]) and dep.dtype == torch.float32
    if not with_seg:
        assert seg is None and bool((cam.seg == -77).all())  # seg_out NULL: nothing written
    dep_h, seg_h = dep.cpu().numpy(), (seg.cpu().numpy() if with_seg else None)
    refs = sr.reference_images(subdiv, res)
    _, _, _, arms, _ = sr.camera_fleet()
    hits = 0
    for k, L in enumerate(arms):
        ref = refs[k][1 if ground else 0]
        check_image(k, dep_h[k], seg_h[k] if with_seg else None, ref, L, metric, tol=sr.IMAGE_TOL)
        hits += int((ref["seg"] >= 0).sum())
    assert hits > (1500 if res == (64, 48) else 150)          # the scenes are in view
    if with_seg:
        assert set(np.unique(seg_h)) == ({-2} if ground else set()) | {-1, 0, 1, 2, 3, 4, 5}
    if with_seg and res == (64, 48):
        # camera 1 on scene 2: where a ray hits slot 0 and, nearer, slot 2, the image shows slot 2 (bodies 4, 5), and the reverse
        first_behind, last_behind = sr.carry_pixels(subdiv, res)
        ok = ~refs[1][0]["ambiguous"]
        assert (first_behind & ok).sum() >= 20 and (last_behind & ok).sum() >= 10
        assert np.isin(seg_h[1][first_behind & ok], (4, 5)).all() and np.isin(seg_h[1][last_behind & ok], (0, 1)).all()
    cam.close()
    env.close()


def test_identity_scene_against_the_unplaced_camera(torch_mod):
    """K = 1, G = 1, R = I, t = 0 on the device set the unplaced camera uses: seg equal everywhere, t within the bar of the same
    fp64 reference (and whether the bits were equal is printed: the rotated basis is formed from products with 0 and 1)."""
    torch = torch_mod
    from dronesim_amd.camera import DepthCamera
    from dronesim_amd.obstacles import ObstacleScenes
    env, off, _ = make_env(torch)
    sc = cr.scene(0)
    scenes = ObstacleScenes(sc, np.zeros((1, 1, 3)), np.zeros((1, 1, 3)))
    placed = DepthCamera(env.ctx, env.state, scenes, far=FAR, ground=True, metric=True, cameras=sr.CAMERAS, offsets=off,
                         type_id=env._type_id, scene_id=np.zeros(cr.FLEET_N, dtype=int))
    plain = DepthCamera(env.ctx, env.state, placed.set.set, far=FAR, ground=True, metric=True, cameras=sr.CAMERAS, offsets=off,
                        type_id=env._type_id)
    d1, s1 = (x.clone() for x in placed.capture())
    d0, s0 = (x.clone() for x in plain.capture())
    torch.cuda.synchronize()
    assert torch.equal(s1, s0) and bool((s0 >= 0).any()) and bool((s0 == cr.SEG_GROUND).any())
    same = torch.equal(d1.view(torch.int32), d0.view(torch.int32))
    print(f"identity scene: depth bits equal to the unplaced camera's: {same}"
          + ("" if same else f" ({int((d1.view(torch.int32) != d0.view(torch.int32)).sum())} of {d0.numel()} pixels differ)"))
    _, (pos, quat), _, arms, _ = sr.camera_fleet()
    for k, L in enumerate(arms):
        ref = cr.reference_image(sc.triangles, sc.body, pos[k], quat[k], L, 64, 48, far=FAR, ground=True)
        for d, s in ((d1, s1), (d0, s0)):
            check_image(k, d[k].cpu().numpy(), s[k].cpu().numpy(), ref, L, True, tol=sr.IMAGE_TOL)
    placed.close()
    env.close()


def test_empty_and_absent_scenes_show_the_plane_or_nothing(torch_mod):
    torch = torch_mod
    from dronesim_amd.camera import DepthCamera
    from dronesim_amd.obstacles import ObstacleScenes
    env, off, _ = make_env(torch)
    pos, rpy = np.zeros((2, 2, 3)), np.zeros((2, 2, 3))
    pos[0], rpy[0] = np.nan, np.nan
    scenes = ObstacleScenes(cr.scene(0), pos, rpy, [0, 2])
    sid = np.full(cr.FLEET_N, -1)
    sid[list(sr.CAMERAS)] = (0, 2, -5, 0, 2 ** 31 - 1, 1)           # empty, out of range either way; the last camera sees scene 1
    _, (cpos, cquat), _, arms, _ = sr.camera_fleet()
    none_tri, none_body = np.zeros((0, 3, 3), np.float32), np.zeros(0, np.int64)
    for ground in (False, True):
        cam = DepthCamera(env.ctx, env.state, scenes, far=FAR, ground=ground, metric=True, cameras=sr.CAMERAS, offsets=off,
                          type_id=env._type_id, scene_id=sid)
        dep, seg = (x.cpu().numpy() for x in cam.capture())
        for k in range(5):
            ref = cr.reference_image(none_tri, none_body, cpos[k], cquat[k], arms[k], 64, 48, far=FAR, ground=ground)
            check_image(k, dep[k], seg[k], ref, arms[k], True, tol=sr.IMAGE_TOL)
            assert set(np.unique(seg[k])) <= {-2, -1} and (ground or np.isinf(dep[k]).all())
        assert (seg[5] >= 0).any()
        cam.close()
    env.close()


def test_library_refuses_bad_placed_calls(torch_mod):
    torch = torch_mod
    from dronesim_amd.camera import camera_reach
    from dronesim_amd import _native as nat
    import ctypes
    env, _, sid = make_env(torch)
    scenes = sr.camera_scenes(0)
    dev = scenes.to_device(env.ctx, camera_reach(env.ctx.types))
    lib, h = env.ctx.lib, env.ctx.handle
    dep = torch.full((2, 48, 64), -7.0, dtype=torch.float32, device=env.ctx.device)
    ids = torch.zeros((env.state.n_pad,), dtype=torch.int32, device=env.ctx.device)
    par = nat.CameraParams(64, 48, 60.0, 1.0, FAR, 0)
    call = lambda s, i, p=par: lib.dsim_depth_image_scenes(h, env.ctx.stream_ptr(), env.state.view(), s, i, ctypes.byref(p), 2, None, None,
                                                           env._type_id.data_ptr(), dep.data_ptr(), None)
    assert call(dev.handle, ids.data_ptr()) == -1                  # rays not enabled on the prototype
    dev.enable_rays()
    assert call(None, ids.data_ptr()) == -1 and call(dev.handle, None) == -1
    assert call(dev.handle, ids.data_ptr(), nat.CameraParams(0, 48, 60.0, 1.0, FAR, 0)) == -1
    torch.cuda.synchronize()
    assert bool((dep == -7.0).all())
    assert call(dev.handle, ids.data_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((dep != -7.0).all())
    dev.close()
    env.close()


def test_env_images_equal_a_direct_camera(torch_mod):
    """vision_attributes=True, vision_scene=scenes: env.dep / env.seg behind a due step are the images a DepthCamera of its own
    gives on the same state, in the caller's numbering; with obstacle_watch=scenes as well, watch and camera share the device scenes."""
    torch = torch_mod
    from dronesim_amd.camera import DepthCamera
    from dronesim_amd.fleet import Targets
    scenes = sr.camera_scenes(0)
    _, _, off, _, sid = sr.camera_fleet()
    env, _, _ = make_env(torch, freq=240, aggregate_phy_steps=5, vision_attributes=True, vision_scene=scenes, vision_drones=sr.CAMERAS,
                         obstacle_watch=scenes, obstacle_margin=0.5, obstacle_offsets=off, obstacle_scene_id=sid)
    assert env._vision.set is env._obst and env._vision.placed
    assert env.IMG_CAPTURE_FREQ == 10 and tuple(env.dep.shape) == (6, 48, 64)
    assert bool((env.dep == 1.0).all()) and bool((env.seg == -1).all())
    tgt = Targets(env.ctx, cr.FLEET_N)
    st = sr.camera_fleet()[0]
    tgt.set(pos=(st[:, :3] + np.array([0.3, 0.0, 0.2])).T.astype(np.float64), yaw=np.zeros(cr.FLEET_N))
    env.step_fused(tgt)
    assert bool((env.dep == 1.0).all())                            # step_counter 5: not due
    env.step_fused(tgt)                                            # 10: due
    own = DepthCamera(env.ctx, env.state, env._obst, ground=True, cameras=sr.CAMERAS, offsets=off, type_id=env._type_id, scene_id=sid)
    want_dep, want_seg = (x.clone() for x in own.capture())
    torch.cuda.synchronize()
    assert torch.equal(env.dep, want_dep) and torch.equal(env.seg, want_seg)
    assert bool((want_seg >= 2).any()) and bool((want_seg == cr.SEG_GROUND).any())
    dep, seg = env.drone_images()
    torch.cuda.synchronize()
    assert dep is env.dep and torch.equal(dep, want_dep) and torch.equal(seg, want_seg)
    clr, near = env.last_obstacle_clearance                        # (the watch ran on the shared scenes behind the same steps)
    assert clr.shape == (cr.FLEET_N,) and int(near.max()) < 6
    env.close()
