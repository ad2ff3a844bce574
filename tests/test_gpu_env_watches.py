"""The three services that follow a step (drone_watch, obstacle_watch, the depth camera with the other drones in view) on ONE env
answer, bit for bit, what each answers alone on an env of its own that flies the same commands."""
import numpy as np
import pytest
import torch

from tests.test_gpu_obstacles import _gate_fleet

pytestmark = pytest.mark.gpu

N = 48             # no multiple of 64: padded lanes; two interleaved types: type-major storage, the caller-numbering paths


def _state(env):
    return env.state.rigid_aos(), env.state.mem_aos()


def test_three_services_on_one_env_answer_what_each_answers_alone():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product has no CPU fallback")
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.fleet import Targets
    s, xyz, off = _gate_fleet(N)
    watch = dict(drone_watch=True)
    obst = dict(obstacle_watch=s, obstacle_offsets=off)
    cam = dict(vision_attributes=True, vision_see_drones=True, vision_res=(16, 12))

    def make(**kw):
        e = CtrlAviary(["robobee", "tello"] * (N // 2), N, initial_xyzs=xyz, freq=240, aggregate_phy_steps=5, noise_seed=0,
                       dict_io=False, **kw)
        assert e.order is not None
        tg = Targets(e.ctx, N)
        tg.set(pos=(xyz + np.array([0.3, -0.2, 0.25])).T.astype(np.float32), yaw=0.0)
        return e, tg

    both, tg_both = make(**watch, **obst, **cam)
    alone = {"watch": make(**watch), "obst": make(**obst), "cam": make(vision_scene=s, obstacle_offsets=off, **cam)}
    assert both.IMG_CAPTURE_FREQ == 10                             # a capture behind every second Env.step
    action = torch.full((N, 4), 0.4, dtype=torch.float32, device=both.ctx.device)
    for k in range(6):
        for e, tg in [(both, tg_both)] + list(alone.values()):
            if k < 4:
                e.step_fused(tg)
            else:
                e.step(action)
        torch.cuda.synchronize()
        for name, (e, _) in alone.items():
            for a, b in zip(_state(both), _state(e)):
                assert np.array_equal(a, b), (k, name)
        for a, b in zip(both.last_clearance, alone["watch"][0].last_clearance):
            assert torch.equal(a, b), k
        for a, b in zip(both.last_obstacle_clearance, alone["obst"][0].last_obstacle_clearance):
            assert torch.equal(a, b), k
        assert torch.equal(both.dep, alone["cam"][0].dep) and torch.equal(both.seg, alone["cam"][0].seg), k
        if k == 0:
            assert bool((both.dep == 1.0).all())                   # not due yet
        if k == 1:
            assert bool((both.dep < 1.0).any())                    # ... and captured
    assert float(both.last_clearance[0].min()) < 1.0 and float(both.last_obstacle_clearance[0].min()) < 1.0    # in reach of each other
    assert both.drone_contacts() == alone["watch"][0].drone_contacts()
    assert both.obstacle_contacts() == alone["obst"][0].obstacle_contacts()
    for e, _ in [(both, None)] + list(alone.values()):
        e.close()
