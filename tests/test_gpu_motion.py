"""GPU tests of moving obstacle scenes (dsim_scenes_motion_set, dsim_scenes_move, dsim_scenes_read; DeviceScenes.set_motion /
move / read; CtrlAviary(obstacle_motion=...)): tests/README_motion.md.

1. the moved table against SceneMotion.place(tau), the fp64 restatement, within the DERIVED tolerance of tests/motion_ref.py;
2. every consumer of the table gives, on the moved scenes, bit for bit what it gives on a fresh static scenes created from read();
3. the world actually moved; 4. the refusals through the raw ABI; 5. the env.  Every case runs motions of every kind
(motion_ref.KINDS) and prints its own worst figure before it asserts."""

import numpy as np
import pytest
import torch

from dronesim_amd import params
from tests import motion_ref as mr
from tests.test_gpu_obstacles import load
from tests.util import f32

pytestmark = pytest.mark.gpu
MARGIN = 0.5
N = 300                                    # two tiles of 256 drones, the second partial


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product has no CPU fallback")
    from dronesim_amd import _native as nat
    from dronesim_amd import fleet
    return nat, fleet


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def clock_tensor(ctx, value):
    return torch.tensor([value], dtype=torch.int64, device=ctx.device)


def device_world(fleet, scenes, model="robobee"):
    from dronesim_amd.obstacles import watch_reach
    ctx = fleet.Context([params.builtin_type(model)])
    return ctx, scenes.to_device(ctx, watch_reach(ctx.types, MARGIN))


def fleet_about(motion, tau, n, seed):
    """n drones, scene i mod K (every third: the empty scene): about a placement of their scene where it stands at ``tau``
    (+-0.8 m), or anywhere in the box.  -> (pos32 [n, 3], scene_id [n])."""
    rng = np.random.default_rng(seed)
    s = motion.scenes
    sid = np.arange(n) % s.K
    _, t = motion.pose(tau)
    cnt = s.count[sid]
    g = (rng.uniform(size=n) * np.maximum(cnt, 1)).astype(np.int64)
    at = np.where((cnt > 0)[:, None], np.nan_to_num(t[sid, g]), rng.uniform([-2, -2, 1], [2, 2, 3], (n, 3)))
    return f32(at + rng.uniform(-0.8, 0.8, (n, 3))), sid


# ---- 1. the table against the formula ------------------------------------------------------------------------------------------------
def _table_case(gpu, scenes, motions_of, what, clocks=mr.CLOCKS):
    nat, fleet = gpu
    ctx, dev = device_world(fleet, scenes)
    base = dev.read()
    assert np.array_equal(bits(base[~np.isnan(base)]), bits(scenes.place[~np.isnan(scenes.place)]))
    assert np.array_equal(np.isnan(base), np.isnan(scenes.place))
    worst = 0.0
    for clock in clocks:
        for i, m in enumerate(motions_of(vel_zero=clock >= 2 ** 33)):
            dev.set_motion(m)
            raw = dev.read()                                    # attached, not moved: the base table
            assert np.array_equal(bits(raw), bits(base))
            dev.move(clock_tensor(ctx, clock), mr.DT)
            got = dev.read()
            worst = max(worst, mr.check_table(got, m, mr.DT * clock, f"{what} motion {i} clock {clock}"))
            # unused and static slots: the raw table's, bit for bit
            still = ~m.moving
            assert np.array_equal(bits(got[still]), bits(raw[still]))
            if clock:
                assert not np.array_equal(bits(got[m.moving]), bits(raw[m.moving]))
    dev.set_motion(None)
    assert np.array_equal(bits(dev.read()), bits(base))         # detached: the base table, bit for bit
    with pytest.raises(ValueError):
        dev.move(None, mr.DT)
    dev.close()
    ctx.close()
    return worst


def test_small_table_matches_the_formula_at_every_clock(gpu):
    """K = 3, G = 3, counts (3, 1, 0), clocks 0, 1, 7 and 2^33 (there with vel = 0): at 2^33 a float32 phase would be wrong by
    radians, which the tolerance (2.4e-7 there) does not forgive."""
    _table_case(gpu, mr.small_world(), mr.small_motions, "small")


def test_table_of_1400_slots_matches_the_formula_at_every_clock(gpu):
    """K = 700, G = 2: six blocks, the last partial; counts 2, 1, 0 in turn, every kind 116 times."""
    _table_case(gpu, mr.big_world(), lambda vel_zero: [mr.big_motion(vel_zero)], "1400 slots")


def test_table_beyond_one_sweep_of_the_grid(gpu):
    """524 800 slots: 512 more than SCM_MAX_BLOCKS x SCM_BLOCK, the only size at which the grid stride takes a second turn."""
    w = mr.stride_world()
    assert w.K * w.G == mr.STRIDE_SLOTS + 512
    _table_case(gpu, w, lambda vel_zero: [mr.motion_of_kinds(w, mr.KINDS, 66, vel_zero)], "stride", clocks=(7,))


def test_null_clock_is_zero_and_t_start_shifts(gpu):
    nat, fleet = gpu
    ctx, dev = device_world(fleet, mr.small_world())
    for m in mr.small_motions():
        dev.set_motion(m)
        dev.move(None, mr.DT)
        mr.check_table(dev.read(), m, 0.0, "null clock")
        dev.move(None, mr.DT, t_start=0.25)
        mr.check_table(dev.read(), m, 0.25, "null clock, t_start")
        dev.move(clock_tensor(ctx, 7), mr.DT, t_start=0.25)
        mr.check_table(dev.read(), m, 0.25 + mr.DT * 7, "clock 7, t_start")
    dev.close()
    ctx.close()


# ---- 2. every consumer sees the moved world, bit for bit -----------------------------------------------------------------------------
def _consumers(ctx, st, dev, sid, cams):
    """Everything that reads the scenes' table, on `dev`: a dict of tensors (cloned: the objects' own are overwritten)."""
    from dronesim_amd import obstacles as obs
    from dronesim_amd.camera import DepthCamera
    from dronesim_amd.scanner import RangeScanner
    from dronesim_amd.sight import LineOfSight
    d, n_pad = ctx.device, st.n_pad
    ids = obs.scene_ids_tensor(sid, st.n, n_pad, d)
    out = {}
    clr = torch.full((n_pad,), -7.0, dtype=torch.float32, device=d)
    near = torch.full((n_pad,), -7, dtype=torch.int32, device=d)
    obs.query_scenes(ctx, st, dev, ids, MARGIN, clr, near)
    out["query.clearance"], out["query.nearest"] = clr, near
    wc, wn, tri = torch.full_like(clr, -7.0), torch.full_like(near, -7), torch.full_like(near, -7)
    rel = torch.zeros((3, n_pad), dtype=torch.float32, device=d)
    obs.witness_scenes(ctx, st, dev, ids, MARGIN, wc, wn, rel, tri)
    out["witness.clearance"], out["witness.nearest"], out["witness.rel"], out["witness.triangle"] = wc, wn, rel, tri
    sc = RangeScanner(ctx, st, dev, RangeScanner.fan(8, up=True, down=True), t_max=5.0, scene_id=sid)
    r, h = sc.scan()
    out["scan.ranges"], out["scan.hits"] = r.clone(), h.clone()
    k = 4
    los = LineOfSight(ctx, st, dev, k, scene_id=sid)
    rg = np.random.default_rng(9)
    seg = torch.zeros((k, 3, n_pad), dtype=torch.float32)
    seg[:, :, : st.n] = torch.from_numpy(f32(rg.uniform(-1.5, 1.5, (k, 3, st.n))))
    s = los.query(seg.to(d))
    out["sight.visible"], out["sight.blocker"], out["sight.frac"] = s.visible.clone(), s.blocker.clone(), s.frac.clone()
    cam = DepthCamera(ctx, st, dev, res=(16, 12), cameras=cams, scene_id=sid)
    dep, sg = cam.capture()
    out["camera.dep"], out["camera.seg"] = dep.clone(), sg.clone()
    torch.cuda.synchronize()
    for o in (sc, los, cam):
        o.close()
    return out


def test_every_consumer_sees_the_moved_world_bit_for_bit(gpu):
    """After a move to clock 7, a fresh static DeviceScenes made from read() holds the same R and t (dsim_scenes_create takes that
    layout verbatim); its c_task may differ by an ulp, and the culls built on it decide speed only.  So every consumer must give
    the same bits on both — and, against the scenes at their base, something else."""
    nat, fleet = gpu
    from dronesim_amd.obstacles import ObstacleScenes
    scenes = mr.small_world()
    for i, m in enumerate(mr.small_motions()):
        ctx, dev = device_world(fleet, scenes)
        dev.enable_rays()
        pos, sid = fleet_about(m, mr.DT * 7, N, 70 + i)
        st = load(fleet, ctx, pos)
        assert st.n_pad > N
        cams = list(range(32))                                  # 32 cameras of 16 x 12 pixels, scenes 0 1 2 in turn
        dev.set_motion(m)
        at_base = _consumers(ctx, st, dev, sid, cams)
        dev.move(clock_tensor(ctx, 7), mr.DT)
        moved = _consumers(ctx, st, dev, sid, cams)
        table = dev.read()
        fresh = ObstacleScenes.from_place(scenes.prototype, table, scenes.count).to_device(ctx, prototype_dev=dev.set)
        assert np.array_equal(bits(fresh.read()), bits(table))
        static = _consumers(ctx, st, fresh, sid, cams)
        differ = [k for k in moved if not torch.equal(moved[k], static[k])]
        seen = {k: int((moved[k] != at_base[k]).sum()) for k in moved}
        print(f"consumers, motion {i}: in reach {int((moved['query.nearest'][:N] >= 0).sum())} of {N}, beams hit "
              f"{int((moved['scan.hits'] >= 0).sum())}, segments blocked {int((moved['sight.blocker'] >= 0).sum())}, pixels on a gate "
              f"{int((moved['camera.seg'] >= 0).sum())}; entries that changed against the base table {seen}; differ from static: {differ}")
        assert not differ, differ
        for k in moved:                                          # (bit for bit, NaN-safe: the float outputs as integers)
            if moved[k].dtype == torch.float32:
                assert same_bits(moved[k], static[k]), k
        # the comparison is of something: every consumer hit the world, and saw it move
        assert int((moved["query.nearest"][:N] >= 0).sum()) > N // 4 and int((moved["scan.hits"] >= 0).sum()) > 0
        assert int((moved["sight.blocker"] >= 0).sum()) > 0 and int((moved["camera.seg"] >= 0).sum()) > 0
        for k in ("query.clearance", "witness.rel", "scan.ranges", "sight.frac", "camera.dep"):
            assert seen[k] > 0, k
        fresh.close()
        dev.close()
        ctx.close()


# ---- 3. the world actually moved -----------------------------------------------------------------------------------------------------
def test_clearances_change_where_a_placement_moved_and_nowhere_else(gpu):
    nat, fleet = gpu
    from dronesim_amd import obstacles as obs
    scenes = mr.small_world()
    for i, m in enumerate(mr.small_motions()):
        ctx, dev = device_world(fleet, scenes)
        pos, sid = fleet_about(m, 0.0, N, 80 + i)
        st = load(fleet, ctx, pos)
        ids = obs.scene_ids_tensor(sid, N, st.n_pad, ctx.device)
        dev.set_motion(m)
        got = []
        for clock in (0, 7):
            dev.move(clock_tensor(ctx, clock), mr.DT)
            clr = torch.full((st.n_pad,), -7.0, dtype=torch.float32, device=ctx.device)
            near = torch.full((st.n_pad,), -7, dtype=torch.int32, device=ctx.device)
            obs.query_scenes(ctx, st, dev, ids, MARGIN, clr, near)
            got.append((clr[:N].cpu().numpy(), near[:N].cpu().numpy()))
        (c0, n0), (c7, n7) = got
        still = ~m.moving.any(1)[sid]                            # drones whose scene is static or empty
        assert still.sum() >= N // 3 and (~still).sum() >= N // 3
        assert np.array_equal(bits(c0[still]), bits(c7[still])) and np.array_equal(n0[still], n7[still])
        # near a MOVING placement: the nearest triangle at clock 0 belongs to a moving slot
        nb = scenes.n_bodies
        by_mover = ~still & (n0 >= 0) & m.moving[sid, np.clip(n0, 0, None) // nb]
        changed = bits(c0) != bits(c7)
        print(f"moved world, motion {i}: {int(by_mover.sum())} drones nearest to a moving placement, {int(changed[by_mover].sum())} "
              f"of them changed clearance, max change {np.abs(c7 - c0)[by_mover].max():.3f} m; {int(still.sum())} drones of static "
              f"or empty scenes unchanged")
        assert by_mover.sum() > 30 and changed[by_mover].all()
        dev.close()
        ctx.close()


# ---- 4. refusals through the raw ABI -------------------------------------------------------------------------------------------------
def test_refusals_through_the_raw_abi_leave_the_table_alone(gpu):
    nat, fleet = gpu
    scenes = mr.small_world()
    ctx, dev = device_world(fleet, scenes)
    lib, E_ARG = ctx.lib, -1                                    # DSIM_E_ARG
    base = dev.read()
    good = mr.small_motions()[0]
    clock = clock_tensor(ctx, 7)
    move = lambda dt=mr.DT, t0=0.0: lib.dsim_scenes_move(ctx.handle, ctx.stream_ptr(), dev.handle, clock.data_ptr(), dt, t0)
    set_ = lambda rec: lib.dsim_scenes_motion_set(ctx.handle, dev.handle, rec.ctypes.data)
    # move without a motion
    assert move() == E_ARG and np.array_equal(bits(dev.read()), bits(base))
    # a non-finite record, a non-unit axis, a zero axis that turns: in a used slot, nothing attached and nothing changed
    for field, value in ((0, np.nan), (7, np.inf), (12, -np.inf), (8, 1.5), (11, 1.0)):
        rec = good.records()
        k, g = (1, 0) if field != 11 else (0, 0)                # (0, 0) is the translation: its axis is zero
        rec[k, g, field] = value
        assert set_(rec) == E_ARG, (field, value)
        assert move() == E_ARG and np.array_equal(bits(dev.read()), bits(base))
    # ... in an unused slot it is not looked at
    rec = good.records()
    rec[2, :, :] = np.nan
    rec[1, 1:, :] = np.inf
    assert set_(rec) == 0 and move() == 0
    moved = dev.read()
    mr.check_table(moved, good, mr.DT * 7, "unused records NaN")
    # with a motion attached: a refused set and a refused move change nothing
    bad = good.records()
    bad[0, 1, 8:11] = [1.0, 1.0, 0.0]
    assert set_(bad) == E_ARG and np.array_equal(bits(dev.read()), bits(moved))
    for dt, t0 in ((np.nan, 0.0), (np.inf, 0.0), (mr.DT, np.nan), (mr.DT, -np.inf)):
        clock.fill_(3)
        assert move(dt, t0) == E_ARG and np.array_equal(bits(dev.read()), bits(moved))
    assert lib.dsim_scenes_move(None, ctx.stream_ptr(), dev.handle, clock.data_ptr(), mr.DT, 0.0) == E_ARG
    assert lib.dsim_scenes_move(ctx.handle, ctx.stream_ptr(), None, clock.data_ptr(), mr.DT, 0.0) == E_ARG
    assert lib.dsim_scenes_motion_set(ctx.handle, None, good.records().ctypes.data) == E_ARG
    out = np.empty((3, 3, 12), dtype=np.float32)
    assert lib.dsim_scenes_read(ctx.handle, ctx.stream_ptr(), None, out.ctypes.data) == E_ARG
    assert lib.dsim_scenes_read(ctx.handle, ctx.stream_ptr(), dev.handle, None) == E_ARG
    # the Python layer refuses a motion made for other scenes
    from dronesim_amd.obstacles import ObstacleScenes, SceneMotion
    twin = ObstacleScenes(scenes.prototype, scenes.position, scenes.rpy, scenes.count)
    with pytest.raises(ValueError):
        dev.set_motion(SceneMotion(twin))
    # a second motion starts from the base table: what the first moved and the second leaves alone goes back
    dev.set_motion(mr.small_motions()[1])
    assert np.array_equal(bits(dev.read()), bits(base))
    assert lib.dsim_scenes_motion_set(ctx.handle, dev.handle, None) == 0 and lib.dsim_scenes_motion_set(ctx.handle, dev.handle, None) == 0
    assert move() == E_ARG and np.array_equal(bits(dev.read()), bits(base))
    dev.close()
    ctx.close()


# ---- 5. the env ----------------------------------------------------------------------------------------------------------------------
def _env(motion, sid, xyz, tid, **kw):
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.scanner import RangeScanner
    types = [params.builtin_type("tello"), params.builtin_type("hexa_6DOF")]
    return CtrlAviary(types, len(sid), initial_xyzs=xyz, type_ids=tid, storage="auto", aggregate_phy_steps=5,
                      obstacle_watch=motion.scenes, obstacle_margin=MARGIN, obstacle_scene_id=sid, obstacle_witness="world",
                      range_scan=RangeScanner.fan(4), range_max=5.0, dict_io=False, noise_seed=0, **kw)


def _env_check(env, motion, sid, what):
    """Behind a launch: the table is the formula's at env.scene_time(), and the watch, the witness and the scan are, bit for bit,
    those of a static scenes made from env.scene_placements() on the state read back from the env."""
    from dronesim_amd import obstacles as obs
    from dronesim_amd.scanner import RangeScanner
    table = env.scene_placements()
    mr.check_table(table, motion, env.scene_time(), what)
    ctx, st = env.ctx, env.state
    fresh = obs.ObstacleScenes.from_place(motion.scenes.prototype, table, motion.scenes.count).to_device(ctx, prototype_dev=env._obst.set)
    clr = torch.full((st.n_pad,), -7.0, dtype=torch.float32, device=ctx.device)
    near = torch.full((st.n_pad,), -7, dtype=torch.int32, device=ctx.device)
    rel = torch.zeros((3, st.n_pad), dtype=torch.float32, device=ctx.device)
    obs.witness_scenes(ctx, st, fresh, env._obst_ids, MARGIN, clr, near, rel, None, env._obst_off, env._type_id)
    want_clr, want_near = env._obst_to_caller(clr, near)
    got_clr, got_near = env.last_obstacle_clearance
    assert same_bits(got_clr, want_clr) and torch.equal(got_near, want_near), what
    assert same_bits(env.last_obstacle_witness, env._rel_to_caller(rel)), what
    sc = RangeScanner(ctx, st, fresh, RangeScanner.fan(4), t_max=5.0, ground=True, type_id=env._type_id, scene_id=sid)
    sc.scan()
    assert same_bits(env.ranges, sc.ranges) and torch.equal(env.range_hits, sc.hits), what
    hit = int((env.range_hits >= 0).sum())
    sc.close()
    fresh.close()
    return int((got_near >= 0).sum()), hit


def test_env_moves_the_world_behind_every_kind_of_launch(gpu):
    nat, _ = gpu
    from dronesim_amd.fleet import Targets
    n = N
    tid = (np.arange(n) % 2).astype(np.uint8)
    dt = 5 / 240                                                # one Env.step: aggregate_phy_steps / freq
    for i, m in enumerate(mr.small_motions()):
        xyz, sid = fleet_about(m, 3 * dt, n, 90 + i)
        xyz = xyz.astype(np.float64)
        env = _env(m, sid, xyz, tid, obstacle_motion=m)
        assert env.order is not None and not np.array_equal(env.order.drone_np, np.arange(n))
        assert env.scene_time() == 0.0
        mr.check_table(env.scene_placements(), m, 0.0, f"env {i} made")
        tg = Targets(env.ctx, n)
        tg.set(pos=f32(xyz).T, yaw=0.0)
        steps, seen = 0, []

        def behind(k, what):
            nonlocal steps
            steps += k
            assert env.scene_time() == steps * dt and env._env_steps == steps, what
            seen.append(_env_check(env, m, sid, f"env {i} {what}"))

        env.step(torch.zeros((n, env.n_act), dtype=torch.float32, device=env.ctx.device))
        behind(1, "step()")
        env.step_fused(tg, n_steps=3)
        behind(3, "step_fused(n_steps=3)")
        g = env.capture_fused(tg, 2)
        assert env.scene_time() == steps * dt                   # the eager pass before the capture does not advance the clock
        mr.check_table(env.scene_placements(), m, steps * dt, f"env {i} captured, not replayed")
        g.replay()
        behind(2, "first replay")
        g.replay()
        behind(2, "second replay")
        env.step_fused(tg)
        behind(1, "an eager step after the replays")
        g.replay()                                              # ... and a replay after it finds the clock right
        behind(2, "a replay after an eager step")
        print(f"env {i}: (drones in reach, beams on a gate) behind each launch {seen}")
        assert min(s[0] for s in seen) > n // 8 and min(s[1] for s in seen) > 0
        env.reset()
        assert env.scene_time() == 0.0
        mr.check_table(env.scene_placements(), m, 0.0, f"env {i} reset")
        env.close()


def test_env_without_the_keyword_is_the_env_of_a_motion_of_zeros(gpu):
    """Off by default: no clock, nothing attached.  And a motion of all zeros — every slot static, the kernel writes nothing —
    leaves every output what the env without the keyword gives, bit for bit."""
    nat, _ = gpu
    from dronesim_amd.fleet import Targets
    from dronesim_amd.obstacles import SceneMotion
    n = N
    tid = (np.arange(n) % 2).astype(np.uint8)
    scenes = mr.small_world()
    zeros = SceneMotion(scenes)
    assert not zeros.moving.any()
    xyz, sid = fleet_about(zeros, 0.0, n, 95)
    xyz = xyz.astype(np.float64)
    plain, moved = _env(zeros, sid, xyz, tid), _env(zeros, sid, xyz, tid, obstacle_motion=zeros)
    assert plain._scene_clock is None and plain._motion is None and plain._obst.motion is None and moved._obst.motion is zeros
    for f in (plain.scene_time, plain.scene_placements):
        with pytest.raises(ValueError):
            f()
    for e in (plain, moved):
        tg = Targets(e.ctx, n)
        tg.set(pos=f32(xyz).T, yaw=0.0)
        e.step(torch.zeros((n, e.n_act), dtype=torch.float32, device=e.ctx.device))
        e.step_fused(tg, n_steps=3)
        e.capture_fused(tg, 2).replay()
        torch.cuda.synchronize()
    assert moved.scene_time() == 6 * 5 / 240
    assert np.array_equal(bits(moved.scene_placements()), bits(scenes.place)) and np.array_equal(bits(plain._obst.read()), bits(scenes.place))
    assert torch.equal(plain.state.fields(0, 13), moved.state.fields(0, 13))
    for a, b in zip(plain.last_obstacle_clearance + (plain.last_obstacle_witness, plain.ranges, plain.range_hits),
                    moved.last_obstacle_clearance + (moved.last_obstacle_witness, moved.ranges, moved.range_hits)):
        assert same_bits(a, b) if a.dtype == torch.float32 else torch.equal(a, b)
    assert int((plain.last_obstacle_clearance[1] >= 0).sum()) > n // 8
    assert plain.obstacle_contacts() == moved.obstacle_contacts()
    plain.close()
    moved.close()
