"""GPU tests of the placed static-obstacle watch (dsim_obstacle_clearance_scenes, ObstacleScenes, obstacles.query_scenes,
CtrlAviary(obstacle_watch=scenes, obstacle_scene_id=...)) against the fp64 brute force of tests/scenes_ref.py: the point into
every placement's frame with the float32 R and t the device holds, then obstacle_ref.tri_dist on the prototype.

Input rule and comparisons are those of tests/test_gpu_obstacles.py (re-draw within GUARD = 1e-4 m of 0 or of the margin, at most
1 %; counts and the -1 status exact; `nearest` exact outside ties), with ATOL = 4 x the float32 restatement's recorded error
(tests/README_scenes.md) and the instance-major body index g n_bodies + body.  The conditions on the inputs are asserted on the
reference alone by tests/test_scenes_cpu.py; every case prints the device's own worst difference before it asserts."""
import numpy as np
import pytest
import torch

from dronesim_amd import params
from tests import scenes_ref as sr
from tests.obstacle_ref import brute
from tests.test_gpu_obstacles import MT_FAR, MT_N, MT_NEAR, _gate_world, check_many_tiles, load, many_tiles_far, soa3
from tests.util import f32

pytestmark = pytest.mark.gpu
ATOL = sr.ATOL


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product has no CPU fallback")
    from dronesim_amd import _native as nat
    from dronesim_amd import fleet
    return nat, fleet


def ids_tensor(sid, n_pad, dev):
    t = torch.full((n_pad,), -1, dtype=torch.int32)
    t[: len(sid)] = torch.from_numpy(np.clip(np.asarray(sid), -1, 2 ** 31 - 1).astype(np.int32))
    return t.to(dev)


def run(ctx, st, dev_scenes, ids, margin, off=None, tid=None, counter=None):
    from dronesim_amd import obstacles as obs
    clr = torch.full((st.n_pad,), -7.0, dtype=torch.float32, device=ctx.device)
    near = torch.full((st.n_pad,), -7, dtype=torch.int32, device=ctx.device)
    obs.query_scenes(ctx, st, dev_scenes, ids, margin, clr, near, off, tid, counter)
    return clr, near


def check(got_clr, got_near, ref, margin, what=""):
    clr, near, gap = ref["clr"], ref["near"], ref["gap"]
    got_clr, got_near = got_clr.cpu().numpy().astype(np.float64), got_near.cpu().numpy().astype(np.int64)
    err = np.abs(got_clr - clr).max()
    print(f"placed clearance {what}: max |got - ref| = {err:.3e} m (ATOL {ATOL:.3e}) over {clr.size} drones, "
          f"{int((near >= 0).sum())} in reach, {ref['contacts']} in contact, min {clr.min():.4f}")
    np.testing.assert_array_equal(got_near >= 0, near >= 0)
    np.testing.assert_allclose(got_clr, clr, rtol=0, atol=ATOL)
    assert np.all(got_clr[near < 0] == np.float32(margin))
    tie = (near >= 0) & (gap < ATOL)
    assert tie.mean() <= 0.01, tie.mean()
    np.testing.assert_array_equal(got_near[~tie], near[~tie])
    return err


# ---- 1. identity: bit for bit the unplaced query -----------------------------------------------------------------------------------
def test_identity_scene_is_the_unplaced_query_bit_for_bit(gpu):
    """K = 1, G = 1, R = I, t = 0: every product with 0 and 1 is exact, so clearance, nearest and the counter are those of
    dsim_obstacle_clearance on the same device set.  700 drones: three tiles, the last partial, n < n_pad; one position NaN."""
    nat, fleet = gpu
    from dronesim_amd import obstacles as obs
    t = params.builtin_type("robobee")
    n, margin = 700, 1.0
    s, rad, pos, _ = _gate_world(n, margin, [t], np.zeros(n, dtype=int), False, 11)
    ctx = fleet.Context([t])
    scenes = obs.ObstacleScenes(s, np.zeros((1, 1, 3)), np.zeros((1, 1, 3)))
    dev = scenes.to_device(ctx, obs.watch_reach(ctx.types, margin))
    st = load(fleet, ctx, pos)
    assert st.n_pad > n
    nan_at = 333
    p = torch.from_numpy(np.ascontiguousarray(pos.T)).clone()
    p[0, nan_at] = float("nan")
    st.set_fields(0, p)
    ids = ids_tensor(np.zeros(n, dtype=int), st.n_pad, ctx.device)
    want_clr = torch.full((st.n_pad,), -7.0, dtype=torch.float32, device=ctx.device)
    want_near = torch.full((st.n_pad,), -7, dtype=torch.int32, device=ctx.device)
    c0, c1 = (torch.zeros((1,), dtype=torch.int64, device=ctx.device) for _ in range(2))
    obs.query(ctx, st, dev.set, margin, want_clr, want_near, None, None, c0)
    before = ctx.query(nat.QUERY_OBSTACLE_CONTACTS)
    clr, near = run(ctx, st, dev, ids, margin, counter=c1)
    assert torch.equal(clr.view(torch.int32), want_clr.view(torch.int32)) and torch.equal(near, want_near)
    assert int(c1.item()) == int(c0.item()) == ctx.query(nat.QUERY_OBSTACLE_CONTACTS) - before > 50
    assert bool((clr[n:] == -7.0).all()) and bool((near[n:] == -7).all())       # the sentinels beyond n are untouched
    assert float(clr[nan_at]) == np.float32(margin) and int(near[nan_at]) == -1
    ref = brute(np.delete(pos, nan_at, 0), s.triangles, s.body, np.delete(rad, nan_at), margin)
    keep = np.arange(n) != nan_at
    np.testing.assert_allclose(clr[:n].cpu().numpy()[keep], ref[0], rtol=0, atol=ATOL)
    dev.close()
    ctx.close()


# ---- 2. placed gates against brute force ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offsets", [False, True])
def test_placed_gates_vs_bruteforce(gpu, offsets):
    nat, fleet = gpu
    from dronesim_amd.obstacles import watch_reach
    d = sr.case_gates(offsets)
    ref, n, margin = d["ref"], len(d["scene_id"]), d["margin"]
    assert d["redrawn"] <= 0.01 and sr.tie_fraction(ref) <= 0.01 and (ref["n_near"] >= 2).sum() >= 20 and ref["contacts"] >= 0.01 * n
    ctx = fleet.Context([params.builtin_type("robobee")])
    dev = d["scenes"].to_device(ctx, watch_reach(ctx.types, margin))
    for layout in ("soa", "tile64"):
        st = load(fleet, ctx, d["pos"], layout)
        cnt = torch.zeros((1,), dtype=torch.int64, device=ctx.device)
        before = ctx.query(nat.QUERY_OBSTACLE_CONTACTS)
        clr, near = run(ctx, st, dev, ids_tensor(d["scene_id"], st.n_pad, ctx.device), margin,
                        soa3(d["off"], st.n_pad, ctx.device) if offsets else None, None, cnt)
        check(clr[:n], near[:n], ref, margin, f"gates {layout} offsets={offsets}")
        assert int(cnt.item()) == ref["contacts"] == ctx.query(nat.QUERY_OBSTACLE_CONTACTS) - before
    dev.close()
    ctx.close()


# ---- 3. ragged and absent ----------------------------------------------------------------------------------------------------------
def test_ragged_counts_and_absent_scenes(gpu):
    """Counts (0, 1, 2, 3, 8) of G = 8, ids from -1 to K: the empty scene and the ids out of range give exactly (float32(margin),
    -1); the slots at or above a count are NaN on the host and never reach a result."""
    nat, fleet = gpu
    from dronesim_amd.obstacles import watch_reach
    d = sr.case_ragged()
    ref, sid, n, margin = d["ref"], d["scene_id"], len(d["scene_id"]), d["margin"]
    ctx = fleet.Context([params.builtin_type("robobee")])
    dev = d["scenes"].to_device(ctx, watch_reach(ctx.types, margin))
    st = load(fleet, ctx, d["pos"])
    clr, near = run(ctx, st, dev, ids_tensor(sid, st.n_pad, ctx.device), margin, soa3(d["off"], st.n_pad, ctx.device))
    check(clr[:n], near[:n], ref, margin, "ragged")
    c_, n_ = clr[:n].cpu().numpy(), near[:n].cpu().numpy()
    none = (sid < 1) | (sid >= 5)
    assert np.all(c_[none] == np.float32(margin)) and np.all(n_[none] == -1) and np.isfinite(c_).all()
    assert ctx.query(nat.QUERY_OBSTACLE_CONTACTS) == ref["contacts"]
    # ids far out of range, of either sign: the same defined case
    wild = torch.full((st.n_pad,), 2 ** 31 - 1, dtype=torch.int32, device=ctx.device)
    wild[::2] = -(2 ** 31)
    clr, near = run(ctx, st, dev, wild, margin)
    assert bool((clr[:n] == np.float32(margin)).all()) and bool((near[:n] == -1).all())
    dev.close()
    ctx.close()


# ---- 4. the large prototype: records through L2, four bodies ---------------------------------------------------------------------
def test_soup_prototype_instance_major_bodies(gpu):
    nat, fleet = gpu
    from dronesim_amd.obstacles import watch_reach
    d = sr.case_soup()
    ref, n, margin = d["ref"], len(d["scene_id"]), d["margin"]
    assert d["scenes"].prototype.n_tri > 512 and set(ref["near"][ref["near"] >= 0]) == set(range(8))
    ctx = fleet.Context([params.builtin_type("hexa_6DOF")])
    dev = d["scenes"].to_device(ctx, watch_reach(ctx.types, margin))
    st = load(fleet, ctx, d["pos"])
    clr, near = run(ctx, st, dev, ids_tensor(d["scene_id"], st.n_pad, ctx.device), margin)
    check(clr[:n], near[:n], ref, margin, "soup")
    assert ctx.query(nat.QUERY_OBSTACLE_CONTACTS) == ref["contacts"]
    dev.close()
    ctx.close()


# ---- 4b. more tiles than workgroups (test_gpu_obstacles.py, 3b) ---------------------------------------------------------------------
def test_many_tiles_per_workgroup(gpu):
    """K = 4 scenes of G = 2 gates within +-2 m, scene_id = i mod K for every drone; the far drones stand out of reach of every
    placement's bounding sphere, so nobody of their tiles has a bit in its mask."""
    nat, fleet = gpu
    from dronesim_amd.obstacles import ObstacleScenes, watch_reach
    K, G, margin, k = 4, 2, 0.5, len(MT_NEAR)
    rng = np.random.default_rng(71)
    scenes = ObstacleScenes(sr.gate(), rng.uniform(-2.0, 2.0, (K, G, 3)), rng.uniform([-0.5, -0.5, -np.pi], [0.5, 0.5, np.pi], (K, G, 3)))
    sid = np.arange(MT_N) % K
    sid_near, rad = sid[MT_NEAR], sr._radius("robobee", k)
    draw = lambda rg, idx: sr._drones_about(rg, scenes, sid_near, idx, False)
    decide = lambda p, o: (sr.brute_scenes(p, scenes, sid_near, rad, margin, o)["raw"], margin)
    p_near, _, frac = sr.settle(rng, draw, k, decide)
    assert frac <= 0.01, frac
    ref = sr.brute_scenes(p_near, scenes, sid_near, rad, margin)
    pos = many_tiles_far(np.random.default_rng(72))
    pos[MT_NEAR] = p_near
    ctx = fleet.Context([params.builtin_type("robobee")])
    dev = scenes.to_device(ctx, watch_reach(ctx.types, margin))
    tri = scenes.prototype.triangles.reshape(-1, 3).astype(np.float64)
    centre, half_diag = 0.5 * (tri.min(0) + tri.max(0)), 0.5 * np.linalg.norm(tri.max(0) - tri.min(0))
    for kk in range(K):
        for g in range(G):
            R, t = sr.placement64(scenes, kk, g)
            assert (np.linalg.norm(pos[MT_FAR] - (R @ centre + t), axis=1) - half_diag).min() > dev.reach
    for lo_, hi_ in ((256, 512), (524288, 524544), (524544, MT_N)):      # each of the three tiles has drones in reach
        assert (ref["near"][(MT_NEAR >= lo_) & (MT_NEAR < hi_)] >= 0).any(), (lo_, hi_)
    assert ref["contacts"] > 0 and sr.tie_fraction(ref) <= 0.01
    st = load(fleet, ctx, pos)
    cnt = torch.zeros((1,), dtype=torch.int64, device=ctx.device)
    before = ctx.query(nat.QUERY_OBSTACLE_CONTACTS)
    clr, near = run(ctx, st, dev, ids_tensor(sid, st.n_pad, ctx.device), margin, counter=cnt)
    check_many_tiles(clr, near, ref, margin, check, "many tiles")
    assert int(cnt.item()) == ref["contacts"] == ctx.query(nat.QUERY_OBSTACLE_CONTACTS) - before
    dev.close()
    ctx.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(gpu):
    import ctypes
    nat, fleet = gpu
    from dronesim_amd.obstacles import ObstacleScenes, watch_reach
    ctx = fleet.Context([params.builtin_type("robobee")])
    margin = 0.5
    scenes = ObstacleScenes(sr.gate(), np.zeros((2, 2, 3)), np.zeros((2, 2, 3)))
    dev = scenes.to_device(ctx, watch_reach(ctx.types, margin))
    st = load(fleet, ctx, f32(np.zeros((64, 3))))
    clr = torch.full((st.n_pad,), -7.0, dtype=torch.float32, device=ctx.device)
    near = torch.full((st.n_pad,), -7, dtype=torch.int32, device=ctx.device)
    ids = ids_tensor(np.zeros(64, dtype=int), st.n_pad, ctx.device)
    call = lambda h, i, m: ctx.lib.dsim_obstacle_clearance_scenes(ctx.handle, ctx.stream_ptr(), st.n, st.view(), h, i, None, None, m,
                                                                  clr.data_ptr(), near.data_ptr(), None)
    assert call(dev.handle, ids.data_ptr(), 0.0) == -1 and call(dev.handle, ids.data_ptr(), float("nan")) == -1
    assert call(dev.handle, ids.data_ptr(), margin * 1.01) == -1              # R_max + margin > reach of the prototype's grid
    assert call(None, ids.data_ptr(), margin) == -1 and call(dev.handle, None, margin) == -1
    torch.cuda.synchronize()
    assert bool((clr == -7.0).all()) and bool((near == -7).all()) and ctx.query(nat.QUERY_OBSTACLE_CONTACTS) == 0
    assert call(dev.handle, ids.data_ptr(), margin) == 0 and call(dev.handle, ids.data_ptr(), 0.25) == 0
    # dsim_scenes_create: limits, counts, and an R that is not a rotation
    h = ctypes.c_void_p()
    eye = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=np.float32), (2, 2, 1))
    make = lambda pl, cnt, K, G: ctx.lib.dsim_scenes_create(ctx.handle, dev.set.handle, pl.ctypes.data,
                                                            cnt.ctypes.data if cnt is not None else None, K, G, ctypes.byref(h))
    assert make(eye, None, 2, 0) == -1 and make(eye, None, 0, 2) == -1 and make(eye, None, 2, 33) == -1
    assert make(eye, None, (1 << 22) // 2 + 1, 2) == -1 and not h
    assert make(eye, np.array([2, 3], dtype=np.int32), 2, 2) == -1 and make(eye, np.array([-1, 0], dtype=np.int32), 2, 2) == -1
    for k, v in ((0, 1.0 + 1e-4), (1, 1e-4), (9, np.nan), (4, np.inf)):       # stretched, sheared, not finite
        bad = eye.copy()
        bad[1, 1, k] = v
        assert make(bad, None, 2, 2) == -1 and not h
        assert make(bad, np.array([2, 1], dtype=np.int32), 2, 2) == 0             # ... unless the slot is not used
        assert ctx.lib.dsim_scenes_destroy(ctx.handle, h) == 0
        h = ctypes.c_void_p()
    mirror = eye.copy()
    mirror[0, 0, 8] = -1.0                                                     # orthonormal, det = -1
    assert make(mirror, None, 2, 2) == -1 and not h
    near_rot = eye.copy()
    near_rot[0, 0, 1], near_rot[0, 0, 3] = 4e-6, -4e-6                         # orthonormal to 1e-5: served
    assert make(near_rot, None, 2, 2) == 0 and ctx.lib.dsim_scenes_destroy(ctx.handle, h) == 0
    dev.close()
    ctx.close()


# ---- 5. env, mixed fleet -----------------------------------------------------------------------------------------------------------
def _env_world(n, K, seed):
    """Robobee and tello interleaved; K scenes of 3 gates; every drone about its own scene's gates, in a frame of its own."""
    from dronesim_amd.obstacles import ObstacleScenes
    types = [params.builtin_type("robobee"), params.builtin_type("tello")]
    tid = (np.arange(n) % 2).astype(np.uint8)
    rad = np.array([np.float32(t.collision_sphere) for t in types])[tid]
    pos, rpy = sr.random_placements(np.random.default_rng(seed), K, 3)
    scenes = ObstacleScenes(sr.gate(), pos, rpy)
    sid = (np.arange(n) * 5 + 3) % K                                # (not i mod K: ids and types must not line up)
    side = int(np.ceil(np.sqrt(n)))
    off = np.stack([np.arange(n) % side, np.arange(n) // side, np.zeros(n)], 1).astype(np.float64) * 8.0
    return types, tid, rad, scenes, sid, off


def test_env_mixed_fleet_answers_in_caller_numbering(gpu):
    nat, _ = gpu
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.fleet import Targets
    n, K, margin = 96, 8, 0.5
    types, tid, rad, scenes, sid, off = _env_world(n, K, 51)
    off32 = f32(off)

    def draw(rng, idx):
        q = scenes.position[sid[idx], rng.integers(0, 3, len(idx))] + rng.uniform(-0.8, 0.8, (len(idx), 3))
        p = f32(q + off[idx])
        return p, off32[idx].copy()
    decide = lambda p, o: (sr.brute_scenes(p, scenes, sid, rad, margin, o)["raw"], margin)
    pos, _, frac = sr.settle(np.random.default_rng(52), draw, n, decide)
    assert frac <= 0.01
    env = CtrlAviary(types, n, initial_xyzs=pos.astype(np.float64), type_ids=tid, storage="auto", obstacle_watch=scenes,
                     obstacle_margin=margin, obstacle_offsets=off, obstacle_scene_id=sid, dict_io=False, noise_seed=0)
    assert env.order is not None and not np.array_equal(env.order.drone_np, np.arange(n))
    positions = lambda: env.state.pos.T.cpu().numpy().astype(np.float32)
    assert np.array_equal(positions(), pos)
    ref = sr.brute_scenes(pos, scenes, sid, rad, margin, off32)
    assert ref["contacts"] >= 3 and (ref["near"] >= 0).sum() > n // 3 and len(set(ref["near"][ref["near"] >= 0])) == 3
    clr, near = env.obstacle_clearance()
    check(clr, near, ref, margin, "env, type-major storage")
    assert int(env._obst_on_demand.item()) == ref["contacts"] and env.obstacle_contacts() == 0
    # negative control: ids left in the caller's order would hand storage slot j the id of drone j, so drone d the id of drone
    # slot[d]; against that permuted copy the comparison fails
    wrong = sr.brute_scenes(pos, scenes, sid[env.order.slot_np], rad, margin, off32)
    assert (sid[env.order.slot_np] != sid).sum() > n // 2
    with pytest.raises(AssertionError):
        check(clr, near, wrong, margin, "env, ids in the caller's order (must fail)")
    tg = Targets(env.ctx, n)
    tg.set(pos=pos.T, yaw=0.0)
    for _ in range(10):
        env.step_fused(tg)
    ref = sr.brute_scenes(positions(), scenes, sid, rad, margin, off32)
    got, got_near = (x.cpu().numpy() for x in env.last_obstacle_clearance)
    print(f"env after 10 steps: max |got - ref| = {np.abs(got - ref['clr']).max():.3e} m")
    np.testing.assert_allclose(got, ref["clr"], rtol=0, atol=ATOL)
    sure = (np.abs(ref["raw"] - margin) >= ATOL) & ~((ref["near"] >= 0) & (ref["gap"] < ATOL))
    np.testing.assert_array_equal(got_near[sure], ref["near"][sure])
    # the flown-state rule of test_gpu_obstacles.py: the last launch's count is the device's own, and differs from the brute-force
    # count by at most the drones within ATOL of 0; the counter holds ten launches
    band = np.abs(ref["raw"]) < ATOL
    np.testing.assert_array_equal((got < 0)[~band], (ref["raw"] < 0)[~band])
    assert abs(int((got < 0).sum()) - ref["contacts"]) <= int(band.sum())
    total = env.obstacle_contacts()
    assert total >= int((got < 0).sum()) and total == env.ctx.query(nat.QUERY_OBSTACLE_CONTACTS) - int(env._obst_on_demand.item())
    env.close()


# ---- 6. capture -------------------------------------------------------------------------------------------------------------------
def test_env_eager_vs_captured_replay(gpu):
    nat, _ = gpu
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.fleet import Targets
    n, K, margin = 256, 8, 0.5
    _, _, rad, scenes, sid, off = _env_world(n, K, 61)
    rng = np.random.default_rng(62)
    xyz = scenes.position[sid, rng.integers(0, 3, n)] + rng.uniform(-0.6, 0.6, (n, 3)) + off
    envs, tgts = [], []
    for _ in range(2):
        e = CtrlAviary(["robobee"], n, initial_xyzs=xyz, obstacle_watch=scenes, obstacle_margin=margin, obstacle_offsets=off,
                       obstacle_scene_id=sid, dict_io=False, noise_seed=0)
        tg = Targets(e.ctx, n)
        tg.set(pos=f32(xyz).T, yaw=0.0)
        envs.append(e)
        tgts.append(tg)
    for _ in range(4):
        envs[0].step_fused(tgts[0])
    g = envs[1].capture_fused(tgts[1], 4)
    g.replay()
    torch.cuda.synchronize()
    assert envs[0]._env_steps == envs[1]._env_steps == 4
    assert torch.equal(envs[0].state.fields(0, 13), envs[1].state.fields(0, 13))
    a, b = envs[0].obstacle_contacts(), envs[1].obstacle_contacts()
    assert a == b > 4 * (n // 8), (a, b)                         # (74 of the 256 start in contact and hover)
    (c0, n0), (c1, n1) = envs[0].last_obstacle_clearance, envs[1].last_obstacle_clearance
    assert torch.equal(c0, c1) and torch.equal(n0, n1) and int((n1 >= 0).sum()) > n // 4
    rad = np.full(n, np.float32(envs[1].ctx.types[0].collision_sphere))
    ref = sr.brute_scenes(envs[1].state.pos.T.cpu().numpy().astype(np.float32), scenes, sid, rad, margin, f32(off))
    np.testing.assert_allclose(c1.cpu().numpy(), ref["clr"], rtol=0, atol=ATOL)
    for e in envs:
        e.close()
