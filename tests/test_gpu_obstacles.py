"""GPU tests of the static-obstacle watch (dsim_obstacle_clearance, ObstacleSet, env.obstacle_clearance / obstacle_watch) against
a brute-force fp64 point-triangle computation on the fp32 positions, offsets and vertices the device holds.

Input rule: |q| <= 16 m in the set's frame, |offset| <= 128 m; drones are re-drawn until none has |c_i| < 1e-4 m or
|c_i - margin| < 1e-4 m, and at most 1 % of the drones may be re-drawn (asserted on the reference alone).  Counts and the
-1 / not -1 status of `nearest` are then compared EXACTLY, clearances with atol 1e-5 m, and a `nearest` body may differ only
where the minima of two bodies are within 1e-5 m (at most 1 % of the drones, asserted on the reference alone).

An fp32 numpy run of the kernel's algorithm (same records, same region walk) differs from the fp64 reference by at most 1.5e-7 m on
20 000 points around the gate, 1.3e-7 m on the soup and 2.4e-7 m on the single triangle; every case prints the device's own worst
difference before it asserts.

A flown state cannot be re-drawn.  There the per-drone contact decision is compared exactly on every drone whose reference
clearance is not within ATOL of 0, the counter must equal the device's own count of negative clearances exactly, and so the counter
may differ from the brute-force count by at most the number of drones with |c_i| < ATOL: a device clearance that is within ATOL of
the reference (asserted) can fall on the other side of 0 nowhere else."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from dronesim_amd import params
from tests.obstacle_ref import brute, region
from tests.util import f32, random_fleet

pytestmark = pytest.mark.gpu

GUARD, ATOL = 1e-4, 1e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product has no CPU fallback")
    from dronesim_amd import _native as nat
    from dronesim_amd import fleet
    return nat, fleet


def settle(rng, draw, n, decide):
    """The input rule: draws n drones with draw(rng, k) -> (pos, offset or None), re-draws those whose raw clearance
    decide(pos, off) sits within GUARD of 0 or of the margin; returns (pos, off, fraction re-drawn)."""
    pos, off = draw(rng, n)
    redrawn = np.zeros(n, dtype=bool)
    for _ in range(50):
        c, margin = decide(pos, off)
        bad = (np.abs(c) < GUARD) | (np.abs(c - margin) < GUARD)
        if not bad.any():
            return pos, off, redrawn.mean()
        redrawn |= bad
        p2, o2 = draw(rng, int(bad.sum()))
        pos[bad] = p2
        if off is not None:
            off[bad] = o2
    raise AssertionError("the input rule did not settle")


def check(got_clr, got_near, ref, margin, what=""):
    clr, near, gap, _, _ = ref
    got_clr, got_near = got_clr.cpu().numpy().astype(np.float64), got_near.cpu().numpy().astype(np.int64)
    err = np.abs(got_clr - clr).max()
    print(f"obstacle clearance {what}: max |got - ref| = {err:.3e} m over {clr.size} drones, {int((near >= 0).sum())} in reach, "
          f"{int((clr < 0).sum())} in contact, min {clr.min():.4f}")
    np.testing.assert_array_equal(got_near >= 0, near >= 0)
    np.testing.assert_allclose(got_clr, clr, rtol=0, atol=ATOL)
    assert np.all(got_clr[near < 0] == np.float32(margin))
    tie = (near >= 0) & (gap < ATOL)
    assert tie.mean() <= 0.01, tie.mean()
    np.testing.assert_array_equal(got_near[~tie], near[~tie])
    return err


def load(fleet, ctx, pos32, layout="soa"):
    n = pos32.shape[0]
    st = fleet.FleetState(ctx, n, layout)
    rigid, mem, _ = random_fleet(np.random.default_rng(5), n, n_act=ctx.n_act)
    rigid[:, 0:3] = pos32
    st.load_aos(rigid, mem)
    assert np.array_equal(st.rigid_aos()[:, 0:3].astype(np.float32), pos32.astype(np.float32))
    return st


def soa3(a, n_pad, dev):
    t = torch.zeros((3, n_pad), dtype=torch.float32)
    t[:, : a.shape[0]] = torch.from_numpy(np.ascontiguousarray(a.T)).float()
    return t.to(dev)


def run(ctx, st, dev_set, margin, off=None, tid=None, counter=None, fill=None):
    from dronesim_amd import obstacles as obs
    clr = torch.full((st.n_pad,), -7.0 if fill is None else fill, dtype=torch.float32, device=ctx.device)
    near = torch.full((st.n_pad,), -7, dtype=torch.int32, device=ctx.device)
    obs.query(ctx, st, dev_set, margin, clr, near, off, tid, counter)
    return clr[: st.n], near[: st.n]


def with_offsets(rng, q):
    """p32 = fl(q + off32), |off| <= 128 m, such that |p32 - off32| stays the intended point to fp32 rounding."""
    off = f32(rng.uniform(-128.0, 128.0, q.shape))
    return f32(q + off.astype(np.float64)), off


@functools.lru_cache(maxsize=None)
def gate():
    from dronesim_amd.obstacles import ObstacleSet
    return ObstacleSet.from_urdf(os.path.join(GOLDEN, "gate_50_curved.urdf"), (0, 0, 0), (0, 0, 0))


@functools.lru_cache(maxsize=None)
def soup():
    """3 000 random triangles (edges up to ~1.5 m) in a 20 m box, four bodies."""
    from dronesim_amd.obstacles import ObstacleSet
    rng = np.random.default_rng(2024)
    ctr = rng.uniform(-9.2, 9.2, (3000, 1, 3))
    tri = ctr + rng.uniform(-0.75, 0.75, (3000, 3, 3))
    return ObstacleSet(tri, np.arange(3000) // 750)


# ---- 1. one triangle: every region, both sides -----------------------------------------------------------------------------------
def test_one_triangle_every_region(gpu):
    nat, fleet = gpu
    from dronesim_amd.obstacles import ObstacleSet, watch_reach
    t = params.builtin_type("robobee")
    R, margin, n = np.float32(t.collision_sphere), 0.5, 700
    tri = np.array([[[0.0, 0.0, 1.0], [2.0, 0.0, 1.0], [0.5, 1.5, 1.3]]])
    s = ObstacleSet(tri, 0)
    rad = np.full(n, R)

    def draw(rng, k):
        return f32(rng.uniform([-0.5, -0.5, 0.6], [2.5, 2.0, 1.8], (k, 3))), None
    decide = lambda p, o: (brute(p, s.triangles, s.body, rad, margin, o)[4], margin)
    pos, _, frac = settle(np.random.default_rng(3), draw, n, decide)
    assert frac <= 0.01
    reg, side = region(pos.astype(np.float64), s.triangles[0])
    ref = brute(pos, s.triangles, s.body, rad, margin)
    for k in range(7):                                            # every region, on both sides of the plane, within reach
        for sg in (-1.0, 1.0):
            assert ((reg == k) & (side == sg) & (ref[1] >= 0)).sum() >= 3, (k, sg)
    assert ref[3] > 20
    ctx = fleet.Context([t])
    dev = s.to_device(ctx, watch_reach(ctx.types, margin))
    st = load(fleet, ctx, pos)
    cnt = torch.zeros((1,), dtype=torch.int64, device=ctx.device)
    clr, near = run(ctx, st, dev, margin, counter=cnt)
    check(clr, near, ref, margin, "one triangle")
    assert int(cnt.item()) == ref[3] == ctx.query(nat.QUERY_OBSTACLE_CONTACTS)
    dev.close()
    ctx.close()


# ---- 2. the gate -----------------------------------------------------------------------------------------------------------------
def _gate_world(n, margin, types, tid, offsets, seed):
    s = gate()
    rad = np.array([np.float32(t.collision_sphere) for t in types])[tid]

    def draw(rng, k):
        q = rng.uniform([-0.55, -1.05, -0.9], [0.55, 1.05, 0.9], (k, 3))
        return with_offsets(rng, q) if offsets else (f32(q), None)
    # (re-drawn drones keep their slot's radius: settle() passes the full arrays back in)
    decide = lambda p, o: (brute(p, s.triangles, s.body, rad, margin, o)[4], margin)
    pos, off, frac = settle(np.random.default_rng(seed), draw, n, decide)
    assert frac <= 0.01, frac
    return s, rad, pos, off


@pytest.mark.parametrize("layout", ["soa", "tile64"])
@pytest.mark.parametrize("offsets", [False, True])
def test_gate_vs_bruteforce(gpu, layout, offsets):
    nat, fleet = gpu
    from dronesim_amd.obstacles import watch_reach
    t = params.builtin_type("robobee")
    n, margin = 700, 1.0
    s, rad, pos, off = _gate_world(n, margin, [t], np.zeros(n, dtype=int), offsets, 11)
    ref = brute(pos, s.triangles, s.body, rad, margin, off)
    assert 0.08 * n < ref[3] < 0.25 * n, ref[3]                   # roughly one in seven in contact
    ctx = fleet.Context([t])
    dev = s.to_device(ctx, watch_reach(ctx.types, margin))
    st = load(fleet, ctx, pos, layout)
    cnt = torch.zeros((1,), dtype=torch.int64, device=ctx.device)
    clr, near = run(ctx, st, dev, margin, soa3(off, st.n_pad, ctx.device) if offsets else None, None, cnt)
    check(clr, near, ref, margin, f"gate {layout} offsets={offsets}")
    assert int(cnt.item()) == ref[3] == ctx.query(nat.QUERY_OBSTACLE_CONTACTS)
    clr2, near2 = run(ctx, st, dev, margin, soa3(off, st.n_pad, ctx.device) if offsets else None, None, cnt)
    assert torch.equal(clr, clr2) and torch.equal(near, near2)   # again: the same outputs, the counters double
    assert int(cnt.item()) == 2 * ref[3] == ctx.query(nat.QUERY_OBSTACLE_CONTACTS)
    dev.close()
    ctx.close()


def _mixed_types():
    types = [params.builtin_type(k) for k in ("robobee", "tello", "hexa_6DOF")]
    ghost = params.builtin_type("tello")
    ghost.name, ghost.collision_sphere = "ghost", 0.0
    return types + [ghost]


def test_gate_mixed_fleet_with_an_invisible_type(gpu):
    nat, fleet = gpu
    from dronesim_amd.obstacles import watch_reach
    types = _mixed_types()
    n, margin = 700, 0.75
    tid = (np.arange(n) % 4).astype(np.uint8)
    s, rad, pos, off = _gate_world(n, margin, types, tid, True, 13)
    ref = brute(pos, s.triangles, s.body, rad, margin, off)
    assert ref[3] > 40 and (rad == 0).sum() == n // 4
    ctx = fleet.Context(types)
    dev = s.to_device(ctx, watch_reach(ctx.types, margin))
    st = load(fleet, ctx, pos)
    t_id = torch.zeros((st.n_pad,), dtype=torch.uint8, device=ctx.device)
    t_id[:n] = torch.from_numpy(tid).to(ctx.device)
    clr, near = run(ctx, st, dev, margin, soa3(off, st.n_pad, ctx.device), t_id)
    check(clr, near, ref, margin, "gate, mixed fleet")
    c_, n_ = clr.cpu().numpy(), near.cpu().numpy()
    assert np.all(c_[rad == 0] == np.float32(margin)) and np.all(n_[rad == 0] == -1)
    assert ctx.query(nat.QUERY_OBSTACLE_CONTACTS) == ref[3]
    # more than one type and no type_id: refused
    out = torch.zeros((st.n_pad,), dtype=torch.float32, device=ctx.device)
    assert ctx.lib.dsim_obstacle_clearance(ctx.handle, ctx.stream_ptr(), n, st.view(), dev.handle, None, None, margin,
                                           out.data_ptr(), None, None) == -1
    dev.close()
    ctx.close()


# ---- 3. the soup: lists across cell borders, records through L2, whole waves outside the grown box -------------------------------
def test_soup_four_bodies_half_the_fleet_outside(gpu):
    nat, fleet = gpu
    from dronesim_amd.obstacles import watch_reach
    s = soup()
    t = params.builtin_type("hexa_6DOF")
    n, margin = 2048, 0.6
    rad = np.full(n, np.float32(t.collision_sphere))
    reach = watch_reach([t], margin)
    g, _, _ = s.grid(reach)
    lo, hi = np.array(list(g.lo), dtype=np.float64), np.array(list(g.hi), dtype=np.float64)
    assert np.abs(lo).max() < 16.0 and np.abs(hi).max() < 16.0 and s.n_tri == 3000 and s.n_bodies == 4

    def draw_in(rng, k):
        return f32(rng.uniform(-10.0, 10.0, (k, 3))), None

    def draw_out(rng, k):                                          # |q| <= 16 m, outside the grown box along at least one axis
        q = rng.uniform(-16.0, 16.0, (4 * k + 64, 3))
        q = q[((q < lo - 1e-3) | (q > hi + 1e-3)).any(1)][:k]
        assert len(q) == k
        return f32(q), None
    decide = lambda p, o: (brute(p, s.triangles, s.body, rad[: len(p)], margin, o)[4], margin)   # (the inside half only)
    rng = np.random.default_rng(29)
    p_in, _, frac = settle(rng, draw_in, n // 2, decide)
    assert frac <= 0.01, frac
    p_out, _ = draw_out(rng, n // 2)
    pos = np.concatenate([p_in, p_out])                            # drones 1024 .. 2047: sixteen whole waves outside the box
    ref = brute(pos, s.triangles, s.body, rad, margin)
    assert ref[3] > 10 and (ref[1][: n // 2] >= 0).sum() > 100 and np.all(ref[1][n // 2:] == -1)
    assert len(set(ref[1][ref[1] >= 0])) == 4
    ctx = fleet.Context([t])
    dev = s.to_device(ctx, reach)
    for layout in ("soa", "tile64"):
        st = load(fleet, ctx, pos, layout)
        before = ctx.query(nat.QUERY_OBSTACLE_CONTACTS)
        clr, near = run(ctx, st, dev, margin)
        check(clr, near, ref, margin, f"soup {layout}")
        assert ctx.query(nat.QUERY_OBSTACLE_CONTACTS) - before == ref[3]
        assert bool((clr[n // 2:] == np.float32(margin)).all()) and bool((near[n // 2:] == -1).all())
    dev.close()
    ctx.close()


# ---- 3b. more tiles than workgroups: the second trip of the tile loop -------------------------------------------------------------
# 2 050 tiles on the launchers' 2 048 workgroups: workgroup 0 walks tiles 0 and 2 048, workgroup 1 tiles 1 and 2 049 (37 live lanes).
# Every drone stands far from the set but three groups about it: tile 1, tile 2 048 and tile 2 049.  So workgroup 0 stages the records
# at its second tile, behind a tile with nobody in the box, and workgroup 1 stages at its first and re-uses them at a ragged second.
MT_N = 2049 * 256 + 37
MT_NEAR = np.concatenate([np.arange(256, 512), np.arange(524288, 524544), np.arange(524544, MT_N)])
MT_FAR = np.setdiff1d(np.arange(MT_N), MT_NEAR)


def many_tiles_far(rng, n=MT_N):
    """Positions about (60, 0, 1) m in the set's frame, a metre of jitter."""
    return f32(np.array([60.0, 0.0, 1.0]) + rng.uniform(-1.0, 1.0, (n, 3)))


def box_distance(p, lo, hi):
    """Distance from every point to the box [lo, hi], fp64."""
    p = np.asarray(p, dtype=np.float64)
    return np.linalg.norm(np.maximum(np.maximum(lo - p, p - hi), 0.0), axis=1)


def check_many_tiles(clr, near, ref, margin, check_fn, what):
    """The near drones against their reference with the file's bars, every other drone exactly (float32(margin), -1)."""
    ix = torch.from_numpy(MT_NEAR).to(clr.device)
    check_fn(clr[ix], near[ix], ref, margin, what)
    c_, n_ = clr[:MT_N].cpu().numpy(), near[:MT_N].cpu().numpy()
    assert np.all(c_[MT_FAR] == np.float32(margin)) and np.all(n_[MT_FAR] == -1)


@pytest.mark.parametrize("world", ["gate", "soup"])
def test_many_tiles_per_workgroup(gpu, world):
    nat, fleet = gpu
    from dronesim_amd.obstacles import watch_reach
    k = len(MT_NEAR)
    assert k == 549 and (MT_N + 255) // 256 == 2050
    if world == "gate":                                           # 108 triangles: the records in LDS
        t, margin = params.builtin_type("robobee"), 1.0
        s, rad, p_near, _ = _gate_world(k, margin, [t], np.zeros(k, dtype=int), False, 71)
    else:                                                         # 3 000 triangles: the records through L2
        t, margin, s = params.builtin_type("hexa_6DOF"), 0.6, soup()
        rad = np.full(k, np.float32(t.collision_sphere))
        decide = lambda p, o: (brute(p, s.triangles, s.body, rad[: len(p)], margin, o)[4], margin)
        p_near, _, frac = settle(np.random.default_rng(73), lambda rng, m: (f32(rng.uniform(-10.0, 10.0, (m, 3))), None), k, decide)
        assert frac <= 0.01, frac
    assert (s.n_tri <= 512) == (world == "gate")
    ref = brute(p_near, s.triangles, s.body, rad, margin)
    pos = many_tiles_far(np.random.default_rng(72))
    pos[MT_NEAR] = p_near
    ctx = fleet.Context([t])
    dev = s.to_device(ctx, watch_reach(ctx.types, margin))
    tri = s.triangles.reshape(-1, 3).astype(np.float64)
    assert box_distance(pos[MT_FAR], tri.min(0), tri.max(0)).min() > dev.reach
    for lo_, hi_ in ((256, 512), (524288, 524544), (524544, MT_N)):      # each of the three tiles has drones in reach
        assert (ref[1][(MT_NEAR >= lo_) & (MT_NEAR < hi_)] >= 0).any(), (lo_, hi_)
    assert ref[3] > 0
    st = load(fleet, ctx, pos)
    cnt = torch.zeros((1,), dtype=torch.int64, device=ctx.device)
    before = ctx.query(nat.QUERY_OBSTACLE_CONTACTS)
    clr, near = run(ctx, st, dev, margin, counter=cnt)
    check_many_tiles(clr, near, ref, margin, check, f"many tiles, {world}")
    assert int(cnt.item()) == ref[3] == ctx.query(nat.QUERY_OBSTACLE_CONTACTS) - before
    dev.close()
    ctx.close()


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(gpu):
    nat, fleet = gpu
    from dronesim_amd.obstacles import ObstacleSet, watch_reach
    t = params.builtin_type("robobee")
    ctx = fleet.Context([t])
    s = gate()
    margin = 0.5
    dev = s.to_device(ctx, watch_reach(ctx.types, margin))
    st = load(fleet, ctx, f32(np.zeros((64, 3))))
    clr = torch.full((st.n_pad,), -7.0, dtype=torch.float32, device=ctx.device)
    near = torch.full((st.n_pad,), -7, dtype=torch.int32, device=ctx.device)
    cnt = torch.zeros((1,), dtype=torch.int64, device=ctx.device)
    call = lambda h, m: ctx.lib.dsim_obstacle_clearance(ctx.handle, ctx.stream_ptr(), st.n, st.view(), h, None, None, m,
                                                        clr.data_ptr(), near.data_ptr(), cnt.data_ptr())
    assert call(dev.handle, 0.0) == -1 and call(dev.handle, -1.0) == -1 and call(dev.handle, float("nan")) == -1
    assert call(dev.handle, margin * 1.01) == -1                  # R_max + margin > reach of the set
    assert call(None, margin) == -1
    torch.cuda.synchronize()
    assert bool((clr == -7.0).all()) and bool((near == -7).all()) and int(cnt.item()) == 0
    assert ctx.query(nat.QUERY_OBSTACLE_CONTACTS) == 0
    assert call(dev.handle, margin) == 0 and call(dev.handle, 0.25) == 0      # (a smaller margin is served by the same set)
    # the device set refuses what the host plan refuses
    h = ctypes.c_void_p()
    tri = np.ascontiguousarray(s.triangles.reshape(-1, 9))
    assert ctx.lib.dsim_obstacles_create(ctx.handle, tri.ctypes.data, None, s.n_tri, 0.0, ctypes.byref(h)) == -1 and not h
    flat = tri.copy()
    flat[5, 6:9] = flat[5, 3:6]
    assert ctx.lib.dsim_obstacles_create(ctx.handle, flat.ctypes.data, None, s.n_tri, 1.0, ctypes.byref(h)) == -1 and not h
    with pytest.raises(ValueError):
        ObstacleSet(flat.reshape(-1, 3, 3), 0)
    dev.close()
    ctx.close()


# ---- 5 / 6. env wiring -------------------------------------------------------------------------------------------------------------
def _gate_fleet(n, seed=41, z0=3.0):
    """n drones hovering about gates of their own: the gate at (0, 0, z0) of each drone's frame, the frames on a 1 m grid."""
    from dronesim_amd.obstacles import ObstacleSet
    s = ObstacleSet.from_urdf(os.path.join(GOLDEN, "gate_50_curved.urdf"), (0.0, 0.0, z0), (0, 0, 0))
    rng = np.random.default_rng(seed)
    q = rng.uniform([-0.55, -1.05, z0 - 0.9], [0.55, 1.05, z0 + 0.9], (n, 3))
    side = int(np.ceil(np.sqrt(n)))
    off = np.stack([np.arange(n) % side, np.arange(n) // side, np.zeros(n)], 1).astype(np.float64)
    return s, q + off, off


def _positions(env):
    """fp32 positions in the caller's numbering, as the device holds them."""
    return env.state.pos.T.cpu().numpy().astype(np.float32)


def flown_contacts(env, before, ref):
    """After a step on a state that cannot be re-drawn: the counter's increment equals the device's own count of negative
    clearances, and the device decides contact as the reference does wherever |c_i| >= ATOL; -> (increment, drones inside
    that band)."""
    got = env.last_obstacle_clearance[0].cpu().numpy().astype(np.float64)
    inc = env.obstacle_contacts() - before
    assert inc == int((got < 0).sum())
    band = np.abs(ref[4]) < ATOL
    np.testing.assert_array_equal((got < 0)[~band], (ref[4] < 0)[~band])
    assert abs(inc - ref[3]) <= int(band.sum())
    return inc, int(band.sum())


def test_counters_over_six_env_steps(gpu):
    nat, _ = gpu
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.fleet import Targets
    n, margin = 512, 1.0
    s, xyz, off = _gate_fleet(n)
    env = CtrlAviary(["robobee"], n, initial_xyzs=xyz, obstacle_watch=s, obstacle_margin=margin, obstacle_offsets=off,
                     dict_io=False, noise_seed=0)
    assert env.obstacle_contacts() == 0 and env.last_obstacle_clearance is None
    rad = np.full(n, np.float32(env.ctx.types[0].collision_sphere))
    tg = Targets(env.ctx, n)
    tg.set(pos=f32(xyz).T, yaw=0.0)
    zero = torch.zeros((n, 4), dtype=torch.float32, device=env.ctx.device)
    total = 0
    for k in range(6):
        if k < 2:
            env.step(zero)
        else:
            env.step_fused(tg)
        ref = brute(_positions(env), s.triangles, s.body, rad, margin, f32(off))
        total += ref[3]
        assert ref[3] > n // 20
        clr, near = env.last_obstacle_clearance
        np.testing.assert_allclose(clr.cpu().numpy(), ref[0], rtol=0, atol=ATOL)
        c2, n2 = env.obstacle_clearance()                        # on demand: the same answer, not an Env.step
        assert torch.equal(c2, clr) and torch.equal(n2, near)
        assert env.obstacle_contacts() == total
    assert int(env._obst_on_demand.item()) == total               # contacts_out of the on-demand calls
    assert env.ctx.query(nat.QUERY_OBSTACLE_CONTACTS) == 2 * total
    env.close()
    # without the keyword nothing is launched or counted, and offsets alone are refused
    plain = CtrlAviary(["robobee"], n, initial_xyzs=xyz, dict_io=False, noise_seed=0)
    plain.step(zero)
    assert plain.obstacle_contacts() == 0 and plain.last_obstacle_clearance is None
    with pytest.raises(ValueError):
        plain.obstacle_clearance()
    plain.close()
    with pytest.raises(ValueError):
        CtrlAviary(["robobee"], n, initial_xyzs=xyz, obstacle_offsets=off, dict_io=False, noise_seed=0)
    with pytest.raises(NotImplementedError):
        CtrlAviary(["robobee"], n, initial_xyzs=xyz, obstacles=True)      # (the `obstacles` flag raises as before)


def test_env_eager_vs_captured_replay(gpu):
    nat, _ = gpu
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.fleet import Targets
    n, margin = 512, 1.0
    s, xyz, off = _gate_fleet(n, seed=43)
    envs, tgts = [], []
    for _ in range(2):
        e = CtrlAviary(["robobee"], n, initial_xyzs=xyz, obstacle_watch=s, obstacle_margin=margin, obstacle_offsets=off,
                       dict_io=False, noise_seed=0)
        tg = Targets(e.ctx, n)
        tg.set(pos=f32(xyz).T, yaw=0.0)
        envs.append(e)
        tgts.append(tg)
    for _ in range(8):
        envs[0].step_fused(tgts[0])
    g = envs[1].capture_fused(tgts[1], 4)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert envs[0]._env_steps == envs[1]._env_steps == 8
    assert torch.equal(envs[0].state.fields(0, 13), envs[1].state.fields(0, 13))
    a, b = envs[0].obstacle_contacts(), envs[1].obstacle_contacts()
    assert a == b > 8 * (n // 20), (a, b)
    (c0, n0), (c1, n1) = envs[0].last_obstacle_clearance, envs[1].last_obstacle_clearance
    assert torch.equal(c0, c1) and torch.equal(n0, n1)
    rad = np.full(n, np.float32(envs[1].ctx.types[0].collision_sphere))
    ref = brute(_positions(envs[1]), s.triangles, s.body, rad, margin, f32(off))
    np.testing.assert_allclose(c1.cpu().numpy(), ref[0], rtol=0, atol=ATOL)
    for e in envs:
        e.close()


def test_env_type_major_storage_answers_in_caller_numbering(gpu):
    nat, _ = gpu
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.fleet import Targets
    n, margin = 512, 0.75
    types = _mixed_types()
    tid = (np.arange(n) % 4).astype(np.uint8)
    rad = np.array([np.float32(t.collision_sphere) for t in types])[tid]
    s, xyz, off = _gate_fleet(n, seed=47)
    off32 = f32(off)

    def decide(p, o):
        return brute(p, s.triangles, s.body, rad, margin, o)[4], margin
    # the input rule on the fp32 positions the device will hold: a drone near a decision gets another point about ITS gate
    rng, pos, redrawn = np.random.default_rng(48), f32(xyz), np.zeros(n, dtype=bool)
    for _ in range(50):
        c_raw, _ = decide(pos, off32)
        bad = (np.abs(c_raw) < GUARD) | (np.abs(c_raw - margin) < GUARD)
        if not bad.any():
            break
        redrawn |= bad
        pos[bad] = f32(rng.uniform([-0.55, -1.05, 2.1], [0.55, 1.05, 3.9], (int(bad.sum()), 3)) + off[bad])
    assert not bad.any() and redrawn.mean() <= 0.01
    env = CtrlAviary(types, n, initial_xyzs=pos.astype(np.float64), type_ids=tid, storage="auto", obstacle_watch=s,
                     obstacle_margin=margin, obstacle_offsets=off, dict_io=False, noise_seed=0)
    assert env.order is not None
    assert np.array_equal(_positions(env), pos)
    ref = brute(pos, s.triangles, s.body, rad, margin, off32)
    clr, near = env.obstacle_clearance()
    check(clr, near, ref, margin, "gate, type-major storage")           # (exact -1 status and nearest, in the caller's numbering)
    c_, n_ = clr.cpu().numpy().astype(np.float64), near.cpu().numpy()
    assert np.all(c_[rad == 0] == np.float32(margin)) and np.all(n_[rad == 0] == -1) and ref[3] > 10
    assert len(set(np.round(c_[(rad > 0) & (n_ >= 0)], 6))) > n // 4        # (per-drone values, not a permuted constant)
    assert int(env._obst_on_demand.item()) == ref[3] and env.obstacle_contacts() == 0
    tg = Targets(env.ctx, n)
    tg.set(pos=pos.T, yaw=0.0)
    env.step_fused(tg)
    ref = brute(_positions(env), s.triangles, s.body, rad, margin, off32)
    np.testing.assert_allclose(env.last_obstacle_clearance[0].cpu().numpy(), ref[0], rtol=0, atol=ATOL)
    inc, band = flown_contacts(env, 0, ref)
    print(f"type-major env after one step: {inc} contacts (brute force {ref[3]}), {band} drones with |c| < {ATOL}")
    env.close()


# ---- 7. a short config-3 flight: replicas of the trajectory through gates of their own -------------------------------------------
def test_config3_flight_watch_equals_bruteforce_every_step(gpu):
    """Whether the flight clears its gate is a finding, not an assertion: the test prints the minimum clearance of the flight."""
    nat, _ = gpu
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.fleet import WaypointTargets
    from dronesim_amd.obstacles import ObstacleSet
    g = np.load(os.path.join(GOLDEN, "traj_track_waypoints.npz"))
    n, margin, steps = 256, 1.0, 60
    mid_gate = g["gates"][1]
    s = ObstacleSet.from_urdf(os.path.join(GOLDEN, "gate_50_curved.urdf"), mid_gate, (0, 0, 0))
    off = np.stack([np.arange(n) % 16, np.arange(n) // 16, np.zeros(n)], 1).astype(np.float64)
    n_wp = g["target_pos"].shape[0]
    # every replica starts ON the trajectory at a phase of its own; the phases bracket the passage through the gate
    at_gate = int(np.argmin(np.linalg.norm(g["target_pos"] - mid_gate, axis=1)))
    wp0 = (at_gate - 90 + (np.arange(n) * 120) // n) % n_wp
    env = CtrlAviary(["robobee"], n, initial_xyzs=g["target_pos"][wp0] + off, aggregate_phy_steps=2, freq=240, dict_io=False,
                     noise_seed=0, obstacle_watch=s, obstacle_margin=margin, obstacle_offsets=off)
    tgt = WaypointTargets(env.ctx, n, g["target_pos"], g["target_vel"], g["target_acc"], g["target_yaw"], wp_counters=wp0,
                          offsets=off)
    rad = np.full(n, np.float32(env.ctx.types[0].collision_sphere))
    lowest, contacts, worst, seen, band = np.inf, 0, 0.0, 0, 0
    for k in range(steps):
        env.step_fused(tgt, control_timestep=2 / 240, action=np.full((n, 4), 0.4, dtype=np.float32) if k == 0 else None)
        ref = brute(_positions(env), s.triangles, s.body, rad, margin, f32(off))
        clr = env.last_obstacle_clearance[0].cpu().numpy().astype(np.float64)
        worst = max(worst, np.abs(clr - ref[0]).max())
        np.testing.assert_allclose(clr, ref[0], rtol=0, atol=ATOL)
        assert abs(clr.min() - ref[0].min()) <= ATOL
        lowest = min(lowest, ref[0].min())
        contacts += ref[3]
        inc, b = flown_contacts(env, seen, ref)
        seen, band = seen + inc, band + b
    assert seen == env.obstacle_contacts()
    print(f"config-3 flight, {n} replicas x {steps} steps: minimum clearance {lowest:.4f} m, {seen} drone-steps in contact "
          f"(brute force {contacts}, {band} drone-steps with |c| < {ATOL}), worst |watch - fp64| {worst:.2e} m")
    assert lowest < margin                                        # the flight came within reach of its gate: the watch saw it
    assert abs(seen - contacts) <= band
    env.close()
