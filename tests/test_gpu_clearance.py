"""GPU tests of the drone-drone contact watch (dsim_clearance, Downwash.clearance, env.drone_clearance / drone_watch) against a
brute-force fp64 computation on the fp32 positions the device holds.

Input rule (tests 1, 4, 5): |x|, |y| <= 128 m; positions are re-drawn for the drones involved until no pair has
| |p_i - p_j| - R_i - R_j | < 1e-4 m and none has | c_ij - margin | < 1e-4 m.  Differences of nearby fp32 coordinates are exact
and what remains is a few ulps of a distance of about 1 m, so overlap and in-reach decisions do not depend on fp32 rounding:
counts and the -1 / not -1 status of `nearest` are compared EXACTLY, clearances with atol 1e-5 m (two orders above that
rounding, two below the smallest geometric feature, the 0.0475 m tello radius), and a `nearest` index may differ only where the
two smallest c_ij of that drone are closer than 1e-5 m (at most 1 % of the drones, asserted on the reference alone)."""
import ctypes

import numpy as np
import pytest
import torch

from dronesim_amd import params
from tests.util import f32, random_fleet

pytestmark = pytest.mark.gpu

GUARD, ATOL = 1e-4, 1e-5


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product has no CPU fallback")
    from dronesim_amd import _native as nat
    from dronesim_amd import fleet
    return nat, fleet


# ---- the reference: brute force, fp64, on the fp32 positions --------------------------------------------------------------
def brute(pos32, radius, margin, lo=0, hi=None):
    """pos32 [m, 3] float32, radius [m] -> for the receivers [lo, hi): clearance, nearest (world index, -1), second-smallest
    c_ij (inf when there is none), and the number of overlapping pairs (i, j) with i a receiver and j > i."""
    p = pos32.astype(np.float32).astype(np.float64)
    r = np.asarray(radius, dtype=np.float32).astype(np.float64)
    m = p.shape[0]
    hi = m if hi is None else hi
    clr, near, second, pairs = np.empty(hi - lo), np.empty(hi - lo, dtype=np.int64), np.empty(hi - lo), 0
    live = r > 0
    for k0 in range(lo, hi, 512):
        k1 = min(k0 + 512, hi)
        d = np.sqrt(((p[k0:k1, None, :] - p[None, :, :]) ** 2).sum(-1))
        c = d - r[k0:k1, None] - r[None, :]
        c[~live[k0:k1], :] = np.inf
        c[:, ~live] = np.inf
        c[np.arange(k1 - k0), np.arange(k0, k1)] = np.inf
        srt = np.sort(c, axis=1)[:, :2] if m > 1 else np.full((k1 - k0, 2), np.inf)
        j = c.argmin(1)
        cm = c[np.arange(k1 - k0), j]
        clr[k0 - lo:k1 - lo] = np.minimum(cm, margin)
        near[k0 - lo:k1 - lo] = np.where(cm < margin, j, -1)
        second[k0 - lo:k1 - lo] = srt[:, 1] if m > 1 else np.inf
        pairs += int(((c < 0) & (np.arange(m)[None, :] > np.arange(k0, k1)[:, None])).sum())
    return clr, near, second, pairs


def settle(rng, pos, radius, margin, redraw, fixed=()):
    """The input rule: re-draws (with `redraw(rng, idx)`) the drones of every pair that sits within GUARD of touching or of the
    margin, until none does.  Drones in `fixed` (planted ones) are never moved — their partner is."""
    fixed = np.zeros(len(pos), dtype=bool) if len(fixed) == 0 else fixed
    for _ in range(200):
        p = pos.astype(np.float32).astype(np.float64)
        r = np.asarray(radius, dtype=np.float32).astype(np.float64)
        bad = np.zeros(len(pos), dtype=bool)
        for k0 in range(0, len(pos), 512):
            k1 = min(k0 + 512, len(pos))
            c = np.sqrt(((p[k0:k1, None, :] - p[None, :, :]) ** 2).sum(-1)) - r[k0:k1, None] - r[None, :]
            c[np.arange(k1 - k0), np.arange(k0, k1)] = np.inf
            c[r[k0:k1] <= 0, :] = np.inf
            c[:, r <= 0] = np.inf
            hit = (np.abs(c) < GUARD) | (np.abs(c - margin) < GUARD)
            bad[k0:k1] |= hit.any(1)
        idx = np.flatnonzero(bad & ~fixed)
        if not bad.any():
            return pos
        assert idx.size, "a planted pair violates the input rule"
        pos[idx] = redraw(rng, idx)
    raise AssertionError("the input rule did not settle")


def check(got_clr, got_near, ref, margin):
    clr, near, second, _ = ref
    got_clr, got_near = got_clr.cpu().numpy().astype(np.float64), got_near.cpu().numpy().astype(np.int64)
    print(f"clearance: max |got - ref| = {np.abs(got_clr - clr).max():.3e} m over {clr.size} drones, "
          f"{int((near >= 0).sum())} in reach, min {clr.min():.4f}")
    np.testing.assert_array_equal(got_near >= 0, near >= 0)
    np.testing.assert_allclose(got_clr, clr, rtol=0, atol=ATOL)
    assert np.all(got_clr[near < 0] == np.float32(margin))
    tie = (near >= 0) & (second - np.minimum(clr, second) < ATOL)
    assert tie.mean() <= 0.01, tie.mean()
    np.testing.assert_array_equal(got_near[~tie], near[~tie])


def load(fleet, ctx, pos, layout="soa", type_id=None):
    n = pos.shape[0]
    st = fleet.FleetState(ctx, n, layout)
    rigid, mem, _ = random_fleet(np.random.default_rng(5), n, n_act=ctx.n_act)
    rigid[:, 0:3] = f32(pos)
    st.load_aos(rigid, mem)
    return st


def contacts(ctx, nat):
    return ctx.query(nat.QUERY_DRONE_CONTACTS)


# ---- 1. homogeneous fleet, a crowded cell, pairs across cell borders -----------------------------------------------------------
def _crowded_world(n=1000, margin=0.5):
    """1 000 robobees in a 40 x 30 x 6 m box, 298 of them inside ONE cell of the grid the call will choose, and 20 overlapping
    pairs that straddle its cell borders in x, in y and diagonally."""
    from dronesim_amd.downwash import clearance_grid
    t = params.builtin_type("robobee")
    R = float(np.float32(t.collision_sphere))
    rng = np.random.default_rng(17)
    lo = np.array([-20.0, -15.0, 0.5])

    def redraw(rng, idx):
        return lo + rng.uniform(0, 1, (len(idx), 3)) * np.array([40.0, 30.0, 6.0])
    pos = redraw(rng, np.arange(n))
    grid = clearance_grid((-20.0, -15.0), (20.0, 15.0), t.collision_sphere, margin, n)
    cell, xmin, ymin, nx, ny = grid
    fixed = np.zeros(n, dtype=bool)
    cx0, cy0 = xmin + 9 * cell, ymin + 7 * cell

    def crowd(rng, k):
        return np.array([cx0, cy0, 1.0]) + rng.uniform(0.05, 0.95, (k, 3)) * np.array([cell, cell, 4.0])
    pos[0:300] = crowd(rng, 300)
    for k in range(20):
        bx, by = xmin + (3 + k) * cell, ymin + (12 + (k % 5)) * cell
        a = 300 + 2 * k
        gap = 0.03 + 0.005 * k                                   # centre distance 2 gap (x / y) or 0.8 sqrt 2 gap: below 2 R = 0.316
        if k % 3 == 0:
            pos[a], pos[a + 1] = (bx - gap, by + 0.4 * cell, 2.0), (bx + gap, by + 0.4 * cell, 2.0)
        elif k % 3 == 1:
            pos[a], pos[a + 1] = (bx + 0.4 * cell, by - gap, 3.0), (bx + 0.4 * cell, by + gap, 3.0)
        else:
            pos[a], pos[a + 1] = (bx - 0.4 * gap, by - 0.4 * gap, 4.0), (bx + 0.4 * gap, by + 0.4 * gap, 4.0)
        fixed[a:a + 2] = True
    pos[0] = (-20.0, -15.0, 1.0)
    pos[1] = (20.0, 15.0, 1.0)                                    # (the corners pin the bounding box, hence the grid)
    fixed[0:2] = True
    rad = np.full(n, R)
    pos = settle(rng, pos, rad, margin, lambda rng, idx: np.where((idx < 300)[:, None], crowd(rng, len(idx)), redraw(rng, idx)), fixed)
    assert np.abs(pos[:, :2]).max() <= 128.0
    return t, pos, rad, grid


@pytest.mark.parametrize("layout", ["soa", "tile64"])
def test_homogeneous_fleet_vs_bruteforce(gpu, layout):
    nat, fleet = gpu
    from dronesim_amd.downwash import Downwash
    n, margin = 1000, 0.5
    t, pos, rad, (cell, xmin, ymin, nx, ny) = _crowded_world(n, margin)
    ctx = fleet.Context([t])
    st = load(fleet, ctx, pos, layout)
    p32 = st.rigid_aos()[:, 0:3].astype(np.float32)
    ref = brute(p32, rad, margin)
    assert ref[3] >= 20 and (ref[1] >= 0).sum() > 300
    dw = Downwash(ctx, st)
    pairs = torch.zeros((1,), dtype=torch.int64, device=ctx.device)
    before = contacts(ctx, nat)
    clr, near = dw.clearance(margin, pairs_out=pairs)
    assert (dw._box[2], dw._box[3]) == (nx, ny) and dw.cell == cell
    check(clr, near, ref, margin)
    assert int(pairs.item()) == ref[3] and contacts(ctx, nat) - before == ref[3]
    clr2, near2 = dw.clearance(margin, pairs_out=pairs)          # again: the outputs are the same, the counters double
    assert torch.equal(clr, clr2) and torch.equal(near, near2)
    assert int(pairs.item()) == 2 * ref[3] and contacts(ctx, nat) - before == 2 * ref[3]
    ctx.close()


# ---- 2. degenerate sizes -----------------------------------------------------------------------------------------------------
def test_degenerate_sizes(gpu):
    nat, fleet = gpu
    from dronesim_amd.downwash import Downwash
    t = params.builtin_type("robobee")
    R, margin = np.float32(t.collision_sphere), 0.75
    # n = 1
    ctx = fleet.Context([t])
    st = load(fleet, ctx, np.array([[3.0, -2.0, 1.0]]))
    clr, near = Downwash(ctx, st).clearance(margin)
    assert clr.cpu().tolist() == [np.float32(margin)] and near.cpu().tolist() == [-1] and contacts(ctx, nat) == 0
    ctx.close()
    # n = 2 at the same position
    ctx = fleet.Context([t])
    st = load(fleet, ctx, np.array([[3.0, -2.0, 1.0], [3.0, -2.0, 1.0]]))
    clr, near = Downwash(ctx, st).clearance(margin)
    np.testing.assert_allclose(clr.cpu().numpy(), [-2.0 * float(R)] * 2, rtol=0, atol=ATOL)
    assert near.cpu().tolist() == [1, 0] and contacts(ctx, nat) == 1
    ctx.close()
    # n = 65: drone 64 (the second wave) overlaps drone 0, everyone else is alone
    pos = np.stack([4.0 * np.arange(65), np.zeros(65), np.ones(65)], 1)
    pos[64] = (0.1, 0.1, 1.05)
    ctx = fleet.Context([t])
    st = load(fleet, ctx, pos)
    clr, near = Downwash(ctx, st).clearance(margin)
    ref = brute(st.rigid_aos()[:, 0:3], np.full(65, R), margin)
    check(clr, near, ref, margin)
    n_ = near.cpu().numpy()
    assert n_[0] == 64 and n_[64] == 0 and np.all(n_[1:64] == -1) and ref[3] == 1 and contacts(ctx, nat) == 1
    ctx.close()


# ---- 3. drones outside the grid's box are clamped into its border cells ----------------------------------------------------------
def test_box_over_the_middle_of_the_fleet(gpu):
    nat, fleet = gpu
    from dronesim_amd.downwash import Downwash
    t = params.builtin_type("tello")
    margin, n = 0.4, 1500
    rng = np.random.default_rng(23)
    redraw = lambda rng, idx: np.stack([rng.uniform(-12, 12, len(idx)), rng.uniform(-6, 6, len(idx)), rng.uniform(0.5, 2.0, len(idx))], 1)
    pos = settle(rng, redraw(rng, np.arange(n)), np.full(n, np.float32(t.collision_sphere)), margin, redraw)
    ctx = fleet.Context([t])
    st = load(fleet, ctx, pos)
    full = Downwash(ctx, st).clearance(margin)
    pairs_full = contacts(ctx, nat)
    ref = brute(st.rigid_aos()[:, 0:3], np.full(n, np.float32(t.collision_sphere)), margin)
    assert pairs_full == ref[3] and (ref[1] >= 0).sum() > n // 4
    box = (-4.0, -6.0, 4.0, 6.0)                                  # the middle third in x: a third of the fleet on either side of it
    outside = (np.abs(pos[:, 0]) > 4.0 + 0.5).mean()
    assert outside > 1.0 / 3.0
    dw = Downwash(ctx, st)
    part = dw.clearance(margin, box=box)
    assert dw._box[0] > -5.0 and dw._box[0] + dw._box[2] * dw.cell < 6.0
    assert torch.equal(full[0], part[0]) and torch.equal(full[1], part[1])
    assert contacts(ctx, nat) == 2 * pairs_full
    ctx.close()


# ---- 4. three radii, type-major storage behind the caller's numbering, an invisible type ------------------------------------------
def _hetero_world(n, margin, seed, invisible=False):
    names = ["robobee", "tello", "hexa_6DOF"]
    types = [params.builtin_type(k) for k in names]
    if invisible:
        ghost = params.builtin_type("tello")
        ghost.name, ghost.collision_sphere = "ghost", 0.0
        types.append(ghost)
    tid = (np.arange(n) % len(types)).astype(np.uint8)
    rad = np.array([np.float32(t.collision_sphere) for t in types])[tid]
    rng = np.random.default_rng(seed)

    def redraw(rng, idx):
        return np.stack([rng.uniform(-30, 30, len(idx)), rng.uniform(-25, 25, len(idx)), rng.uniform(0.5, 3.0, len(idx))], 1)
    pos = settle(rng, redraw(rng, np.arange(n)), rad, margin, redraw)
    return types, tid, rad, pos


@pytest.mark.parametrize("storage", ["auto", "caller"])
def test_heterogeneous_env_in_caller_numbering(gpu, storage):
    nat, _ = gpu
    from dronesim_amd.envs import CtrlAviary
    n, margin = 3001, 1.0
    types, tid, rad, pos = _hetero_world(n, margin, 31)
    env = CtrlAviary(types, n, initial_xyzs=pos, type_ids=tid, storage=storage, dict_io=False, noise_seed=0)
    assert (env.order is not None) == (storage == "auto")
    ref = brute(env.state.rigid_aos()[:, 0:3], rad, margin)
    assert ref[3] > 0 and (ref[1] >= 0).sum() > n // 3
    clr, near = env.drone_clearance(margin)
    check(clr, near, ref, margin)
    assert env.drone_contacts() == 0                              # (an on-demand query is not an Env.step)
    assert env.ctx.query(nat.QUERY_DRONE_CONTACTS) == ref[3]
    env.close()


def test_type_without_a_sphere_is_invisible(gpu):
    nat, _ = gpu
    from dronesim_amd.envs import CtrlAviary
    n, margin = 1200, 1.0
    types, tid, rad, pos = _hetero_world(n, margin, 37, invisible=True)
    assert (rad == 0).sum() == n // 4
    env = CtrlAviary(types, n, initial_xyzs=pos, type_ids=tid, dict_io=False, noise_seed=0)
    ref = brute(env.state.rigid_aos()[:, 0:3], rad, margin)
    clr, near = env.drone_clearance(margin)
    check(clr, near, ref, margin)
    c_, n_ = clr.cpu().numpy(), near.cpu().numpy()
    assert np.all(c_[rad == 0] == np.float32(margin)) and np.all(n_[rad == 0] == -1)
    assert not np.isin(n_[n_ >= 0], np.flatnonzero(rad == 0)).any()
    assert env.ctx.query(nat.QUERY_DRONE_CONTACTS) == ref[3]
    env.close()


# ---- 5. the pos_all form: a shard of a larger world ----------------------------------------------------------------------------
def _two_type_world(m, margin):
    types = [params.builtin_type(k) for k in ("robobee", "tello")]
    tid = (np.arange(m) % 2).astype(np.uint8)
    rad = np.array([np.float32(t.collision_sphere) for t in types])[tid]
    rng = np.random.default_rng(41)

    def redraw(rng, idx):
        return np.stack([rng.uniform(-100, -70, len(idx)), rng.uniform(100, 125, len(idx)), rng.uniform(0.5, 3.0, len(idx))], 1)
    return types, tid, rad, settle(rng, redraw(rng, np.arange(m)), rad, margin, redraw)


def test_world_form_shards_tile_the_pair_count(gpu):
    nat, fleet = gpu
    from dronesim_amd.downwash import Downwash
    m, margin = 2500, 0.6
    types, tid, rad, pos = _two_type_world(m, margin)
    p32 = pos.astype(np.float32)
    world_ref = brute(p32, rad, margin)
    assert world_ref[3] > 10
    wp = torch.from_numpy(np.ascontiguousarray(p32.T)).cuda()
    wr = torch.from_numpy(rad.astype(np.float32)).cuda()
    total = 0
    for lo, hi in ((0, 700), (700, 1500), (1500, 2500)):
        ctx = fleet.Context(types)
        st = load(fleet, ctx, p32[lo:hi].astype(np.float64))
        t_id = torch.zeros((st.n_pad,), dtype=torch.uint8, device=ctx.device)
        t_id[: hi - lo] = torch.from_numpy(tid[lo:hi]).to(ctx.device)
        dw = Downwash(ctx, st, t_id)
        pairs = torch.zeros((1,), dtype=torch.int64, device=ctx.device)
        clr, near = dw.clearance(margin, world_pos=wp, world_radius=wr, local_offset=lo, pairs_out=pairs)
        ref = brute(p32, rad, margin, lo, hi)
        check(clr, near, ref, margin)                               # (nearest: world indices)
        assert int(pairs.item()) == ref[3] == contacts(ctx, nat)
        total += ref[3]
        if lo == 700:
            # bad arguments, on the raw entry point: radii without world positions, and a cell below 2 R_max + margin
            a = dw._clr_args
            out = torch.zeros((st.n_pad,), dtype=torch.float32, device=ctx.device)
            call = lambda args, radius: ctx.lib.dsim_clearance(ctx.handle, ctx.stream_ptr(), st.n, st.view(), ctypes.byref(args), radius,
                                                               margin, out.data_ptr(), None, None)
            assert call(a, wr.data_ptr()) == 0
            b = nat.DownwashArgs.from_buffer_copy(a)
            b.pos_all, b.m, b.m_pad, b.local_offset = None, st.n, st.n, 0
            assert call(b, wr.data_ptr()) == -1
            assert call(a, None) == -1
            b = nat.DownwashArgs.from_buffer_copy(a)
            b.cell = float(np.float32(2.0 * max(t.collision_sphere for t in types) + margin) * np.float32(0.999))
            assert call(b, wr.data_ptr()) == -1
            hp = nat.HaloPlan()
            b = nat.DownwashArgs.from_buffer_copy(a)
            b.halo = ctypes.addressof(hp)
            assert call(b, wr.data_ptr()) == -5
        ctx.close()
    assert total == world_ref[3]


# ---- 6. env wiring -------------------------------------------------------------------------------------------------------------
def _lattice(n=320):
    k = np.arange(n)
    return np.stack([0.25 * (k % 32), 2.0 * (k // 32), np.full(n, 1.0)], 1)


def test_env_watch_counts_every_step(gpu):
    nat, _ = gpu
    from dronesim_amd.envs import CtrlAviary, VelocityAviary
    from dronesim_amd.fleet import Targets
    n, xyz = 320, _lattice()
    t = params.builtin_type("robobee")
    rad = np.full(n, np.float32(t.collision_sphere))
    envs = [CtrlAviary(["robobee"], n, initial_xyzs=xyz, drone_watch=w, dict_io=False, noise_seed=0) for w in (True, False)]
    assert envs[0].drone_contacts() == 0 and envs[0].last_clearance is None
    tgts = []
    for e in envs:
        tg = Targets(e.ctx, n)
        tg.set(pos=f32(xyz).T, yaw=0.0)
        tgts.append(tg)
    running = 0
    zero = torch.zeros((n, 4), dtype=torch.float32, device=envs[0].ctx.device)
    for k in range(15):
        for e, tg in zip(envs, tgts):
            if k < 10:
                e.step(zero)
            else:
                e.step_fused(tg)
        ref = brute(envs[0].state.rigid_aos()[:, 0:3], rad, 1.0)
        running += ref[3]
        assert ref[3] >= 10 * 31                                 # (the 0.25 m pitch: every x-neighbour overlaps)
        assert envs[0].drone_contacts() == running
        clr, near = envs[0].last_clearance
        np.testing.assert_allclose(clr.cpu().numpy(), ref[0], rtol=0, atol=ATOL)
        np.testing.assert_array_equal(near.cpu().numpy() >= 0, ref[1] >= 0)
    a, b = envs[0].state.data, envs[1].state.data
    assert torch.equal(a, b)                                      # the watch changes no result, bit for bit
    assert envs[1].ctx.query(nat.QUERY_DRONE_CONTACTS) == 0 and envs[1].drone_contacts() == 0 and envs[1].last_clearance is None
    for e in envs:
        e.close()
    # an adaptor env counts too
    v = VelocityAviary(["robobee"], n, initial_xyzs=xyz, drone_watch=True, dict_io=False, noise_seed=0)
    act = torch.zeros((n, 4), dtype=torch.float32, device=v.ctx.device)
    running = 0
    for k in range(3):
        v.step(act)
        running += brute(v.state.rigid_aos()[:, 0:3], rad, 1.0)[3]
        assert v.drone_contacts() == running > 0
    v.close()


class _TwoRanks:
    @staticmethod
    def is_initialized():
        return True

    @staticmethod
    def get_world_size():
        return 2

    @staticmethod
    def get_rank():
        return 0


def test_env_watch_refuses_what_it_does_not_serve(gpu):
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.fleet import Targets
    n, xyz = 320, _lattice()
    with pytest.raises(NotImplementedError):
        CtrlAviary(["robobee"], n, initial_xyzs=xyz, drone_watch=True, dict_io=False, noise_seed=0, dist=_TwoRanks())
    env = CtrlAviary(["robobee"], n, initial_xyzs=xyz, drone_watch=True, dict_io=False, noise_seed=0)
    tg = Targets(env.ctx, n)
    tg.set(pos=f32(xyz).T, yaw=0.0)
    with pytest.raises(NotImplementedError):
        env.capture_fused(tg, 4)
    env.close()


# ---- 7. a hovering config-5-like fleet: the watch beside the neighbour downwash -------------------------------------------------
def test_watch_leaves_the_downwash_fleet_alone(gpu):
    nat, _ = gpu
    from dronesim_amd.envs import CtrlAviary, Physics
    from dronesim_amd.fleet import Targets
    n = 2048
    k = np.arange(n)
    xyz = np.stack([5.0 * (k % 32), 5.0 * ((k // 32) % 32), 2.0 + 5.0 * (k // 1024)], 1)      # (two layers: the term acts on the lower one)
    models = ["robobee", "hexa_6DOF"]
    tid = (k % 2).astype(np.uint8)
    envs, tgts = [], []
    for w in (True, False):
        e = CtrlAviary(models, n, initial_xyzs=xyz, type_ids=tid, physics=Physics.PYB_DW, drone_watch=w, dict_io=False, noise_seed=0)
        tg = Targets(e.ctx, n)
        tg.set(pos=f32(xyz).T, yaw=0.0)
        envs.append(e)
        tgts.append(tg)
    for s_ in range(20):
        for e, tg in zip(envs, tgts):
            e.step_fused(tg)
        if s_ in (0, 7, 19):
            assert torch.equal(envs[0]._downwash.force, envs[1]._downwash.force)
            clr, near = envs[0].last_clearance
            assert bool((clr == 1.0).all()) and bool((near == -1).all())
    assert float(envs[0]._downwash.force[2].abs().max()) > 0.0
    assert torch.equal(envs[0].state.data, envs[1].state.data)
    assert envs[0].drone_contacts() == 0
    for e in envs:
        e.close()
