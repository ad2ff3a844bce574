"""GPU tests of the nearest-neighbour observation (dsim_knn, Downwash.nearest, env.nearest_neighbors / neighbor_obs) against the
brute-force fp64 reference of tests/knn_ref.py on the fp32 positions and velocities the device holds.  The input rules and the
tolerances are in tests/README_knn.md: outside the tie mask indices, order and count are compared exactly; distances, rel_pos and
rel_vel with atol 1e-5 everywhere."""
import ctypes

import numpy as np
import pytest
import torch

from dronesim_amd import params
from tests import knn_ref as kr
from tests.util import f32, random_fleet

pytestmark = pytest.mark.gpu

R = kr.RADIUS


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product has no CPU fallback")
    from dronesim_amd import _native as nat
    from dronesim_amd import fleet
    return nat, fleet


def load(fleet, ctx, pos, vel=None, layout="soa"):
    n = pos.shape[0]
    st = fleet.FleetState(ctx, n, layout)
    rigid, mem, _ = random_fleet(np.random.default_rng(5), n, n_act=ctx.n_act)
    rigid[:, 0:3] = pos.astype(np.float32).astype(np.float64)      # (not through f32(): a planted NaN stays one)
    if vel is not None:
        rigid[:, 7:10] = f32(vel)
    st.load_aos(rigid, mem)
    return st


def held(st):
    """(pos32, vel32) [n, 3] as the device holds them."""
    r = st.rigid_aos()
    return r[:, 0:3].astype(np.float32), r[:, 7:10].astype(np.float32)


def host(nb):
    return tuple(None if t is None else t.cpu().numpy() for t in nb)


@pytest.fixture(scope="module")
def standard(gpu):
    """The standard world once: its state on the device, what the device holds, and (filled by test 1) the results per k."""
    nat, fleet = gpu
    pos, vel = kr.standard_world(17)
    ctx = fleet.Context([params.builtin_type("tello")])
    world = {"ctx": ctx, "got": {}}
    for layout in ("soa", "tile64"):
        world[layout] = load(fleet, ctx, pos, vel, layout)
    world["p32"], world["v32"] = held(world["soa"])
    yield world
    ctx.close()


# ---- 1. the standard world, every instance of the kernel, every output ------------------------------------------------------------
@pytest.mark.parametrize("k,layout", [(4, "soa"), (8, "tile64"), (16, "soa")])
def test_standard_world_vs_bruteforce(gpu, standard, k, layout):
    from dronesim_amd.downwash import Downwash, Neighbors
    ctx, st = standard["ctx"], standard[layout]
    p32, v32 = standard["p32"], standard["v32"]
    ref = kr.brute(p32, R, k, vel32=v32)
    assert (ref.count > k).mean() > 0.3 and (ref.count < k).any() and (ref.count == 0).any()     # full, short and empty lists
    dw = Downwash(ctx, st)
    nb = dw.nearest(R, k)
    assert nb.index.shape == (k, st.n) and nb.rel_pos.shape == (k, 3, st.n) and nb.count.shape == (st.n,)
    got = host(nb)
    kr.compare(got, ref, k, R, p32, v32, what=f"standard {layout}")
    exact = ~ref.exempt & (ref.count > k)
    assert exact.any() and np.array_equal(got[4][exact], ref.count[exact])       # the count is exact also where count > k
    standard["got"][k] = nb
    # again, into a record at fixed addresses, without the relative outputs: the same lists, bit for bit; what is None stays None
    dev = ctx.device
    out = Neighbors(torch.full((k, st.n_pad), 7, dtype=torch.int32, device=dev), torch.zeros((k, st.n_pad), device=dev), None, None,
                    torch.zeros((st.n_pad,), dtype=torch.int32, device=dev))
    nb2 = dw.nearest(R, k, out=out)
    assert nb2.rel_pos is None and nb2.rel_vel is None and nb2.index.data_ptr() == out.index.data_ptr()
    assert torch.equal(nb2.index, nb.index) and torch.equal(nb2.dist, nb.dist) and torch.equal(nb2.count, nb.count)
    assert torch.all(out.index[:, st.n:] == 7)                                    # lanes i >= n are not written
    only = dw.nearest(R, k, rel_pos=False, rel_vel=False, count=False)
    assert only.rel_pos is None and only.rel_vel is None and only.count is None and torch.equal(only.index, nb.index)


# ---- 2. k = 1 against the contact watch -------------------------------------------------------------------------------------------
def test_k1_is_the_clearance_watch_nearest(gpu, standard):
    from dronesim_amd.downwash import Downwash
    ctx, st, p32 = standard["ctx"], standard["soa"], standard["p32"]
    rad = float(np.float32(ctx.types[0].collision_sphere))
    margin = 0.8
    radius = margin + 2.0 * rad               # equal radii: c_ij < margin is d_ij < radius, the least clearance the least distance
    clr, near = Downwash(ctx, st).clearance(margin)
    nb = Downwash(ctx, st).nearest(radius, 1)
    ref = kr.brute(p32, radius, 1)
    assert ref.exempt.mean() <= kr.EXEMPT_CAP
    near, clr, idx, dist = near.cpu().numpy(), clr.cpu().numpy(), nb.index[0].cpu().numpy(), nb.dist[0].cpu().numpy()
    seen = (near >= 0) & ~ref.exempt
    assert seen.mean() > 0.3
    np.testing.assert_array_equal(idx[seen], near[seen])
    np.testing.assert_allclose(dist[seen], clr[seen] + 2.0 * rad, rtol=0, atol=kr.ATOL)
    np.testing.assert_array_equal((idx >= 0)[~ref.exempt], (near >= 0)[~ref.exempt])


# ---- 3. the smallest shapes ---------------------------------------------------------------------------------------------------------
def _one(gpu, pos, k, radius=R, vel=None, **kw):
    nat, fleet = gpu
    from dronesim_amd.downwash import Downwash
    ctx = fleet.Context([params.builtin_type("tello")])
    st = load(fleet, ctx, np.asarray(pos, dtype=np.float64), vel)
    got = host(Downwash(ctx, st).nearest(radius, k, **kw))
    p32, v32 = held(st)
    n_pad = st.n_pad
    ctx.close()
    return got, p32, v32, n_pad


def test_one_drone_has_no_neighbour(gpu):
    (index, dist, rel_pos, rel_vel, count), *_ = _one(gpu, [[3.0, -2.0, 1.0]], 4)
    assert index.shape == (4, 1) and np.all(index == -1) and np.all(np.isposinf(dist)) and count.tolist() == [0]
    assert np.all(rel_pos == 0.0) and np.all(rel_vel == 0.0)


@pytest.mark.parametrize("factor,inside", [(0.9, True), (1.1, False)])
def test_a_pair_inside_and_outside_the_radius(gpu, factor, inside):
    pos = np.array([[1.0, 1.0, 1.0], [1.0 + factor * R, 1.0, 1.0]])
    vel = np.array([[1.0, 0.0, 0.5], [-2.0, 3.0, 0.0]])
    (index, dist, rel_pos, rel_vel, count), p32, v32, _ = _one(gpu, pos, 2, vel=vel)
    if not inside:
        assert np.all(index == -1) and np.all(np.isposinf(dist)) and count.tolist() == [0, 0] and np.all(rel_pos == 0.0)
        return
    assert index.tolist() == [[1, 0], [-1, -1]] and count.tolist() == [1, 1] and np.all(np.isposinf(dist[1]))
    d = float(p32[1, 0].astype(np.float64) - p32[0, 0].astype(np.float64))
    np.testing.assert_allclose(dist[0], [d, d], rtol=0, atol=kr.ATOL)
    np.testing.assert_allclose(rel_pos[0], [[d, -d], [0, 0], [0, 0]], rtol=0, atol=kr.ATOL)
    np.testing.assert_allclose(rel_vel[0], np.stack([v32[1] - v32[0], v32[0] - v32[1]], 1), rtol=0, atol=kr.ATOL)
    assert np.all(rel_pos[1] == 0.0) and np.all(rel_vel[1] == 0.0)


def test_a_second_ragged_workgroup(gpu):
    pos, vel = kr.ragged_world()
    got, p32, v32, n_pad = _one(gpu, pos, 8, vel=vel)
    assert pos.shape[0] == 257 and n_pad > 257
    ref = kr.brute(p32, R, 8, vel32=v32)
    assert ref.count[256] > 0
    kr.compare(got, ref, 8, R, p32, v32, what="ragged 257")


@pytest.mark.parametrize("k", [3, 4, 7, 8, 16])
def test_planted_set_leaves_out_the_farthest(gpu, k):
    """k + 1 drones at distinct distances round receiver 0, handed over far to near: slot t holds drone k + 1 - t, drone 1 (the
    farthest) is the one left out, the count says k + 1.  (k = 3 and 7 keep more than they write: the list is cut at k.)"""
    pos = kr.planted_world(k)
    got, p32, v32, _ = _one(gpu, pos, k)
    index, dist, rel_pos, rel_vel, count = got
    assert index[:, 0].tolist() == list(range(k + 1, 1, -1)) and count[0] == k + 1
    ref = kr.brute(p32, R, k, vel32=v32)
    assert ref.index[0].tolist() == index[:, 0].tolist() and not ref.exempt[0]
    np.testing.assert_allclose(dist[:, 0], ref.dist[0], rtol=0, atol=kr.ATOL)
    np.testing.assert_allclose(dist[:, 0], 0.30 + 0.05 * np.arange(k), rtol=0, atol=1e-4)    # (the hand-picked distances themselves)
    np.testing.assert_allclose(rel_pos[:, :, 0], ref.rel_pos[0], rtol=0, atol=kr.ATOL)


def test_an_exact_tie_goes_to_the_lower_index(gpu):
    pos = kr.mirror_world()
    (index, dist, rel_pos, _, count), p32, _, _ = _one(gpu, pos, 4)
    assert np.array_equal(p32.astype(np.float64), pos)                       # the mirror images are exact in fp32
    assert index[:, 0].tolist() == [3, 1, 2, -1] and count[0] == 3
    assert dist[1, 0] == dist[2, 0] and np.all(rel_pos[1, :, 0] == -rel_pos[2, :, 0])
    (index2, *_), *_ = _one(gpu, pos, 2)                                      # cut between the two: the lower index stays
    assert index2[:, 0].tolist() == [3, 1]


# ---- 4. drones outside the grid's box are clamped into its border cells -------------------------------------------------------------
@pytest.mark.parametrize("k", [4, 16])
def test_box_over_the_central_third(gpu, standard, k):
    from dronesim_amd.downwash import Downwash
    ctx, st = standard["ctx"], standard["soa"]
    full = standard["got"].get(k) or Downwash(ctx, st).nearest(R, k)
    box = (-10.0 / 3.0, -2.5, 10.0 / 3.0, 2.5)                       # the central third of the 20 x 15 m arena in x and in y
    p = standard["p32"]
    outside = ((np.abs(p[:, 0]) > 10.0 / 3.0 + R) | (np.abs(p[:, 1]) > 2.5 + R)).mean()
    assert outside > 0.3
    dw = Downwash(ctx, st)
    part = dw.nearest(R, k, box=box)
    assert dw._box[0] > -10.0 / 3.0 - 2.0 * dw.cell and dw._box[0] + dw._box[2] * dw.cell < 10.0 / 3.0 + 3.0 * dw.cell
    for a, b in zip(full, part):
        assert torch.equal(a, b)


# ---- 5. the env: a storage order in force, behind step() and step_fused() -----------------------------------------------------------
def test_env_in_the_callers_numbering(gpu):
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.fleet import Targets
    pos = kr.hetero_world()
    n, k = pos.shape[0], 8
    tid = (np.arange(n) % 2).astype(np.uint8)                         # tello, hexa, tello, ...: handed over interleaved
    vel = np.random.default_rng(3).uniform(-2.0, 2.0, (n, 3))
    env = CtrlAviary(["tello", "hexa_6DOF"], n, initial_xyzs=pos, initial_vels=vel, type_ids=tid, dict_io=False, noise_seed=0,
                     neighbor_obs=k, neighbor_radius=R)
    assert env.order is not None and env.last_neighbors is None

    def check(nb, what, k=k, radius=R):
        r = env.state.rigid_aos()                                     # (the caller's numbering)
        p32, v32 = r[:, 0:3].astype(np.float32), r[:, 7:10].astype(np.float32)
        ref = kr.brute(p32, radius, k, vel32=v32)
        assert (ref.count >= k).mean() > 0.3
        kr.compare(host(nb), ref, k, radius, p32, v32, what=what)

    check(env.nearest_neighbors(), "env on demand")
    assert env.last_neighbors is None                                 # (an on-demand query is not a step)
    check(env.nearest_neighbors(k=3, radius=1.0), "env on demand, k = 3", 3, 1.0)
    env.step(torch.zeros((n, env.n_act), dtype=torch.float32, device=env.ctx.device))
    check(env.last_neighbors, "env behind step()")
    tg = Targets(env.ctx, n)
    tg.set(pos=f32(pos).T, yaw=0.0)
    env.step_fused(tg, n_steps=3)
    check(env.last_neighbors, "env behind step_fused(n_steps=3)")
    check(env.nearest_neighbors(), "env on demand behind the steps")
    with pytest.raises(NotImplementedError):
        env.capture_fused(tg, 2)
    env.close()
    # off by default: nothing behind a step, and no query without a k
    env = CtrlAviary(["tello"], 4, initial_xyzs=pos[:4], dict_io=False, noise_seed=0)
    env.step(torch.zeros((4, 4), dtype=torch.float32, device=env.ctx.device))
    assert env.last_neighbors is None and env._knn is None
    with pytest.raises(ValueError):
        env.nearest_neighbors()
    env.close()


# ---- 6. the receivers are a slice of a larger world ---------------------------------------------------------------------------------
def test_world_form_gives_world_indices(gpu):
    nat, fleet = gpu
    from dronesim_amd.downwash import Downwash
    world = kr.slice_world()
    m, lo, hi, k = world.shape[0], 300, 700, 8
    p32 = world.astype(np.float32)
    wp = torch.from_numpy(np.ascontiguousarray(p32.T)).cuda()
    ctx = fleet.Context([params.builtin_type("tello")])
    st = load(fleet, ctx, world[lo:hi])
    dw = Downwash(ctx, st)
    nb = dw.nearest(R, k, world_pos=wp, local_offset=lo, rel_vel=False)
    assert nb.rel_vel is None
    ref = kr.brute(p32, R, k, lo, hi)
    got = host(nb)
    kr.compare(got, ref, k, R, p32, None, lo=lo, what="world slice")
    assert (got[0] >= hi).any() and ((got[0] >= 0) & (got[0] < lo)).any()         # neighbours on either side of the slice
    with pytest.raises(ValueError):
        dw.nearest(R, k, world_pos=wp, local_offset=lo)                            # rel_vel (the default) with world_pos
    # ... and on the raw entry point
    a, q, _ = dw._knn_args
    sentinel = torch.full((k, 3, st.n_pad), 5.0, device=ctx.device)
    q2 = nat.KnnArgs.from_buffer_copy(q)
    q2.rel_vel_out = sentinel.data_ptr()
    assert ctx.lib.dsim_knn(ctx.handle, ctx.stream_ptr(), st.n, st.view(), ctypes.byref(q2)) == -1
    torch.cuda.synchronize()
    assert torch.all(sentinel == 5.0)
    ctx.close()


# ---- 7. a drone whose position is not finite ----------------------------------------------------------------------------------------
def test_a_nan_position_is_nobodys_neighbour(gpu, standard):
    nat, fleet = gpu
    from dronesim_amd.downwash import Downwash
    k = 8
    pos, vel = kr.standard_world(17)
    lost = int(np.argmax(kr.brute(pos, R, k).count))                  # the busiest drone of the crowd
    pos[lost, 1] = np.nan
    ctx = fleet.Context([params.builtin_type("tello")])
    st = load(fleet, ctx, pos, vel)
    p32, v32 = held(st)
    assert np.isnan(p32[lost, 1])
    index, dist, rel_pos, rel_vel, count = got = host(Downwash(ctx, st).nearest(R, k))
    assert count[lost] == 0 and np.all(index[:, lost] == -1) and np.all(np.isposinf(dist[:, lost]))
    assert np.all(rel_pos[:, :, lost] == 0.0) and np.all(rel_vel[:, :, lost] == 0.0)
    assert not np.any(index == lost)
    # everybody else: the reference of the world without that drone, its indices moved back over the gap
    keep = np.arange(pos.shape[0]) != lost
    ref = kr.brute(p32[keep], R, k, vel32=v32[keep])
    back = np.flatnonzero(keep)
    ok = ~ref.exempt
    np.testing.assert_array_equal(index.T[keep][ok], np.where(ref.index >= 0, back[ref.index.clip(0)], -1)[ok])
    np.testing.assert_array_equal(count[keep][ok], ref.count[ok])
    kr.compare(got, kr.brute(p32, R, k, vel32=v32), k, R, p32, v32, what="one NaN position")
    ctx.close()


# ---- 8. what the raw entry point refuses, with nothing enqueued ---------------------------------------------------------------------
def test_raw_refusals_leave_the_outputs_alone(gpu, standard):
    nat, _ = gpu
    from dronesim_amd.downwash import Downwash
    ctx, st = standard["ctx"], standard["soa"]
    dw = Downwash(ctx, st)
    k = 4
    dw.nearest(R, k)
    a, q, _ = dw._knn_args
    dev = ctx.device
    idx = torch.full((16, st.n_pad), 99, dtype=torch.int32, device=dev)
    flt = torch.full((16, 3, st.n_pad), 5.0, device=dev)
    dst = torch.full((16, st.n_pad), 5.0, device=dev)
    cnt = torch.full((st.n_pad,), 99, dtype=torch.int32, device=dev)

    def call(q=None, a=None, ctx_h=ctx.handle, **over):
        g = nat.DownwashArgs.from_buffer_copy(dw._knn_args[0])
        for name, v in (a or {}).items():
            setattr(g, name, v)
        x = nat.KnnArgs(ctypes.addressof(g), R, k, 0, idx.data_ptr(), dst.data_ptr(), flt.data_ptr(), None, cnt.data_ptr())
        for name, v in over.items():
            setattr(x, name, v)
        return ctx.lib.dsim_knn(ctx_h, ctx.stream_ptr(), st.n, st.view(), ctypes.byref(x) if q is None else q)

    E_ARG, E_UNSUPPORTED = -1, -5
    assert call(ctx_h=None) == E_ARG
    assert call(q=ctypes.POINTER(nat.KnnArgs)()) == E_ARG
    assert call(grid=None) == E_ARG
    assert call(index_out=None) == E_ARG
    for bad_k in (0, -1, 17):
        assert call(k=bad_k) == E_ARG
    for bad_r in (0.0, -1.0, float("inf"), float("nan")):
        assert call(radius=bad_r) == E_ARG
    assert call(flags=1) == E_ARG
    assert call(a={"cell": float(np.float32(R) * np.float32(0.999))}) == E_ARG
    assert call(a={"workspace_len": int(ctx.lib.dsim_knn_workspace(st.n, a.nx, a.ny)) - 1}) == E_ARG
    hp = nat.HaloPlan()
    assert call(a={"halo": ctypes.addressof(hp)}) == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.all(idx == 99) and torch.all(flt == 5.0) and torch.all(dst == 5.0) and torch.all(cnt == 99)
    assert call() == 0                                                # ... and the same record, unchanged, is served
    torch.cuda.synchronize()
    assert torch.equal(idx[:k, : st.n], dw.nearest(R, k).index) and torch.all(idx[k:] == 99)


# ---- 9. the example: a decentralised controller on the observation alone ------------------------------------------------------------
def test_flock_example_keeps_its_distance(gpu):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("fly_velocity_flock_fleet", os.path.join(root, "examples", "fly_velocity_flock_fleet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    q, contacts = mod.main(["--num_drones", "300", "--duration_sec", "2"])
    two_r = 2.0 * float(params.builtin_type("tello").collision_sphere)
    assert contacts == 0 and q[0] > two_r and 0.5 < q[2] < 3.0          # nobody touched; the median neighbour inside the radius
