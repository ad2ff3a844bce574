"""GPU tests of the swept drone-drone contact watch (dsim_clearance_sweep, Downwash.clearance_sweep / clearance_prime, the env's
drone_sweep keywords) against a brute-force fp64 computation (tests/clearance_sweep_ref.py) on the fp32 positions and previous
positions the device holds.  tests/README_clearance_sweep.md.

Input rule: |x|, |y| <= 128 m; the chords of the drones of every pair within GUARD = 1e-4 m of touching or of the margin, and those
whose length is within 1e-5 of travel, are re-drawn (at most 1 % of the drones, asserted on the reference alone by
tests/test_clearance_sweep_cpu.py).  Counts and the -1 / not -1 status of `nearest` are then compared EXACTLY, clearances with
atol ATOL = 4 x the recorded error of the float32 restatement, and a `nearest` index may differ only where the two smallest c_ij of
that drone are closer than ATOL.  Every case prints the device's own worst difference before it asserts.  A flown state cannot be
re-drawn: there the decision is exact wherever the reference's |c| >= ATOL."""
import ctypes

import numpy as np
import pytest
import torch

from dronesim_amd import params
from tests import clearance_sweep_ref as cs
from tests.clearance_sweep_ref import ATOL, f32
from tests.test_gpu_clearance import contacts, load

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product has no CPU fallback")
    from dronesim_amd import _native as nat
    from dronesim_amd import fleet
    return nat, fleet


def soa3(a, n_pad, device, fill=-5.0):
    t = torch.full((3, n_pad), fill, dtype=torch.float32)
    t[:, : a.shape[0]] = torch.from_numpy(np.ascontiguousarray(a.astype(np.float32).T))
    return t.to(device)


def counters(ctx):
    return (torch.zeros((1,), dtype=torch.int64, device=ctx.device), torch.zeros((1,), dtype=torch.int64, device=ctx.device))


def check(label, got_clr, got_near, ref, margin):
    clr, near, second = ref[0], ref[1], ref[2]
    got_clr, got_near = got_clr.cpu().numpy().astype(np.float64), got_near.cpu().numpy().astype(np.int64)
    print(f"{label}: worst |clearance - fp64| = {np.abs(got_clr - clr).max():.3e} m over {clr.size} drones, "
          f"{int((near >= 0).sum())} in reach, min {clr.min():.4f}")
    np.testing.assert_array_equal(got_near >= 0, near >= 0)
    np.testing.assert_allclose(got_clr, clr, rtol=0, atol=ATOL)
    assert np.all(got_clr[near < 0] == np.float32(margin))
    tie = (near >= 0) & (second - np.minimum(clr, second) < ATOL)
    assert tie.mean() <= 0.01, tie.mean()
    np.testing.assert_array_equal(got_near[~tie], near[~tie])


def positions(st):
    return st.rigid_aos()[:, 0:3].astype(np.float32)


# ---- 1. two robobees, and the sizes -------------------------------------------------------------------------------------------------
def test_two_robobees_swap_and_the_small_cases(gpu):
    nat, fleet = gpu
    from dronesim_amd.downwash import Downwash
    t = params.builtin_type("robobee")
    R = np.float32(t.collision_sphere)
    rad, margin = np.full(2, R), cs.SWAP_MARGIN
    for name, (prev, pos, travel) in cs.small_cases().items():
        ctx = fleet.Context([t])
        st = load(fleet, ctx, pos)
        dw = Downwash(ctx, st)
        d_prev = soa3(f32(prev), st.n_pad, ctx.device)
        pairs, uns = counters(ctx)
        # the point query on the state the step left
        p_pairs = torch.zeros((1,), dtype=torch.int64, device=ctx.device)
        p_clr, p_near = Downwash(ctx, st).clearance(margin, pairs_out=p_pairs)
        before = contacts(ctx, nat)
        clr, near = dw.clearance_sweep(margin, 0.0, travel, d_prev, pairs_out=pairs, unswept_out=uns)
        ref = cs.sweep_pairs_brute(f32(prev), positions(st), rad, margin, 0.0, travel)
        check(name, clr, near, ref, margin)
        assert int(pairs.item()) == ref[3] == contacts(ctx, nat) - before and int(uns.item()) == 0
        assert bool((clr <= p_clr + ATOL).all())
        if name == "swap":
            assert int(p_pairs.item()) == 0 and p_near.cpu().tolist() == [-1, -1]        # the samples see nothing ...
            assert int(pairs.item()) == 1 and near.cpu().tolist() == [1, 0]               # ... the sweep one pair
            np.testing.assert_allclose(clr.cpu().numpy(), [0.05 - 2.0 * float(R)] * 2, rtol=0, atol=ATOL)
        if name == "same velocity":
            assert int(p_pairs.item()) == int(pairs.item()) == 1 and torch.equal(near, p_near)
            np.testing.assert_allclose(clr.cpu().numpy(), p_clr.cpu().numpy(), rtol=0, atol=ATOL)
        assert np.array_equal(d_prev[:, :2].cpu().numpy().T, positions(st)) and bool((d_prev[:, 2:] == -5.0).all())
        ctx.close()


def test_sizes_and_the_sentinels_beyond_n(gpu):
    nat, fleet = gpu
    from dronesim_amd.downwash import Downwash
    t = params.builtin_type("robobee")
    R, margin = np.float32(t.collision_sphere), cs.SWAP_MARGIN
    # n = 1: margin and -1
    ctx = fleet.Context([t])
    st = load(fleet, ctx, np.array([[3.0, -2.0, 1.0]]))
    d_prev = soa3(np.array([[2.9, -2.0, 1.0]]), st.n_pad, ctx.device)
    clr, near = Downwash(ctx, st).clearance_sweep(margin, 0.0, 0.3, d_prev)
    assert clr.cpu().tolist() == [np.float32(margin)] and near.cpu().tolist() == [-1] and contacts(ctx, nat) == 0
    assert d_prev[:, 0].cpu().tolist() == [3.0, -2.0, 1.0]
    ctx.close()
    # n = 257 on a line: a second tile with one lane; raw call, so that the outputs' sentinels beyond n are ours
    prev, pos = cs.line_case()
    n = len(pos)
    ctx = fleet.Context([t])
    st = load(fleet, ctx, pos.astype(np.float64))
    assert st.n_pad > n
    dw = Downwash(ctx, st)
    d_prev = soa3(prev, st.n_pad, ctx.device)
    clr, near = dw.clearance_sweep(margin, 0.0, 0.3, d_prev, keep_prev=True)
    ref = cs.sweep_pairs_brute(prev, positions(st), np.full(n, R), margin, 0.0, 0.3)
    check("line of 257", clr, near, ref, margin)
    assert ref[3] == n - 1 == contacts(ctx, nat) and np.array_equal(d_prev[:, :n].cpu().numpy().T, prev)
    out = torch.full((st.n_pad,), -7.0, dtype=torch.float32, device=ctx.device)
    idx = torch.full((st.n_pad,), -7, dtype=torch.int32, device=ctx.device)
    a = nat.ClearanceSweepArgs(d_prev.data_ptr(), margin, 0.0, 0.3, 0, out.data_ptr(), idx.data_ptr(), None, None)
    assert ctx.lib.dsim_clearance_sweep(ctx.handle, ctx.stream_ptr(), st.n, st.view(), ctypes.byref(dw._clr_args), ctypes.byref(a)) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:n], clr) and torch.equal(idx[:n], near)
    assert bool((out[n:] == -7.0).all()) and bool((idx[n:] == -7).all()) and bool((d_prev[:, n:] == -5.0).all())
    assert np.array_equal(d_prev[:, :n].cpu().numpy().T, positions(st))
    ctx.close()


# ---- 2. the crowded world, chords behind every drone, pairs the 2 travel term exists for ---------------------------------------------
@pytest.mark.parametrize("layout", ["soa", "tile64"])
def test_crowded_world_vs_bruteforce(gpu, layout):
    nat, fleet = gpu
    from dronesim_amd.downwash import Downwash
    d = cs.case_crowded()
    n, margin, travel = len(d["pos"]), d["margin"], d["travel"]
    ctx = fleet.Context([d["type"]])
    st = load(fleet, ctx, d["pos"].astype(np.float64), layout)
    assert np.array_equal(positions(st), d["pos"])
    p_clr, _ = Downwash(ctx, st).clearance(margin)
    dw = Downwash(ctx, st)
    d_prev = soa3(d["prev"], st.n_pad, ctx.device)
    pairs, uns = counters(ctx)
    before = contacts(ctx, nat)
    clr, near = dw.clearance_sweep(margin, d["sag"], travel, d_prev, pairs_out=pairs, unswept_out=uns)
    assert (dw.cell, *dw._box) == d["sweep_grid"]
    check(f"crowded world, {layout}", clr, near, d["ref"], margin)
    assert int(pairs.item()) == d["ref"][3] == contacts(ctx, nat) - before and int(uns.item()) == 0
    # the sweep never reports more room than the samples at the step's end
    worst = float((clr - p_clr).max())
    print(f"swept - point clearance: at most {worst:.3e} m")
    assert worst <= ATOL
    i = np.arange(cs.PLANT_FIRST, cs.PLANT_FIRST + 2 * cs.PLANT_PAIRS)
    assert bool((p_clr[i] > 0).all()) and bool((clr[i] < 0).all())    # (planted: clear at the step's end, in contact inside it)
    # prev moved on to the positions, bit for bit
    assert np.array_equal(d_prev[:, :n].cpu().numpy().T, d["pos"]) and bool((d_prev[:, n:] == -5.0).all())
    # KEEP_PREV: prev untouched, the same tensors
    d_prev2 = soa3(d["prev"], st.n_pad, ctx.device)
    clr2, near2 = dw.clearance_sweep(margin, d["sag"], travel, d_prev2, keep_prev=True)
    assert torch.equal(clr, clr2) and torch.equal(near, near2)
    assert np.array_equal(d_prev2[:, :n].cpu().numpy().T, d["prev"])
    ctx.close()


# ---- 3. a mixed fleet behind the env: type-major storage, the caller's numbering, a type without a sphere -----------------------------
def test_mixed_fleet_through_the_env_in_caller_numbering(gpu):
    nat, _ = gpu
    from dronesim_amd.envs import CtrlAviary
    d = cs.case_mixed()
    n, margin = len(d["pos"]), d["margin"]
    env = CtrlAviary(d["types"], n, initial_xyzs=d["prev"].astype(np.float64), type_ids=d["tid"], drone_watch=True,
                     drone_watch_margin=margin, drone_sweep=True, drone_sweep_sag=d["sag"], drone_sweep_travel=d["travel"],
                     dict_io=False, noise_seed=0)
    assert env.order is not None                                   # (type-major storage)
    assert np.array_equal(env.order.to_caller(env._drone_prev[:, :n], 1).cpu().numpy().T, d["prev"])    # primed where placed
    env.state.set_fields(0, torch.from_numpy(np.ascontiguousarray(d["pos"].T)))
    assert np.array_equal(positions(env.state), d["pos"])
    env._stepped()                                                 # the epilogue of a launch: the watch on the state it finds
    clr, near = env.last_clearance
    check("mixed fleet", clr, near, d["ref"], margin)
    assert env.drone_contacts() == d["ref"][3] and env.drone_unswept() == 0
    c_, n_ = clr.cpu().numpy(), near.cpu().numpy()
    ghost = d["rad"] == 0
    assert np.all(c_[ghost] == np.float32(margin)) and np.all(n_[ghost] == -1)
    assert not np.isin(n_[n_ >= 0], np.flatnonzero(ghost)).any()
    assert np.array_equal(env.order.to_caller(env._drone_prev[:, :n], 1).cpu().numpy().T, d["pos"])
    # on demand: the point query of the current state, not an Env.step
    p_clr, _ = env.drone_clearance(margin)
    assert bool((clr <= p_clr + ATOL).all()) and env.drone_contacts() == d["ref"][3]
    env.close()


# ---- 4. unswept drones, and PRIME ------------------------------------------------------------------------------------------------------
def test_unswept_drones_are_point_samples_and_prime_writes_prev_only(gpu):
    nat, fleet = gpu
    from dronesim_amd.downwash import Downwash
    d = cs.case_unswept()
    n, margin, travel = len(d["pos"]), d["margin"], d["travel"]
    ctx = fleet.Context(d["types"])
    st = fleet.FleetState(ctx, n, "soa")
    st.set_fields(0, torch.from_numpy(np.ascontiguousarray(d["pos"].T)))
    tid = torch.zeros((st.n_pad,), dtype=torch.uint8, device=ctx.device)
    tid[:n] = torch.from_numpy(d["tid"]).to(ctx.device)
    dw = Downwash(ctx, st, tid)
    d_prev = soa3(d["prev"], st.n_pad, ctx.device)
    pairs, uns = counters(ctx)
    clr, near = dw.clearance_sweep(margin, 0.0, travel, d_prev, pairs_out=pairs, unswept_out=uns, box=d["box"])
    check("unswept", clr, near, d["ref"], margin)
    assert int(pairs.item()) == d["ref"][3] == contacts(ctx, nat)
    assert int(uns.item()) == d["ref"][4] == 30                     # (46 point samples, 16 of them without a sphere)
    got_prev = d_prev[:, :n].cpu().numpy().T
    assert np.array_equal(got_prev, d["pos"], equal_nan=True) and np.isnan(got_prev[45, 1])     # the lost drone leaves itself in prev
    # PRIME: prev and nothing else; the outputs are handed in and stay as they were
    out = torch.full((st.n_pad,), -7.0, dtype=torch.float32, device=ctx.device)
    idx = torch.full((st.n_pad,), -7, dtype=torch.int32, device=ctx.device)
    pairs.zero_(); uns.zero_()
    d_prev.fill_(-5.0)
    a = nat.ClearanceSweepArgs(d_prev.data_ptr(), margin, 0.0, travel, nat.SWEEP_PRIME, out.data_ptr(), idx.data_ptr(), pairs.data_ptr(),
                               uns.data_ptr())
    seen = contacts(ctx, nat)
    assert ctx.lib.dsim_clearance_sweep(ctx.handle, ctx.stream_ptr(), st.n, st.view(), ctypes.byref(dw._clr_args), ctypes.byref(a)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(d_prev[:, :n].cpu().numpy().T, d["pos"], equal_nan=True) and bool((d_prev[:, n:] == -5.0).all())
    assert bool((out == -7.0).all()) and bool((idx == -7).all()) and int(pairs.item()) == 0 and int(uns.item()) == 0
    assert contacts(ctx, nat) == seen
    d_prev.fill_(-5.0)
    dw.clearance_prime(d_prev)                                      # (no grid, no outputs)
    assert np.array_equal(d_prev[:, :n].cpu().numpy().T, d["pos"], equal_nan=True) and bool((d_prev[:, n:] == -5.0).all())
    ctx.close()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(gpu):
    nat, fleet = gpu
    from dronesim_amd.downwash import Downwash
    t = params.builtin_type("robobee")
    ctx = fleet.Context([t])
    prev, pos = cs.line_case(64)
    st = load(fleet, ctx, pos.astype(np.float64))
    margin, sag, travel = 0.5, 0.01, 0.2
    dw = Downwash(ctx, st)
    dw.clearance_sweep(margin, sag, travel, soa3(prev, st.n_pad, ctx.device))       # the grid and the workspace of a call in order
    g = dw._clr_args
    need = ctx.lib.dsim_clearance_sweep_workspace(g.m, g.nx, g.ny)
    assert g.workspace_len >= need
    clr = torch.full((st.n_pad,), -7.0, dtype=torch.float32, device=ctx.device)
    near = torch.full((st.n_pad,), -7, dtype=torch.int32, device=ctx.device)
    d_prev = torch.full((3, st.n_pad), -5.0, dtype=torch.float32, device=ctx.device)
    pairs, uns = counters(ctx)
    seen = contacts(ctx, nat)

    def call(grid=g, m=margin, s=sag, tr=travel, flags=0, p=d_prev.data_ptr(), out=clr.data_ptr(), n=st.n, c=ctx.handle, null_args=False):
        a = nat.ClearanceSweepArgs(p, m, s, tr, flags, out, near.data_ptr(), pairs.data_ptr(), uns.data_ptr())
        return ctx.lib.dsim_clearance_sweep(c, ctx.stream_ptr(), n, st.view(), ctypes.byref(grid) if grid is not None else None,
                                            None if null_args else ctypes.byref(a))

    def grid(**kw):
        b = nat.DownwashArgs.from_buffer_copy(g)
        for k, v in kw.items():
            setattr(b, k, v)
        return b
    inf, nan = float("inf"), float("nan")
    world = torch.zeros((3, st.n_pad), dtype=torch.float32, device=ctx.device)
    hp = nat.HaloPlan()
    assert call(grid=grid(pos_all=world.data_ptr(), m_pad=st.n_pad)) == -5 and call(grid=grid(halo=ctypes.addressof(hp))) == -5
    rule = np.float32(2.0) * (np.float32(t.collision_sphere) + np.float32(sag)) + np.float32(margin) + np.float32(2.0) * np.float32(travel)
    assert call(grid=grid(cell=float(rule * np.float32(0.9999)))) == -1
    assert call(grid=grid(workspace_len=need - 1)) == -1
    assert call(tr=0.0) == -1 and call(tr=-0.1) == -1 and call(tr=nan) == -1 and call(tr=inf) == -1
    assert call(s=-1.0) == -1 and call(s=nan) == -1 and call(s=inf) == -1
    assert call(m=inf) == -1 and call(m=0.0) == -1 and call(m=nan) == -1
    assert call(n=st.n_pad + 1) == -1 and call(n=0) == -1
    assert call(null_args=True) == -1 and call(p=None) == -1 and call(out=None) == -1 and call(c=None) == -1 and call(grid=None) == -1
    assert call(flags=3) == -1 and call(flags=4) == -1
    assert call(grid=grid(m=st.n - 1)) == -1                         # (the world is this fleet)
    torch.cuda.synchronize()
    assert bool((clr == -7.0).all()) and bool((near == -7).all()) and bool((d_prev == -5.0).all())
    assert int(pairs.item()) == 0 and int(uns.item()) == 0 and contacts(ctx, nat) == seen
    # more than one type without type_id
    two = fleet.Context([t, params.builtin_type("tello")])
    st2 = load(fleet, two, pos.astype(np.float64))
    a = nat.ClearanceSweepArgs(d_prev.data_ptr(), margin, sag, travel, 0, clr.data_ptr(), None, None, None)
    assert two.lib.dsim_clearance_sweep(two.handle, two.stream_ptr(), st2.n, st2.view(), ctypes.byref(g), ctypes.byref(a)) == -1
    two.close()
    # and the calls that are in order are served: a cell exactly at the rule, a workspace exactly as long as asked for
    d_prev[:, : st.n] = torch.from_numpy(np.ascontiguousarray(prev.T)).to(ctx.device)
    assert call(grid=grid(workspace_len=need), flags=nat.SWEEP_KEEP_PREV) == 0
    torch.cuda.synchronize()
    assert not bool((clr[: st.n] == -7.0).any()) and int(uns.item()) == 0
    ctx.close()


# ---- 6. the env, flown: a column dropped through a hovering row ----------------------------------------------------------------------------
def test_env_dropped_column_sweeps_what_the_samples_miss(gpu):
    nat, _ = gpu
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.fleet import Targets
    from dronesim_amd.obstacles import sweep_sag
    t = params.builtin_type("tello")
    xyz, vel = cs.drop_fleet()
    n, margin, steps = len(xyz), cs.DROP_MARGIN, cs.DROP_STEPS
    sag = sweep_sag(9.8, cs.DROP_DT)
    rad = np.full(n, np.float32(t.collision_sphere))
    kw = dict(initial_xyzs=xyz, initial_vels=vel, aggregate_phy_steps=5, freq=240, drone_watch=True, drone_watch_margin=margin,
              dict_io=False, noise_seed=0)
    sweep = dict(drone_sweep=True, drone_sweep_sag=sag)
    env = CtrlAviary(["tello"], n, drone_sweep_travel=cs.DROP_TRAVEL, **sweep, **kw)
    twin = CtrlAviary(["tello"], n, **kw)
    with pytest.raises(ValueError):
        twin.drone_unswept()
    # the row hovers on its rotors, the column's are off
    act = torch.zeros((n, 4), dtype=torch.float32, device=env.ctx.device)
    act[: cs.DROP_N] = t.hover_pwm
    assert env.drone_contacts() == 0 and env.drone_unswept() == 0 and env.last_clearance is None

    def swept_step(e, total, label):
        before = positions(e.state)
        e.step(act)
        after = positions(e.state)
        ref = cs.sweep_pairs_brute(before, after, rad, margin, sag, cs.DROP_TRAVEL)
        got, got_near = (x.cpu().numpy() for x in e.last_clearance)
        got = got.astype(np.float64)
        np.testing.assert_allclose(got, ref[0], rtol=0, atol=ATOL, err_msg=label)
        inc = e.drone_contacts() - total
        # (the pairs are 1 m apart: a drone overlaps one partner at most, so the device's own count of pairs is half its negative clearances)
        assert 2 * inc == int((got < 0).sum())
        sure = (np.abs(ref[5]) >= ATOL) & (np.abs(ref[5] - margin) >= ATOL)
        np.testing.assert_array_equal((got < 0)[sure], (ref[5] < 0)[sure])
        np.testing.assert_array_equal((got_near >= 0)[sure], (ref[1] >= 0)[sure])
        return inc, ref[3], np.abs(got - ref[0]).max(), after

    total = ref_total = 0
    worst = 0.0
    for k in range(steps):
        inc, r3, err, after = swept_step(env, total, f"step {k}")
        total, ref_total, worst = total + inc, ref_total + r3, max(worst, err)
        twin.step(act)
        assert np.array_equal(positions(twin.state), after)          # (the watch acts on nothing: the same flight)
    print(f"dropped column, {n} tellos x {steps} steps: swept {total} pair-steps in contact (reference {ref_total}), the samples "
          f"{twin.drone_contacts()}; worst |swept - fp64| {worst:.2e} m")
    assert after[: cs.DROP_N, 2].min() > 5.5 and after[cs.DROP_N:, 2].max() < 5.0      # the row stood, the column went through
    assert total >= cs.DROP_N and total > twin.drone_contacts() > 0
    assert env.drone_contacts() == total and env.drone_unswept() == 0
    # after reset() the first step is swept from the placed positions: neither from where the flight ended, nor a point sample
    env.reset()
    assert np.array_equal(positions(env.state), f32(xyz))
    assert np.array_equal(env._drone_prev[:, :n].cpu().numpy().T, f32(xyz))
    swept_step(env, total, "first step after reset")
    assert env.drone_unswept() == 0
    env.close()
    twin.close()
    # four Env.steps per launch: with a travel sized for them every chord is swept; with the default, 10 m/s x one Env.step, the column's are not
    tpos = xyz.copy()
    tpos[cs.DROP_N:, 2] = 0.5                                       # the column is sent on down
    for travel, none_unswept in ((4 * cs.DROP_TRAVEL, True), (None, False)):
        e = CtrlAviary(["tello"], n, drone_sweep_travel=travel, **sweep, **kw)
        tg = Targets(e.ctx, n)
        tg.set(pos=f32(tpos).T, yaw=0.0)
        for k in range(steps // 4):
            before = positions(e.state)
            e.step_fused(tg, n_steps=4)
            chord = np.linalg.norm(positions(e.state).astype(np.float64) - before, axis=1)
            if k == 0:
                assert chord[cs.DROP_N:].min() > 10.0 * cs.DROP_DT and chord.max() < 4 * cs.DROP_TRAVEL
        assert (e.drone_unswept() == 0) == none_unswept, (travel, e.drone_unswept())
        if travel is None:
            with pytest.raises(NotImplementedError):
                e.capture_fused(tg, 4)
        e.close()
