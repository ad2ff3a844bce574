"""The trajectory bank on the device: dsim_trajgen (K min-snap courses in one launch) against the reference's own trajGenerator
outputs (tests/golden/trajgen_courses.npz) and against tests/trajgen_ref.py, and dsim_traj_sample_bank (a course per drone)
against dsim_traj_sample.  Bars and where they come from: tests/README_trajgen.md."""

import numpy as np
import pytest
import torch

from dronesim_amd import params
from tests import trajgen_ref as R
from tests.test_trajgen_cpu import TRAJGEN_RESTATED_WORST

pytestmark = pytest.mark.gpu

BAR = 4.0 * TRAJGEN_RESTATED_WORST          # the project's convention: 4 x what the restatement differs from the reference by
SETTINGS = ((0.7, 1e6), (2.0, 1e3), (5.0, 100.0))


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product has no CPU fallback")
    from dronesim_amd import _native as nat
    from dronesim_amd import fleet
    return nat, fleet


@pytest.fixture(scope="module")
def courses(golden_dir):
    return R.load_courses(golden_dir)


@pytest.fixture(scope="module")
def ctx(gpu):
    nat, fleet = gpu
    c = fleet.Context([params.builtin_type("robobee")])
    yield c
    c.close()


def group(courses, max_vel):
    return [c for c in courses if c["max_vel"] == max_vel]


def whole(bank):
    """Every output of a bank, padding included, on the host."""
    return [t.cpu().numpy() for t in (bank.coeffs, bank.ts, bank.seg_times, bank._n_seg, bank._cost, bank._evals, bank._status)]


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def check_padding(bank):
    """Past a course's own segments the bank holds NaN."""
    co, ts = bank.coeffs.cpu().numpy(), bank.ts.cpu().numpy()
    for k, n in enumerate(bank.n_seg):
        assert np.isnan(co[n * 30:, k]).all() and np.isnan(ts[n + 1:, k]).all() and not np.isnan(co[:n * 30, k]).any(), k


# ---------------------------------------------------------------------------------------------------------------------
# generator
# ---------------------------------------------------------------------------------------------------------------------
def test_minimize_snap_parity_at_the_references_times(gpu, ctx, courses):
    """The 16 fixture courses in ONE bank (n_seg 1 .. 7 side by side: the padding is exercised), DSIM_TRAJGEN_GIVEN with the reference's
    TS: sampled pos / vel / acc within 4 x TRAJGEN_RESTATED_WORST of the reference's coeffs, cost within the same bound."""
    nat, fleet = gpu
    bank = fleet.TrajectoryBank(ctx, [c["waypoints"] for c in courses], times=[c["TS"] for c in courses])
    assert bank.K == 16 and bank.K_pad == 64 and bank.L_max == 8
    assert (bank.status == 0).all() and (bank.evals == 0).all()
    np.testing.assert_array_equal(bank.n_seg, [len(c["waypoints"]) - 1 for c in courses])
    worst = 0.0
    for k, c in enumerate(courses):
        np.testing.assert_array_equal(bank.TS_of(k), c["TS"])                     # left as given
        np.testing.assert_array_equal(bank.T_of(k), np.diff(c["TS"]))
        w = R.worst_relative(bank.coeffs_of(k), c["coeffs"], c["TS"])
        dc = abs(bank.cost[k] / c["cost"] - 1)
        print(f"course {k}: pos {w[0]:.2e} vel {w[1]:.2e} acc {w[2]:.2e} cost {dc:.2e}")
        worst = max(worst, max(w))
        assert max(w) <= BAR and dc <= BAR, k
    print(f"worst {worst:.3e} (bar {BAR:.3e})")
    check_padding(bank)


def test_tmin_mode(gpu, ctx, courses):
    """DSIM_TRAJGEN_TMIN on the (0.7, 1e6) courses, where the reference's search returned Tmin: ts equal to its TS to 1e-12 relative
    (a norm and a division), coefficients under the bar."""
    nat, fleet = gpu
    cs = group(courses, 0.7)
    assert len(cs) == 6
    bank = fleet.TrajectoryBank(ctx, [c["waypoints"] for c in cs], max_vel=0.7, gamma=1e6, times="tmin")
    assert (bank.status == 0).all() and (bank.evals == 0).all()
    for k, c in enumerate(cs):
        np.testing.assert_allclose(bank.TS_of(k), c["TS"], rtol=1e-12, atol=0)
        np.testing.assert_array_equal(bank.T_of(k), c["Tmin"])
        w = R.worst_relative(bank.coeffs_of(k), c["coeffs"], c["TS"])
        print(f"course {k}: {w}")
        assert max(w) <= BAR, k
    check_padding(bank)


@pytest.mark.parametrize("max_vel,gamma", SETTINGS)
def test_optimize_mode(gpu, ctx, courses, max_vel, gamma):
    """DSIM_TRAJGEN_OPTIMIZE: T >= Tmin exactly, J(T_dev) (evaluated by trajgen_ref) <= J_ref (1 + 1e-6), evals <= max_evals; the
    coefficients are MinimizeSnap(T_dev); max_evals = 1 returns Tmin; two launches are bit-identical."""
    nat, fleet = gpu
    cs = group(courses, max_vel)
    wps = [c["waypoints"] for c in cs]
    bank = fleet.TrajectoryBank(ctx, wps, max_vel=max_vel, gamma=gamma, times="optimize", max_evals=2000)
    assert (bank.status == 0).all()
    evals = bank.evals
    assert (evals >= 1).all() and (evals <= 2000).all()
    for k, c in enumerate(cs):
        T = bank.T_of(k)
        assert (T >= c["Tmin"]).all(), k
        Jd, Jr = R.J(c["waypoints"], T, gamma), R.J(c["waypoints"], np.diff(c["TS"]), gamma)
        print(f"L {len(T) + 1} ({max_vel}, {gamma:g}): J/J_ref - 1 {Jd / Jr - 1:+.2e} in {evals[k]} evaluations")
        assert Jd <= Jr * (1 + 1e-6), k
        np.testing.assert_allclose(bank.TS_of(k)[1:], np.cumsum(T), rtol=1e-15, atol=0)
        co, cost = R.minimize_snap(c["waypoints"], T)
        assert max(R.worst_relative(bank.coeffs_of(k), co, bank.TS_of(k))) <= BAR and abs(bank.cost[k] / cost - 1) <= BAR, k
    again = fleet.TrajectoryBank(ctx, wps, max_vel=max_vel, gamma=gamma, times="optimize", max_evals=2000)
    assert same(whole(bank), whole(again))
    one = fleet.TrajectoryBank(ctx, wps, max_vel=max_vel, gamma=gamma, times="optimize", max_evals=1)
    tmin = fleet.TrajectoryBank(ctx, wps, max_vel=max_vel, gamma=gamma, times="tmin")
    assert (one.evals == 1).all() and (one.status == 0).all()
    for k, c in enumerate(cs):
        np.testing.assert_array_equal(one.T_of(k), c["Tmin"])
    assert same(whole(one)[:3], whole(tmin)[:3])
    capped = fleet.TrajectoryBank(ctx, wps, max_vel=max_vel, gamma=gamma, times="optimize", max_evals=9)
    assert (capped.evals <= 9).all() and (capped.status == 0).all()


@pytest.mark.parametrize("K", [1, 63, 65])
def test_bank_sizes(gpu, ctx, courses, K):
    """K = 1, 63, 65 (K_pad 64, 64, 128: a second workgroup with one course): every course equals the same course in a bank of its
    own kind, bit for bit, wherever it sits."""
    nat, fleet = gpu
    cs = group(courses, 2.0)
    pick = [cs[k % len(cs)] for k in range(K)]
    bank = fleet.TrajectoryBank(ctx, [c["waypoints"] for c in pick], max_vel=2.0, gamma=1e3, times="optimize")
    base = fleet.TrajectoryBank(ctx, [c["waypoints"] for c in cs], max_vel=2.0, gamma=1e3, times="optimize", L_max=bank.L_max)
    assert bank.K_pad == (K + 63) // 64 * 64 and (bank.status == 0).all()
    for k in range(K):
        j = k % len(cs)
        np.testing.assert_array_equal(bank.coeffs_of(k), base.coeffs_of(j))
        np.testing.assert_array_equal(bank.TS_of(k), base.TS_of(j))
        assert bank.cost[k] == base.cost[j] and bank.evals[k] == base.evals[j]
    w = R.worst_relative(bank.coeffs_of(K - 1), R.minimize_snap(pick[-1]["waypoints"], bank.T_of(K - 1))[0], bank.TS_of(K - 1))
    assert max(w) <= BAR
    check_padding(bank)


def test_bank_of_two_waypoint_courses_and_the_longest_bank(gpu, ctx, courses):
    """L = 2 only (no interior waypoint: the reference's unkns == 0 branch, no workspace); a bank at L_max = 9 with a nine-waypoint
    course beside a two-waypoint one, against the restatement; L_max = 10 is DSIM_E_ARG."""
    nat, fleet = gpu
    two = [c for c in courses if len(c["waypoints"]) == 2]
    bank = fleet.TrajectoryBank(ctx, [c["waypoints"] for c in two], times=[c["TS"] for c in two])
    assert bank.L_max == 2 and ctx.lib.dsim_trajgen_workspace(bank.K_pad, 2) == 0 and (bank.status == 0).all()
    for k, c in enumerate(two):
        assert max(R.worst_relative(bank.coeffs_of(k), c["coeffs"], c["TS"])) <= BAR
        assert abs(bank.cost[k] / c["cost"] - 1) <= BAR
    rng = np.random.default_rng(99)
    nine = np.cumsum(rng.uniform(-3, 3, (9, 3)), axis=0) + np.array([0, 0, 6.0])
    ten = np.cumsum(rng.uniform(-3, 3, (10, 3)), axis=0) + np.array([0, 0, 6.0])
    bank = fleet.TrajectoryBank(ctx, [nine, two[0]["waypoints"]], max_vel=2.0, gamma=1e3, times="optimize")
    assert bank.L_max == 9 and (bank.status == 0).all() and list(bank.n_seg) == [8, 1]
    for k, wp in enumerate([nine, two[0]["waypoints"]]):
        T = bank.T_of(k)
        assert (T >= R.tmin(wp, 2.0)).all()
        co, cost = R.minimize_snap(wp, T)
        assert max(R.worst_relative(bank.coeffs_of(k), co, bank.TS_of(k))) <= BAR and abs(bank.cost[k] / cost - 1) <= BAR
        Tr, er = R.search(wp, 2.0, 1e3)
        assert R.J(wp, T, 1e3) <= R.J(wp, Tr, 1e3) * (1 + 1e-6)
    check_padding(bank)
    with pytest.raises(nat.DsimError):
        fleet.TrajectoryBank(ctx, [ten], times="tmin")
    over = fleet.TrajectoryBank(ctx, [ten, nine], times="tmin", L_max=9)          # ten waypoints in a bank with room for nine
    assert list(over.status) == [nat.TRAJGEN_BAD_COUNT, 0]


def test_bad_courses_do_not_touch_their_neighbours(gpu, ctx, courses):
    """A NaN waypoint, two equal consecutive waypoints and a single waypoint among good courses: status != 0, NaN coeffs / ts / cost
    and n_seg 0 for those; the good ones bit-identical to a launch that holds good courses in the bad ones' places."""
    nat, fleet = gpu
    cs = group(courses, 5.0)
    wps = [c["waypoints"].copy() for c in cs] + [c["waypoints"].copy() for c in cs[:3]]
    good = fleet.TrajectoryBank(ctx, wps, max_vel=5.0, gamma=100.0, times="optimize")
    bad = [w.copy() for w in wps]
    bad[1][1, 2] = np.nan
    bad[4][3] = bad[4][2]
    bad[6] = bad[6][:1]
    mixed = fleet.TrajectoryBank(ctx, bad, max_vel=5.0, gamma=100.0, times="optimize", L_max=good.L_max)
    st = mixed.status
    assert st[1] == nat.TRAJGEN_BAD_WAYPOINT and st[4] == nat.TRAJGEN_BAD_SEGMENT and st[6] == nat.TRAJGEN_BAD_COUNT
    a, b = whole(good), whole(mixed)
    for k in range(len(wps)):
        if k in (1, 4, 6):
            assert np.isnan(b[0][:, k]).all() and np.isnan(b[1][:, k]).all() and np.isnan(b[2][:, k]).all()
            assert b[3][k] == 0 and np.isnan(b[4][k]) and b[5][k] == 0
        else:
            assert st[k] == 0 and all(np.array_equal(x[..., k], y[..., k], equal_nan=True) for x, y in zip(a, b)), k
    inf = [w.copy() for w in wps]
    inf[0][0, 0] = np.inf
    assert fleet.TrajectoryBank(ctx, inf, max_vel=5.0, gamma=100.0, times="tmin").status[0] == nat.TRAJGEN_BAD_WAYPOINT
    ts = [np.concatenate([[0.0], np.cumsum(R.tmin(w, 5.0))]) for w in wps]
    ts[2][1] = ts[2][0]
    assert list(fleet.TrajectoryBank(ctx, wps, times=ts).status[:4]) == [0, 0, nat.TRAJGEN_BAD_TIME, 0]


def test_arguments_refused(gpu, ctx, courses):
    """(gamma <= 0 has no minimum under "optimize", the default mode here; "tmin" and given times do not read gamma:
    tests/test_gpu_trajgen_exact.py)"""
    nat, fleet = gpu
    wps = [courses[3]["waypoints"]]
    for kw in (dict(max_vel=0.0), dict(max_vel=float("nan")), dict(gamma=float("inf")), dict(max_evals=0), dict(L_max=1),
               dict(gamma=0.0), dict(gamma=-1.0), dict(gamma=float("nan"))):
        with pytest.raises(nat.DsimError):
            fleet.TrajectoryBank(ctx, wps, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# sampler
# ---------------------------------------------------------------------------------------------------------------------
def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64)


@pytest.fixture(scope="module")
def bank16(gpu, ctx, courses):
    nat, fleet = gpu
    return fleet.TrajectoryBank(ctx, [c["waypoints"] for c in courses], times=[c["TS"] for c in courses])


@pytest.mark.parametrize("layout", ["soa", "tile64"])
def test_one_course_is_bit_identical_to_the_single_course_sampler(gpu, ctx, courses, layout):
    """K = 1, traj_id = 0 on the example's course: 257 drones (two workgroups, the second with one drone), their own t0 and offsets,
    1 300 samples at 1/96 s — past the end of the course, so the clamp and the yaw rule at rest are covered: targets, t and
    yaw_state of dsim_traj_sample_bank and dsim_traj_sample hold the same bits after every sample."""
    nat, fleet = gpu
    c = courses[15]
    bank = fleet.TrajectoryBank(ctx, [c["waypoints"]], max_vel=0.7, gamma=1e6, times="optimize")
    n = 257
    rng = np.random.default_rng(3)
    t0, off = rng.uniform(0, 3, n), rng.uniform(-50, 50, (n, 3))
    t0[0] = 0.0
    assert bank.TS_of(0)[-1] < 1299 / 96
    a = fleet.BankTrajectoryTargets(ctx, n, bank, traj_id=np.zeros(n, dtype=np.int32), t0=t0, offsets=off, layout=layout, pad=64)
    b = fleet.TrajectoryTargets(ctx, n, bank.coeffs_of(0), bank.TS_of(0), t0=t0, offsets=off, layout=layout, pad=64)
    ok = torch.ones((), dtype=torch.bool, device=ctx.device)
    for k in range(1300):
        a.sample(1 / 96)
        b.sample(1 / 96)
        ok &= (bits(a._data) == bits(b._data)).all() & (bits(a.yaw_state) == bits(b.yaw_state)).all() & (bits(a.t) == bits(b.t)).all()
    assert bool(ok)
    yaw = a.fields(9, 1)[0].cpu().numpy()
    assert np.isnan(yaw).any()                         # at rest past the end: the reference's NaN yaw, reached
    assert np.isfinite(a.fields(0, 9).cpu().numpy()).all()


@pytest.mark.parametrize("layout", ["soa", "tile64"])
def test_random_courses_equal_the_single_course_sampler(gpu, ctx, bank16, layout):
    """K = 16, random traj_id on 1 000 drones, 40 samples: every drone equals the single-course call on its own course, bit for bit."""
    nat, fleet = gpu
    n, S = 1000, 40
    rng = np.random.default_rng(4)
    tid = rng.integers(0, 16, n).astype(np.int32)
    tid[:16] = np.arange(16)
    t0, off = rng.uniform(0, 12, n), rng.uniform(-50, 50, (n, 3))
    a = fleet.BankTrajectoryTargets(ctx, n, bank16, traj_id=tid, t0=t0, offsets=off, layout=layout, pad=64)
    got = []
    for s in range(S):
        a.sample(1 / 96)
        got.append(a.fields(0, 10).clone())
    got = torch.stack(got)
    for k in range(16):
        sel = np.flatnonzero(tid == k)
        b = fleet.TrajectoryTargets(ctx, len(sel), bank16.coeffs_of(k), bank16.TS_of(k), t0=t0[sel], offsets=off[sel], layout=layout, pad=64)
        idx = torch.from_numpy(sel).to(ctx.device)
        for s in range(S):
            b.sample(1 / 96)
            assert torch.equal(bits(got[s][:, idx].contiguous()), bits(b.fields(0, 10).contiguous())), (k, s)
        assert torch.equal(bits(a.t[idx]), bits(b.t[: len(sel)])) and torch.equal(bits(a.yaw_state[:, idx].contiguous()),
                                                                                   bits(b.yaw_state[:, : len(sel)].contiguous()))


def test_identity_and_out_of_range_ids(gpu, ctx, bank16):
    """traj_id = None with K == n is traj_id = arange; an id outside [0, K) gives that drone NaN targets and nothing else changes; a
    course that could not be made gives NaN too; None with K != n is refused."""
    nat, fleet = gpu
    n = 16
    t0 = np.linspace(0, 5, n)
    a = fleet.BankTrajectoryTargets(ctx, n, bank16, t0=t0, pad=64)
    b = fleet.BankTrajectoryTargets(ctx, n, bank16, traj_id=np.arange(n), t0=t0, pad=64)
    assert a.traj_id is None
    tid = np.arange(n)
    tid[3], tid[9] = -1, 16
    c = fleet.BankTrajectoryTargets(ctx, n, bank16, traj_id=tid, t0=t0, pad=64)
    for s in range(5):
        for x in (a, b, c):
            x.sample(1 / 96)
        assert torch.equal(bits(a._data), bits(b._data))
        fa, fc = a.fields(0, 10).cpu().numpy(), c.fields(0, 10).cpu().numpy()
        keep = np.setdiff1d(np.arange(n), [3, 9])
        np.testing.assert_array_equal(fa[:, keep], fc[:, keep])
        # (drone 0 starts at t = 0, exactly at rest: its yaw is the rule's NaN, in both objects alike; pos / vel / acc are finite)
        assert np.isnan(fc[:, [3, 9]]).all() and np.isfinite(fc[:9, keep]).all() and np.isfinite(fc[9, keep[1:]]).all()
    np.testing.assert_array_equal(c.t.cpu().numpy()[:n], a.t.cpu().numpy()[:n])
    with pytest.raises(ValueError):
        fleet.BankTrajectoryTargets(ctx, n + 1, bank16)
    wps = [np.array([[0, 0, 1.0], [1, 0, 1]]), np.array([[0, 0, 1.0], [np.nan, 0, 1]])]
    half = fleet.TrajectoryBank(ctx, wps, times="tmin")
    d = fleet.BankTrajectoryTargets(ctx, 2, half, pad=64)
    d.sample(1 / 96)
    f = d.fields(0, 10).cpu().numpy()
    assert np.isfinite(f[:9, 0]).all() and np.isnan(f[:, 1]).all()


def test_type_major_fleet_keeps_the_callers_numbering(gpu, courses):
    """A fleet of two airframes in random order, stored type-major (fleet.StorageOrder): traj_id, t0 and offsets are given and the
    targets read back in the CALLER's numbering, equal to a fleet stored as given; with traj_id = None drone d flies course d."""
    nat, fleet = gpu
    from dronesim_amd.envs import CtrlAviary
    n = 300
    rng = np.random.default_rng(5)
    typ = rng.integers(0, 2, n).astype(np.uint8)
    xyz = np.stack([np.arange(n) % 20, np.arange(n) // 20, np.full(n, 5.0)], 1).astype(np.float64)
    tid = rng.integers(0, 16, n).astype(np.int32)
    t0, off = rng.uniform(0, 8, n), rng.uniform(-20, 20, (n, 3))
    wps = [courses[k % 16]["waypoints"] for k in range(n)]
    out = {}
    for storage in ("auto", "caller"):
        env = CtrlAviary(["robobee", "tello"], n, initial_xyzs=xyz, dict_io=False, type_ids=typ, storage=storage)
        assert (env.order is not None) == (storage == "auto")
        bank = fleet.TrajectoryBank(env.ctx, [c["waypoints"] for c in courses], times=[c["TS"] for c in courses])
        own = fleet.TrajectoryBank(env.ctx, wps, max_vel=2.0, gamma=1e3, times="tmin")
        a = fleet.BankTrajectoryTargets(env.ctx, n, bank, traj_id=tid, t0=t0, offsets=off)
        b = fleet.BankTrajectoryTargets(env.ctx, n, own, t0=t0, offsets=off)
        e = fleet.BankTrajectoryTargets(env.ctx, n, own, traj_id=np.arange(n), t0=t0, offsets=off)
        rows = []
        for s in range(3):
            for x in (a, b, e):
                x.sample(1 / 96)
            rows.append([x.fields(0, 10).cpu().numpy() for x in (a, b, e)])
        out[storage] = rows
        env.close()
    for ra, rc in zip(out["auto"], out["caller"]):
        for x, y in zip(ra, rc):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(ra[1], ra[2])
    assert np.isfinite(out["auto"][0][0][:9]).all()


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
def test_sixty_four_drones_fly_their_own_courses(gpu):
    """64 robobees, a seeded three-gate course each (made on the device at the example's max_vel 0.7, gamma 1e6), 200 control steps
    through env.step_fused(BankTrajectoryTargets): the targets of every step equal those of the drone's course fed through the
    single-course TrajectoryTargets on its own; every state finite, no WLS failure."""
    nat, fleet = gpu
    from dronesim_amd.envs import CtrlAviary
    n, steps, AGGR, FREQ = 64, 200, 2, 240
    rng = np.random.default_rng(6)
    wps = []
    while len(wps) < n:
        w = np.cumsum(rng.uniform(-3, 3, (3, 3)), axis=0) + np.array([0, 0, 6.0])
        if w[:, 2].min() > 1.0:
            wps.append(w)
    off = np.stack([10.0 * (np.arange(n) % 8), 10.0 * (np.arange(n) // 8), np.zeros(n)], 1)
    start = np.array([w[0] for w in wps]) + off
    env = CtrlAviary(["robobee"], n, initial_xyzs=start, aggregate_phy_steps=AGGR, freq=FREQ, dict_io=False)
    bank = fleet.TrajectoryBank(env.ctx, wps, max_vel=0.7, gamma=1e6, times="optimize")
    assert (bank.status == 0).all()
    dt = AGGR / FREQ
    # (a course made here is EXACTLY at rest at t = 0, where the reference's yaw rule gives NaN for good — its own coefficients
    # carry rounding noise there; the flight starts one control step in)
    t0 = np.full(n, dt)
    tgt = fleet.BankTrajectoryTargets(env.ctx, n, bank, t0=t0, offsets=off)
    rows = []
    for k in range(steps):
        tgt.sample(dt)
        rows.append(tgt.fields(0, 10).clone())
        env.step_fused(tgt, control_timestep=dt, action=np.full((n, 4), 0.4, dtype=np.float32) if k == 0 else None)
    rows = torch.stack(rows)                                    # [steps, 10, n]
    for d in range(n):
        one = fleet.TrajectoryTargets(env.ctx, 1, bank.coeffs_of(d), bank.TS_of(d), t0=t0[d:d + 1], offsets=off[d:d + 1], pad=64)
        mine = []
        for k in range(steps):
            one.sample(dt)
            mine.append(one.fields(0, 10)[:, 0].clone())
        assert torch.equal(bits(torch.stack(mine).contiguous()), bits(rows[:, :, d].contiguous())), d
    rigid, mem = env.state.rigid_aos(), env.state.mem_aos()
    assert np.isfinite(rigid).all() and np.isfinite(mem).all() and bool(torch.isfinite(rows).all())
    assert env.ctx.query(nat.QUERY_WLS_FAILURES) == 0
    err = np.linalg.norm(rigid[:, 0:3] - rows[-1, 0:3].T.cpu().numpy().astype(np.float64), axis=1)
    # (printed, not asserted: how closely INDI follows a target is the controller's business, which this feature does not touch,
    # and no bound on it can be derived here.  On an MI355X: typically 0.12-0.17 m behind the target, one drone 0.72 m.)
    print(f"distance to the target after {steps} steps: median {np.median(err):.3f} m, worst {err.max():.3f} m")
    env.close()
