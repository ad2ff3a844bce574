"""dsim_trajgen against the exact min-snap solve (tests/golden/trajgen_exact.npz, tests/trajgen_exact.py): short legs beside long
ones, legs from 1 mm to 10 km, a course 1e6 m from the origin — far outside the family of trajgen_courses.npz.  A course is served
within the published bar or refused with DSIM_TRAJGEN_BAD_CONDITION; never served wrong.  The class of every course (A, B-easy,
B-hard) is decided on the CPU from the exact solve and the sweep the library used before, never from the device's output
(tests/test_trajgen_exact_cpu.py).  Bars and where they come from: tests/README_trajgen.md."""

import numpy as np
import pytest
import torch

from dronesim_amd import params
from tests import trajgen_exact as X
from tests import trajgen_ref as R
from tests.test_trajgen_exact_cpu import BAR, TRAJGEN_EXACT_WORST, classify

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product has no CPU fallback")
    from dronesim_amd import _native as nat
    from dronesim_amd import fleet
    return nat, fleet


@pytest.fixture(scope="module")
def ctx(gpu):
    nat, fleet = gpu
    c = fleet.Context([params.builtin_type("robobee")])
    yield c
    c.close()


@pytest.fixture(scope="module")
def exact(golden_dir):
    """The courses of trajgen_exact.npz, each with its class and whether it is benign."""
    cs = X.load_exact(golden_dir)
    cls, benign = classify(cs)
    for c, k, b in zip(cs, cls, benign):
        c["class"], c["benign"] = k, b
    return cs


def cumulative(T):
    return np.concatenate([[0.0], np.cumsum(T)])


def whole(bank):
    """Every output of a bank, padding included, on the host."""
    return [t.cpu().numpy() for t in (bank.coeffs, bank.ts, bank.seg_times, bank._n_seg, bank._cost, bank._evals, bank._status)]


def check_against_exact(nat, bank, cs, what, times_equal):
    """Every course of the bank: served (status 0, finite, within BAR of the exact course on sampled pos / vel / acc and on cost; on
    benign courses within 4 x TRAJGEN_EXACT_WORST) or, B-hard courses only, refused (DSIM_TRAJGEN_BAD_CONDITION, NaN coeffs, ts,
    seg_times, cost, n_seg 0).  Returns the indices refused."""
    co, ts, st, n_seg, cost, evals, status = whole(bank)
    worst = {"A": 0.0, "B-easy": 0.0, "B-hard": 0.0, "benign": 0.0}
    served, refused, failures = [], [], []
    for k, c in enumerate(cs):
        name = f"{what} {k} ({X.FAMILIES[c['family']]}, ratio {c['ratio']:g}, {c['class']})"
        n = len(c["T"])
        if status[k] != 0:
            if not (status[k] == nat.TRAJGEN_BAD_CONDITION and c["class"] == "B-hard"):
                failures.append(f"{name}: status {status[k]}")
                continue
            assert np.isnan(co[:, k]).all() and np.isnan(ts[:, k]).all() and np.isnan(st[:, k]).all(), name
            assert np.isnan(cost[k]) and n_seg[k] == 0, name
            refused.append(k)
            continue
        assert n_seg[k] == n, name
        mine = co[: n * 30, k].reshape(n * 10, 3)
        assert np.isnan(co[n * 30:, k]).all(), name
        if not (np.isfinite(mine).all() and np.isfinite(cost[k])):                                              # never NaN under status 0
            failures.append(f"{name}: status 0 with a coefficient or a cost that is not finite")
            continue
        if times_equal:
            np.testing.assert_array_equal(st[:n, k], c["T"], err_msg=name)
        else:
            # (differences of the given cumulative times: each is rounded at the size of the course's end time)
            np.testing.assert_allclose(st[:n, k], c["T"], rtol=0, atol=4 * np.finfo(np.float64).eps * c["T"].sum(), err_msg=name)
        w = X.worst_relative(mine, c["coeffs"], c["T"])
        dc = abs(cost[k] / c["cost"] - 1.0)
        print(f"{name}: pos {w[0]:.2e} vel {w[1]:.2e} acc {w[2]:.2e} cost {dc:.2e}")
        worst[c["class"]] = max(worst[c["class"]], max(w), dc)
        if not (max(w) <= BAR and dc <= BAR):
            failures.append(f"{name}: status 0 with pos / vel / acc {max(w):.2e}, cost {dc:.2e} from the exact course (bar {BAR:.3e})")
        if c["benign"]:
            worst["benign"] = max(worst["benign"], max(w))
            if not max(w) <= 4.0 * TRAJGEN_EXACT_WORST:
                failures.append(f"{name}: benign, {max(w):.2e} from the exact course (bar {4.0 * TRAJGEN_EXACT_WORST:.1e})")
        if c["class"] == "B-hard":
            served.append(k)
    print(f"{what}: worst difference from the exact course per class {({k: f'{v:.2e}' for k, v in worst.items()})}; "
          f"bars {BAR:.3e}, benign {4.0 * TRAJGEN_EXACT_WORST:.1e}")
    print(f"{what}: B-hard served {[(X.FAMILIES[cs[k]['family']], cs[k]['ratio']) for k in served]}")
    print(f"{what}: B-hard refused {[(X.FAMILIES[cs[k]['family']], cs[k]['ratio']) for k in refused]}")
    assert not failures, "\n".join([f"{len(failures)} courses"] + failures)         # (every course is looked at before the first complaint)
    return refused


@pytest.mark.parametrize("part", ["seeded", "reference"])
def test_given_times_against_the_exact_solve(gpu, ctx, exact, part):
    """DSIM_TRAJGEN_GIVEN at the fixture's T: the seeded list in one bank (126 courses, two workgroups), the 16 courses of
    trajgen_courses.npz at the reference's TS in another."""
    nat, fleet = gpu
    cs = exact[:-16] if part == "seeded" else exact[-16:]
    assert len(cs) <= 128
    bank = fleet.TrajectoryBank(ctx, [c["waypoints"] for c in cs], times=[cumulative(c["T"]) for c in cs], L_max=X.L_MAX)
    assert (bank.evals == 0).all()
    refused = check_against_exact(nat, bank, cs, f"GIVEN {part}", times_equal=False)
    if part == "reference":
        assert not refused


@pytest.mark.parametrize("max_vel", [0.01, 2.0, 100.0])
def test_tmin_against_the_exact_solve(gpu, ctx, exact, max_vel):
    """DSIM_TRAJGEN_TMIN on the courses whose fixture T is Tmin, one bank per max_vel: seg_times equal the fixture's bit for bit."""
    nat, fleet = gpu
    cs = [c for c in exact if c["tmin"] and c["max_vel"] == max_vel]
    assert 3 <= len(cs) <= 128
    bank = fleet.TrajectoryBank(ctx, [c["waypoints"] for c in cs], max_vel=max_vel, times="tmin", L_max=X.L_MAX)
    assert (bank.evals == 0).all()
    refused = check_against_exact(nat, bank, cs, f"TMIN {max_vel:g}", times_equal=True)
    if max_vel == 2.0:
        # both kinds present, so that the neighbours' test below means something; long-short-long is served up to ratio 1 000
        assert refused and len(refused) < sum(c["class"] == "B-hard" for c in cs)
        assert not [k for k in refused if cs[k]["family"] == 0 and cs[k]["ratio"] <= 1e3]
    else:
        assert not refused


def test_refused_courses_do_not_touch_their_neighbours(gpu, ctx, exact):
    """The seeded list holds refused and served courses interleaved.  The served ones are bit-identical to a launch that holds a benign
    course in the place of every refused one (test_bad_courses_do_not_touch_their_neighbours' rule)."""
    nat, fleet = gpu
    cs = exact[:-16]
    mixed = fleet.TrajectoryBank(ctx, [c["waypoints"] for c in cs], times=[cumulative(c["T"]) for c in cs], L_max=X.L_MAX)
    st = mixed.status
    bad = np.flatnonzero(st != 0)
    assert len(bad) >= 4 and (st[bad] == nat.TRAJGEN_BAD_CONDITION).all()
    assert any(st[k - 1] == 0 for k in bad) and any(st[k + 1] == 0 for k in bad)          # interleaved
    clean = [cs[0] if st[k] != 0 else c for k, c in enumerate(cs)]
    good = fleet.TrajectoryBank(ctx, [c["waypoints"] for c in clean], times=[cumulative(c["T"]) for c in clean], L_max=X.L_MAX)
    assert (good.status == 0).all()
    a, b = whole(good), whole(mixed)
    for k in range(len(cs)):
        if st[k] == 0:
            assert all(np.array_equal(x[..., k], y[..., k], equal_nan=True) for x, y in zip(a, b)), k
    for x, y in zip(a, b):                                               # the padding courses too
        assert np.array_equal(x[..., len(cs):], y[..., len(cs):], equal_nan=True)


def optimize_picks(exact):
    """Class A at max_vel 2: the first seed of every pattern at ratio 1, 10 and 100, the far, collinear and there-and-back courses."""
    return [c for k, c in enumerate(exact[:-16]) if c["class"] == "A" and c["tmin"] and c["max_vel"] == 2.0 and
            ((c["family"] < 7 and c["ratio"] in (1.0, 10.0, 100.0) and k % 2 == 0) or c["family"] in (8, 9, 10))]


def test_optimize_on_class_a(gpu, ctx, exact):
    """DSIM_TRAJGEN_OPTIMIZE (gamma 1e3) on 24 class A courses: T >= Tmin exactly; J(T_dev), with the EXACT cost, <= J(Tmin) and within
    1e-6 relative of the J the restated search reaches; coefficients and cost within BAR of the exact solve at the device's own
    seg_times (mpmath on the host, for these courses only)."""
    nat, fleet = gpu
    gamma = 1e3
    cs = optimize_picks(exact)
    assert 20 <= len(cs) <= 40
    bank = fleet.TrajectoryBank(ctx, [c["waypoints"] for c in cs], max_vel=2.0, gamma=gamma, times="optimize", L_max=X.L_MAX)
    assert (bank.status == 0).all() and (bank.evals >= 1).all() and (bank.evals <= 2000).all()
    if not X.HAVE_MPMATH:
        print("mpmath is not importable: the exact solve at the device's times runs in exact fractions")
    worst = 0.0
    for k, c in enumerate(cs):
        T = bank.T_of(k)
        assert (T >= c["T"]).all(), k                                    # (the fixture's T is Tmin, bit for bit)
        np.testing.assert_allclose(bank.TS_of(k)[1:], np.cumsum(T), rtol=1e-15, atol=0)
        co, cost = X.solve(c["waypoints"], T)
        Jd, Jmin = cost + gamma * T.sum(), c["cost"] + gamma * c["T"].sum()
        Tr, _ = R.search(c["waypoints"], 2.0, gamma)
        Jr = X.solve(c["waypoints"], Tr)[1] + gamma * Tr.sum()
        w = X.worst_relative(bank.coeffs_of(k), co, T)
        dc = abs(bank.cost[k] / cost - 1.0)
        print(f"{X.FAMILIES[c['family']]}, ratio {c['ratio']:g}: J/J(Tmin) {Jd / Jmin:.4f}, J/J_restated - 1 {Jd / Jr - 1:+.2e} in {bank.evals[k]} "
              f"evaluations; pos {w[0]:.2e} vel {w[1]:.2e} acc {w[2]:.2e} cost {dc:.2e}")
        worst = max(worst, max(w), dc)
        assert Jd <= Jmin and Jd <= Jr * (1 + 1e-6), k
        assert max(w) <= BAR and dc <= BAR, k
    print(f"OPTIMIZE: worst difference from the exact course at the device's times {worst:.2e} (bar {BAR:.3e})")


def test_gamma_without_a_minimum_is_refused(gpu, ctx, exact):
    """gamma <= 0 with DSIM_TRAJGEN_OPTIMIZE: DSIM_E_ARG, nothing enqueued, outputs untouched.  GIVEN and TMIN do not read gamma and
    serve the course as before."""
    nat, fleet = gpu
    import ctypes
    c = exact[-1]
    for gamma in (0.0, -1.0, -0.0):
        with pytest.raises(nat.DsimError):
            fleet.TrajectoryBank(ctx, [c["waypoints"]], max_vel=0.7, gamma=gamma, times="optimize")
    base = fleet.TrajectoryBank(ctx, [c["waypoints"]], max_vel=0.7, gamma=1e6, times="tmin")
    before = whole(base)
    ws = torch.empty((max(int(ctx.lib.dsim_trajgen_workspace(base.K_pad, base.L_max)), 1),), dtype=torch.float64, device=ctx.device)
    args = nat.TrajGenArgs(wp=base.wp.data_ptr(), n_wp=base.n_wp.data_ptr(), max_vel=0.7, gamma=0.0, mode=nat.TRAJGEN_OPTIMIZE,
                           max_evals=2000, cost=base._cost.data_ptr(), evals=base._evals.data_ptr(), status=base._status.data_ptr(),
                           seg_times=base.seg_times.data_ptr(), workspace=ws.data_ptr(), workspace_len=ws.numel())
    assert ctx.lib.dsim_trajgen(ctx.handle, ctx.stream_ptr(), ctypes.byref(base.c), ctypes.byref(args)) == -1      # DSIM_E_ARG
    torch.cuda.synchronize()
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(before, whole(base)))
    for gamma in (0.0, -1.0):
        for times in ("tmin", [cumulative(c["T"])]):
            b = fleet.TrajectoryBank(ctx, [c["waypoints"]], max_vel=0.7, gamma=gamma, times=times)
            assert (b.status == 0).all()
            if isinstance(times, str):
                assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(before, whole(b)))


@pytest.mark.parametrize("T", [1e-60, 1e60])
def test_given_times_whose_seventh_power_leaves_fp64(gpu, ctx, T):
    """DSIM_TRAJGEN_GIVEN with T = 1e-60 and 1e60 on every segment (T^7 under- and overflows), courses of 2, 3 and 5 waypoints beside
    one at T = 1.5: refused, or finite and within BAR of the exact solve; never NaN under status 0.  The course beside them is served."""
    nat, fleet = gpu
    rng = np.random.default_rng(11)
    wps = [np.cumsum(rng.uniform(-3, 3, (L, 3)), axis=0) for L in (2, 3, 5, 4)]
    Ts = [np.full(len(w) - 1, T) for w in wps[:3]] + [np.full(3, 1.5)]
    bank = fleet.TrajectoryBank(ctx, wps, times=[cumulative(t) for t in Ts])
    co, ts, st, n_seg, cost, evals, status = whole(bank)
    assert status[3] == 0
    for k in range(4):
        if status[k] != 0:
            assert status[k] == nat.TRAJGEN_BAD_CONDITION
            assert np.isnan(co[:, k]).all() and np.isnan(ts[:, k]).all() and np.isnan(st[:, k]).all() and np.isnan(cost[k]) and n_seg[k] == 0
            continue
        n = len(Ts[k])
        mine = co[: n * 30, k].reshape(n * 10, 3)
        assert np.isfinite(mine).all() and np.isfinite(cost[k]) and n_seg[k] == n
        want, wcost = X.solve(wps[k], Ts[k])
        assert max(X.worst_relative(mine, want, Ts[k])) <= BAR and abs(cost[k] / wcost - 1.0) <= BAR, k
    print(f"T = {T:g}: status {list(status[:4])}")
