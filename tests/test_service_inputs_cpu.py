"""The inputs of tests/test_gpu_service_kernels.py, checked where no GPU is: every property the device tests rely on is proved
here on the very arrays they use (tests/util.py builds them) — the adjacency distances are exact in fp32, each case holds the
edges it is named for, the reset fleets hold the angle table and stay clear of the Euler clamp, the oracle's sampler runs on
every listed start time and the yaw memories wrap, the bounds fleets have the signs and extremes their names promise."""
import math
import os

import numpy as np
import pytest

from dronesim_amd import params
from oracle import oracle as orc
from tests.util import (ADJ_RADIUS, ADJACENCY_CASES, BOUNDS_KINDS, BOUNDS_SIZES, EULER_CLAMP, HPI32, PI32, RESET_ANGLE_TABLE, TRAJ_DT,
                        TRAJ_N, TRAJ_SAMPLES, TRAJ_WRAPPERS, adjacency_brute, adjacency_case, adjacency_cells, adjacency_d2,
                        bounds_expected, bounds_fleet, reset_expected, reset_inputs, traj_oracle_run, traj_service_fleet)


# ---- reset --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("n", [1, 65, 712])
def test_reset_inputs_hold_the_angle_table_and_avoid_the_euler_clamp(n, mixed):
    inp = reset_inputs(n, mixed)
    for k in ("pos", "rpy", "vel", "cmd"):
        assert np.array_equal(inp[k], inp[k].astype(np.float32).astype(np.float64)), k         # fp32-representable
    rpy = inp["rpy"]
    k = min(n, len(RESET_ANGLE_TABLE))
    np.testing.assert_array_equal(rpy[:k], RESET_ANGLE_TABLE[:k].astype(np.float32).astype(np.float64))
    assert np.abs(rpy).max() <= PI32
    tab = RESET_ANGLE_TABLE
    assert (tab == 0).all(1).any() and (tab[:, 1] == HPI32).any() and (tab[:, 1] == -HPI32).any()
    assert {PI32, -PI32} <= set(tab[:, 0]) and {PI32, -PI32} <= set(tab[:, 2]) and (np.abs(tab) == 1e-4).any()
    if n > len(tab):
        spread = rpy[len(tab):]
        assert (spread.min(0) < -2.5).all() and (spread.max(0) > 2.5).all()                    # the whole of (-pi, pi] on every axis
        assert (np.abs(spread[:, 1]) > math.pi / 2).sum() > n // 4                             # pitch beyond the gimbal point too
        sarg = np.abs(np.sin(spread[:, 1]))
        assert (np.abs(sarg - EULER_CLAMP) >= 1e-4).all()
    if mixed:
        assert inp["cmd"].shape[1] == 6 and not inp["cmd"][inp["tid"] == 0, 4:6].any()
        if n > 1:
            assert set(inp["tid"][:2]) == {0, 1}                                               # lane-interleaved
    types = [params.builtin_type(m) for m in (["robobee", "hexa_6DOF"] if mixed else ["robobee"])]
    rigid, mem = reset_expected(types, inp, True, False)
    np.testing.assert_allclose(np.linalg.norm(rigid[:, 3:7], axis=1), 1.0, rtol=0, atol=1e-15)
    if mixed and n > 1:      # the per-type reset values differ: a kernel that read type 0 for everybody would be seen
        assert types[0].reset_thrust != types[1].reset_thrust and types[0].reset_cmd != types[1].reset_cmd
        assert (mem[inp["tid"] == 1, 6] == np.float32(types[1].reset_thrust)).all() and not mem[inp["tid"] == 0, 11:13].any()


# ---- trajectory sampler -------------------------------------------------------------------------------------------------------
def test_sampler_fleet_holds_every_edge_and_the_oracle_runs_on_it(golden_dir):
    g = np.load(os.path.join(golden_dir, "traj_track_waypoints.npz"))
    co, TS = g["coeffs"], g["TS"]
    t0, ys0, off = traj_service_fleet(co, TS)
    assert len(t0) == TRAJ_N and ys0.shape == (3, TRAJ_N) and off.shape == (TRAJ_N, 3)
    for tk in TS:
        assert (t0 == tk).any() and (t0 == np.nextafter(tk, -np.inf)).any() and (t0 == np.nextafter(tk, np.inf)).any()
    assert (t0 == TS[-1] + 1e-9).any() and (t0 == TS[-1] + 5.0).any() and (t0 == 0.0).any()
    assert (t0 > TS[-1]).sum() >= 3                                                            # the clamp t_end - 0.001
    rows, tt, yy = traj_oracle_run(co, TS, t0, ys0)
    assert np.isfinite(rows).all() and np.isfinite(yy).all()
    np.testing.assert_allclose(tt[-1], t0 + TRAJ_SAMPLES * TRAJ_DT, rtol=0, atol=1e-12)
    # a drone behind the end samples the clamped time, whatever its own t
    late = np.flatnonzero(t0 > TS[-1])
    for i in late:
        y = np.zeros(3)
        np.testing.assert_array_equal(rows[0, i, 0:9], orc.traj_sample(co, TS, TS[-1] - 0.001, y)[0:9])
    # ... and a kernel without the clamp would answer differently by far more than the bars
    far = int(np.flatnonzero(t0 == TS[-1] + 5.0)[0])
    dt_ = t0[far] - TS[-2]
    unclamped = sum(co[10 * (len(TS) - 2) + j] * dt_ ** j for j in range(10))
    assert np.abs(unclamped - rows[0, far, 0:3]).max() > 1.0
    # both segments are sampled, and drones straddle the boundary during the run
    seg_lo, seg_hi = (t0 < TS[1]).sum(), ((t0 >= TS[1]) & (t0 <= TS[-1])).sum()
    assert seg_lo > 100 and seg_hi > 100 and ((t0 < TS[1]) & (t0 + TRAJ_SAMPLES * TRAJ_DT > TS[1])).sum() >= 3
    # the yaw memories wrap through +-pi, in both directions, between two samples (not within rounding of one)
    yaw = rows[:, :, 9]
    jump = np.diff(np.concatenate([ys0[0][None], yaw]), axis=0)                                # (the first sample against the memory)
    wraps = (np.abs(jump) > math.pi).any(0)
    assert wraps[-TRAJ_WRAPPERS:].sum() >= 20 and (jump > math.pi).any() and (jump < -math.pi).any()
    assert (np.abs(np.abs(yaw[:, wraps]) - math.pi) > 1e-6).all()
    assert np.abs(off).max() <= 6.0 and np.abs(rows[:, :, 0:3] + off[None]).max() < 16.0      # one fp32 ulp of a position < 1e-6 m


def test_zero_velocity_sets_are_what_their_names_say(golden_dir):
    g = np.load(os.path.join(golden_dir, "traj_edges.npz"))
    assert not g["climb_coeffs"][:, 0:2][np.arange(20) % 10 != 0].any()                        # x, y constant: a vertical climb
    assert (g["climb_rows"][:, 3:5] == 0).all() and (g["climb_rows"][:, 5] > 0).all()
    assert (g["launch_rows"][0, 3:5] == 0).all() and (np.abs(g["launch_rows"][1:, 3:5]) > 0).all()
    assert np.isnan(g["climb_rows"][:, 9]).all() and np.isnan(g["climb_rows_late"][:, 9]).all()
    assert np.isnan(g["launch_rows"][:, 9]).all() and np.isfinite(g["launch_rows_late"]).all()
    assert (g["climb_t_late"] > g["TS"][-1]).any()                                             # the clamp is among the recorded rows


# ---- adjacency ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ADJACENCY_CASES)
def test_adjacency_distances_are_exact_in_fp32(name):
    """fp32 sums == fp64 sums for EVERY receiver x world pair (not only those the grid visits), in two orders of the sum."""
    c = adjacency_case(name)
    pos = c["pos"]
    assert pos.dtype == np.float32 and pos.min() >= 0 and pos.max() < 256 and np.array_equal(pos * 8, np.round(pos * 8))
    d32, d64 = adjacency_d2(pos, c["lo"], c["hi"]), adjacency_d2(pos, c["lo"], c["hi"], np.float64)
    np.testing.assert_array_equal(d32.astype(np.float64), d64)
    p = pos.astype(np.float32)
    d = p[c["lo"]:c["hi"], None, :] - p[None, :, :]
    other = d[..., 2] * d[..., 2] + (d[..., 1] * d[..., 1] + d[..., 0] * d[..., 0])
    np.testing.assert_array_equal(other, d32)
    assert np.float32(ADJ_RADIUS) ** 2 == 56.25 and c["cell"] >= c["radius"]


def test_adjacency_cases_hold_their_edges():
    R2 = ADJ_RADIUS ** 2
    c = adjacency_case("strict")
    d2 = adjacency_d2(c["pos"], 0, len(c["pos"]), np.float64)
    assert c["cell"] == c["radius"]
    assert (d2 == R2).sum() >= 2 * 50                                                          # pairs AT the radius (both directions)
    assert (d2 == 7.375 ** 2).sum() >= 100 and (d2 == 7.625 ** 2).sum() >= 100
    nb = adjacency_brute(c)
    assert not nb[d2 == R2].any() and nb[d2 == 7.375 ** 2].all() and not nb[d2 == 7.625 ** 2].any()
    assert (nb.sum(1) <= 64).all()
    # `<` turned into `<=` would count every pair at the radius
    assert ((d2 <= R2).sum(1) - 1 != nb.sum(1)).sum() >= 100

    c = adjacency_case("borders")
    on_x, on_y = c["pos"][:, 0] % 8 == 0, c["pos"][:, 1] % 8 == 0
    assert on_x.sum() >= 600 and on_y.sum() >= 400 and (on_x & on_y).sum() >= 100
    nb = adjacency_brute(c)
    cells = adjacency_cells(c)
    i, j = np.nonzero(nb)
    assert ((cells[i] != cells[j]) & (on_x[i] | on_y[i])).sum() >= 200                         # neighbours across a border they sit on
    assert nb.sum(1).max() <= 64

    m = adjacency_case("middle")
    np.testing.assert_array_equal(m["pos"], c["pos"])
    out = (m["pos"][:, 0] < 16) | (m["pos"][:, 0] >= 240) | (m["pos"][:, 1] < 16) | (m["pos"][:, 1] >= 240)
    assert 0.2 <= out.mean() <= 0.3                                                            # a quarter outside the box
    assert (nb[out].sum(1) > 0).sum() >= 100                                                   # ... and they have neighbours
    # clamped into border cells, every neighbour pair still sits in adjacent cells (what makes the 3 x 3 scan exact)
    mc = adjacency_cells(m)
    assert (np.abs(mc[i] % m["nx"] - mc[j] % m["nx"]) <= 1).all() and (np.abs(mc[i] // m["nx"] - mc[j] // m["nx"]) <= 1).all()

    w = adjacency_case("world")
    assert (w["lo"], w["hi"], len(w["pos"])) == (500, 1000, 1500)
    nb = adjacency_brute(w)
    assert nb[:, :500].sum() > 500 and nb[:, 1000:].sum() > 500 and nb[:, 500:1000].sum() > 500   # remote and local neighbours
    assert not nb[np.arange(500), np.arange(500, 1000)].any() and nb.sum(1).max() <= 64

    for n in (1, 2, 65, 700):
        s = adjacency_case(f"one_cell_{n}")
        assert len(s["pos"]) == n and len(set(adjacency_cells(s))) == 1
        if n >= 65:
            assert (np.unique(s["pos"], axis=0, return_counts=True)[1] == 8).sum() == 1        # eight drones on one point
            assert adjacency_brute(s).sum(1).max() >= 64
    o = adjacency_case("overflow")
    cnt = adjacency_brute(o).sum(1)
    assert o["max_k"] == 8 and (cnt >= 20).sum() >= 300 and ((cnt > 0) & (cnt < 8)).sum() >= 20 and (cnt == 0).sum() >= 1


# ---- fleet bounds -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", BOUNDS_SIZES)
def test_bounds_fleets_have_the_signs_their_names_promise(n):
    r, _ = bounds_fleet("negative", n)
    assert (r[:, 0:2] < 0).all() and (r[:, 7:10] < 0).all()
    e = bounds_expected(r)
    assert (e[:4] < 0).all() and e[4] == np.abs(r[:, 7:10]).max() > 0
    # without the ~u of the keys negative floats order BACKWARDS: min and max would swap on this fleet
    if n > 1:
        assert e[0] < e[2] and e[1] < e[3]
    r, _ = bounds_fleet("straddle", n)
    if n > 1:
        e = bounds_expected(r)
        assert e[0] < 0 < e[2] and e[1] < 0 < e[3]
    r, _ = bounds_fleet("zeros", n)
    assert (r[:, 0] <= 0).all() and (r[:, 1] >= 0).all() and r[:, 0].max() == 0 and r[:, 1].min() == 0
    z = r[:, 0] == 0
    assert np.signbit(r[z, 0]).any() and (n < 3 or (~np.signbit(r[z, 0])).any())
    r, _ = bounds_fleet("magnitudes", n)
    a = np.abs(r[:, 0:2])
    assert a.min() >= 1e-31 and a.max() <= 1e6 and np.isfinite(r).all()
    if n >= 5000:
        assert a.min() < 1e-27 and a.max() > 1e5 and (r[:, 0:2] < 0).any() and (r[:, 0:2] > 0).any()
        assert (np.float32(a.min()) > 0)
    r, _ = bounds_fleet("nan_x", n)
    assert np.isnan(r[:, 0]).sum() == (1 if n >= 2 else 0) and np.isfinite(bounds_expected(r)).all()
    assert set(BOUNDS_KINDS) == {"negative", "straddle", "zeros", "magnitudes", "nan_x"}
