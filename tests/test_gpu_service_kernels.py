"""The small service kernels every flight passes through — dsim_reset, dsim_traj_sample, dsim_adjacency, dsim_fleet_bounds —
through the bare C-ABI, at their edges, against a plain reference of the same operation: the fp64 definition of reset(), the
oracle's sampler, an exact numpy brute force, numpy's fp32 min / max.  The inputs are built in tests/util.py and their
properties (exact fp32 distances, the named edge counts, the oracle's sampler on every start time) are proved on the CPU by
tests/test_service_inputs_cpu.py."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from dronesim_amd import params
from oracle import oracle as orc
from tests.util import (ADJACENCY_CASES, BOUNDS_KINDS, BOUNDS_SIZES, TRAJ_DT, TRAJ_N, TRAJ_SAMPLES, adjacency_brute, adjacency_case,
                        adjacency_cells, assert_step_parity, bounds_expected, bounds_fleet, f32, random_fleet, reset_expected,
                        reset_inputs, traj_oracle_run, traj_service_fleet, ulp32)

pytestmark = pytest.mark.gpu

DT = float(np.float32(1.0 / 240.0))
SENT = 12345.678
G = 4096                    # guard band, in elements, on either side of every output array
# |q_device - q_fp64| per component, in ulp32(1) = 1.19e-7.  MEASURED on the MI355X over every case of test_reset_vs_fp64_definition
# (18 fleets, 4 launches each): worst 1.017 ulp32(1) = 1.21e-7 (mixed fleet, n = 712; the quaternion's norm: worst 1.000).  The bar
# is twice that, rounded up to a whole ulp — the factor 2 is for other seeds.
QUAT_WORST_MEASURED = 1.017
QUAT_K = float(math.ceil(2.0 * QUAT_WORST_MEASURED))        # 3


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product has no CPU fallback")
    from dronesim_amd import _native as nat
    from dronesim_amd import fleet
    return nat, fleet


def whole_block(b):
    """[F, n_pad] float32 host copy of a BlockedSoA, padding lanes included"""
    d = b._data
    if b.layout != "soa":
        d = d.permute(1, 0, 2).reshape(b.n_fields, b.n_pad)
    return d.cpu().numpy().copy()


def dev_soa(a, n_pad, device, dtype=np.float32):
    """[n, k] host -> [k, n_pad] device, the padding zeroed"""
    o = np.zeros((a.shape[1], n_pad), dtype=dtype)
    o[:, : a.shape[0]] = a.T
    return torch.from_numpy(o).to(device)


# ---------------------------------------------------------------------------------------------------------------------
# 1. reset
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["soa", "tile64", "tile256"])
@pytest.mark.parametrize("n", [1, 65, 712])
@pytest.mark.parametrize("fleet_kind", ["robobee", "mixed"])
def test_reset_vs_fp64_definition(gpu, fleet_kind, n, layout):
    """dsim_reset on a robobee fleet and on a lane-interleaved robobee + hexa_6DOF fleet (26 fields), vel and cmd given and NULL:
    position, velocity and a given command are copied bit for bit; angular velocity, last_vel and last_rates are +0.0; last_thrust
    and the command of a NULL cmd are the per-type values of Oracle.reset_mem (0 behind a quad's four actuators); the quaternion is
    orc.quat_from_euler's to QUAT_K ulp32(1) per component and of unit length to the same bar, at 0, +-pi/2 pitch, +-pi roll and
    yaw, 1e-4 and a spread over (-pi, pi]^3.  The block is filled with a sentinel first: afterwards every padding lane holds the
    reset of a type-0 drone at the origin.  Then one dsim_step from the block against Oracle.step at the bar of every step test."""
    nat, fleet = gpu
    mixed = fleet_kind == "mixed"
    types = [params.builtin_type(m) for m in (["robobee", "hexa_6DOF"] if mixed else ["robobee"])]
    ctx = fleet.Context(types)
    dev = ctx.device
    inp = reset_inputs(n, mixed)
    st = fleet.FleetState(ctx, n, layout, pad=64)
    n_pad, na = st.n_pad, ctx.n_act
    assert st.n_fields == (26 if mixed else 24)
    pos_d, rpy_d, vel_d = (dev_soa(inp[k], n_pad, dev) for k in ("pos", "rpy", "vel"))
    cmd_d = dev_soa(inp["cmd"], n_pad, dev)
    tid_d = None
    if mixed:
        tid_d = torch.zeros(n_pad, dtype=torch.uint8, device=dev)
        tid_d[:n] = torch.from_numpy(inp["tid"])
    worst_q = worst_norm = 0.0
    for vel_given, cmd_given in ((False, False), (False, True), (True, False), (True, True)):
        st._data.fill_(SENT)
        nat.check(ctx.lib.dsim_reset(ctx.handle, ctx.stream_ptr(), n, st.view(), pos_d.data_ptr(), rpy_d.data_ptr(),
                                     vel_d.data_ptr() if vel_given else None, cmd_d.data_ptr() if cmd_given else None,
                                     tid_d.data_ptr() if mixed else None))
        blk = whole_block(st)
        assert np.isfinite(blk).all() and not (blk == np.float32(SENT)).any()
        rigid_e, mem_e = reset_expected(types, inp, vel_given, cmd_given)
        got = blk[:, :n].T
        np.testing.assert_array_equal(got[:, 0:3], rigid_e[:, 0:3].astype(np.float32))
        np.testing.assert_array_equal(got[:, 7:10], rigid_e[:, 7:10].astype(np.float32))
        for f in list(range(10, 19)) + ([] if vel_given else [7, 8, 9]):
            assert not got[:, f].any() and not np.signbit(got[:, f]).any(), f                      # +0.0
        np.testing.assert_array_equal(got[:, 19], mem_e[:, 6].astype(np.float32))
        np.testing.assert_array_equal(got[:, 20:20 + na], mem_e[:, 7:7 + na].astype(np.float32))
        if mixed and not cmd_given:
            assert not got[inp["tid"] == 0, 24:26].any() and (got[inp["tid"] == 1, 24:26] == np.float32(types[1].reset_cmd)).all()
        err = np.abs(got[:, 3:7].astype(np.float64) - rigid_e[:, 3:7]).max() / ulp32(1.0)
        nrm = np.abs(np.linalg.norm(got[:, 3:7].astype(np.float64), axis=1) - 1.0).max() / ulp32(1.0)
        worst_q, worst_norm = max(worst_q, float(err)), max(worst_norm, float(nrm))
        # the padding lanes: a type-0 drone at the origin, zero angles
        pad_e = np.zeros((st.n_fields, n_pad - n), dtype=np.float32)
        pad_e[6] = 1.0
        pad_e[19] = np.float32(types[0].reset_thrust)
        if not cmd_given:
            pad_e[20:20 + types[0].n_act] = np.float32(types[0].reset_cmd)
        np.testing.assert_array_equal(blk[:, n:], pad_e)
    print(f"reset[{fleet_kind},{n},{layout}]: quaternion worst |err| {worst_q:.3f} ulp32(1), worst | |q| - 1 | {worst_norm:.3f} ulp32(1)")
    assert worst_q <= QUAT_K and worst_norm <= QUAT_K, (worst_q, worst_norm)
    # the block (velocity and command given) is a valid start of a flight at these attitudes
    r0, m0 = st.rigid_aos(), st.mem_aos()
    tgt = f32(np.concatenate([r0[:, 0:3] + np.random.default_rng(3).uniform(-1, 1, (n, 3)), np.zeros((n, 6)), np.full((n, 1), 0.4)], 1))
    tg = fleet.Targets(ctx, n, layout, pad=64)
    tg.set_fields(0, torch.from_numpy(np.ascontiguousarray(tgt.T)))
    dtc = float(np.float32(2 / 240))
    a = nat.StepArgs()
    a.phys_substeps, a.dt_phys, a.dt_ctrl = 2, DT, dtc
    a.type_id = tid_d.data_ptr() if mixed else None
    nat.check(ctx.lib.dsim_step(ctx.handle, ctx.stream_ptr(), n, st.view(), tg.view(), ctypes.byref(a)))
    r1, m1 = r0.copy(), m0.copy()
    assert orc.Oracle(types).step(r1, m1, tgt, 2, DT, dtc, type_id=inp["tid"]) == 0
    assert_step_parity(f"step_after_reset[{fleet_kind},{layout}]", types, inp["tid"], r0, m0, tgt, st.rigid_aos(), st.mem_aos(),
                       r1, m1, DT, dtc, 2)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. trajectory sampler
# ---------------------------------------------------------------------------------------------------------------------
_TRAJ_REF = {}


def _traj_ref(golden_dir):
    """(coeffs, TS, t0, ys0, off, rows, t, yaw_state): the fleet and the oracle's run, computed once for both layouts"""
    if not _TRAJ_REF:
        g = np.load(os.path.join(golden_dir, "traj_track_waypoints.npz"))
        t0, ys0, off = traj_service_fleet(g["coeffs"], g["TS"])
        _TRAJ_REF["v"] = (g["coeffs"], g["TS"], t0, ys0, off) + traj_oracle_run(g["coeffs"], g["TS"], t0, ys0)
    return _TRAJ_REF["v"]


def _sample_and_compare(tr, n, samples, dt, off, rows, tt, yy):
    """`samples` launches of tr against the oracle's run: ten fields, t, yaw_state; padding lanes untouched.  NaN where NaN."""
    n_pad = tr.n_pad
    worst = np.zeros(4)
    for k in range(samples):
        tr.sample(dt)
        blk = whole_block(tr)
        T = blk[:, :n].T.astype(np.float64)
        exp_pos = (rows[k][:, 0:3].astype(np.float32) + off.astype(np.float32)).astype(np.float64)       # the kernel's fp32 add
        nan = np.isnan(rows[k])
        np.testing.assert_array_equal(np.isnan(T), nan)
        assert not nan[:, 0:9].any()
        fin = ~nan[:, 9]
        d = [np.abs(T[:, 0:3] - exp_pos).max(), np.abs(T[:, 3:6] - rows[k][:, 3:6]).max(), np.abs(T[:, 6:9] - rows[k][:, 6:9]).max(),
             np.abs(T[fin, 9] - rows[k][fin, 9]).max() if fin.any() else 0.0]
        worst = np.maximum(worst, d)
        assert d[0] <= 2e-6 and d[1] <= 1e-6 and d[2] <= 1e-6 and d[3] <= 2e-5, (k, d)
        t_dev, ys_dev = tr.t.cpu().numpy(), tr.yaw_state.cpu().numpy()
        np.testing.assert_allclose(t_dev[:n], tt[k], rtol=0, atol=1e-12)
        np.testing.assert_array_equal(np.isnan(ys_dev[:, :n]), np.isnan(yy[k]))
        np.testing.assert_allclose(np.nan_to_num(ys_dev[:, :n], nan=0.0), np.nan_to_num(yy[k], nan=0.0), rtol=0, atol=1e-12)
        assert (t_dev[n:] == -3.0).all() and (ys_dev[:, n:] == -3.0).all() and (blk[:, n:] == np.float32(SENT)).all()
    return worst


def _sentinels(tr, n):
    tr._data.fill_(SENT)
    tr.t[n:] = -3.0
    tr.yaw_state[:, n:] = -3.0


@pytest.mark.parametrize("layout", ["soa", "tile64"])
def test_traj_sampler_vs_oracle_at_the_edges(gpu, golden_dir, layout):
    """dsim_traj_sample on 600 drones (n_pad 640: three workgroups, a ragged last one), per-drone offsets, 20 samples at 1/96 s,
    against orc.traj_sample fed the same per-drone t and yaw memory.  Start times: every TS[k] exactly and one fp64 ulp either
    side, TS[-1] + 1e-9 and TS[-1] + 5 (the clamp t_end - 0.001), 0, a spread; 24 drones carry a yaw memory that passes +-pi
    during the run.  Bars of the existing sampler test: 2e-6 m, 1e-6 on velocity and acceleration, 2e-5 rad; t and yaw_state
    to 1e-12; the padding lanes of t, yaw_state and the target block keep their sentinels."""
    nat, fleet = gpu
    coeffs, TS, t0, ys0, off, rows, tt, yy = _traj_ref(golden_dir)
    n = TRAJ_N
    ctx = fleet.Context([params.builtin_type("robobee")])
    tr = fleet.TrajectoryTargets(ctx, n, coeffs, TS, t0=t0, offsets=off, layout=layout, pad=64)
    assert tr.n_pad == 640
    tr.yaw_state[:, :n] = torch.from_numpy(ys0).to(ctx.device)
    _sentinels(tr, n)
    worst = _sample_and_compare(tr, n, TRAJ_SAMPLES, TRAJ_DT, off, rows, tt, yy)
    print(f"traj_sample[{layout}]: worst |device - oracle| pos {worst[0]:.2e} m, vel {worst[1]:.2e}, acc {worst[2]:.2e}, yaw {worst[3]:.2e} rad")
    ctx.close()


@pytest.mark.parametrize("name", ["climb", "launch"])
def test_traj_sampler_at_zero_horizontal_velocity(gpu, golden_dir, name):
    """The rule of trajGen.get_yaw at zero horizontal velocity, as recorded from the reference (golden/traj_edges.npz, pinned to the
    oracle by test_oracle_control.py): the yaw is NaN from that sample on.  Two drones per coefficient set, one started on the zero
    and one started later, against the oracle — NaN where it has NaN — and against the reference's recorded rows."""
    nat, fleet = gpu
    g = np.load(os.path.join(golden_dir, "traj_edges.npz"))
    co, TS = g[f"{name}_coeffs"], g["TS"]
    t0 = np.array([g[f"{name}_t"][0], g[f"{name}_t_late"][0]])
    samples = len(g[f"{name}_t"])
    ys0, off = np.zeros((3, 2)), np.zeros((2, 3))
    rows, tt, yy = traj_oracle_run(co, TS, t0, ys0, samples)
    assert np.isnan(rows[:, 0, 9]).all() and np.isnan(rows[:, 1, 9]).all() == (name == "climb")
    ctx = fleet.Context([params.builtin_type("robobee")])
    tr = fleet.TrajectoryTargets(ctx, 2, co, TS, t0=t0, layout="soa", pad=64)
    _sentinels(tr, 2)
    got = []
    for k in range(samples):
        _sample_and_compare(tr, 2, 1, TRAJ_DT, off, rows[k:k + 1], tt[k:k + 1], yy[k:k + 1])
        got.append(whole_block(tr)[:, :2].T.astype(np.float64))
    got = np.array(got)
    ref0 = g[f"{name}_rows"]
    np.testing.assert_array_equal(np.isnan(got[:, 0, 9]), np.isnan(ref0[:, 9]))
    np.testing.assert_allclose(got[:, 0, 0:9], ref0[:, 0:9], rtol=0, atol=2e-6)
    if name == "launch":                       # the late sampler of this set was recorded at the same times: finite yaw
        ref1 = g["launch_rows_late"]
        np.testing.assert_allclose(got[:, 1, :], ref1, rtol=0, atol=2e-5)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. adjacency
# ---------------------------------------------------------------------------------------------------------------------
def _adjacency(gpu, ctx, c, layout="soa", max_k=None, cell=None):
    """dsim_adjacency through the bare C-ABI on case c (tests/util.py:adjacency_case) -> (rc, count [n], list [max_k, n] or None).
    The world form (pos_all + local_offset) when the receivers are a slice of the world; outputs carved out of guarded arrays."""
    nat, fleet = gpu
    pos, lo, hi = c["pos"], c["lo"], c["hi"]
    n, m = hi - lo, pos.shape[0]
    max_k = c["max_k"] if max_k is None else max_k
    st = fleet.FleetState(ctx, n, layout, pad=64)
    rigid, mem, _ = random_fleet(np.random.default_rng(5), n)
    rigid[:, 0:3] = pos[lo:hi]
    st._data.fill_(SENT)
    st.load_aos(rigid, mem)
    g = nat.DownwashArgs()
    wp = None
    if (lo, hi) != (0, m):
        m_pad = (m + 63) // 64 * 64
        wp = dev_soa(pos, m_pad, ctx.device)
        g.pos_all, g.m, g.m_pad, g.local_offset = wp.data_ptr(), m, m_pad, lo
    else:
        g.pos_all, g.m, g.m_pad, g.local_offset = None, n, n, 0
    g.xmin, g.ymin, g.cell, g.nx, g.ny = c["xmin"], c["ymin"], (c["cell"] if cell is None else cell), c["nx"], c["ny"]
    ws = torch.empty((int(ctx.lib.dsim_downwash_workspace(m, c["nx"], c["ny"])),), dtype=torch.int32, device=ctx.device)
    g.workspace, g.workspace_len = ws.data_ptr(), ws.numel()
    cnt = torch.full((st.n_pad + 2 * G,), -7, dtype=torch.int32, device=ctx.device)
    lst = torch.full((max(max_k, 1) * st.n_pad + 2 * G,), -7, dtype=torch.int32, device=ctx.device)
    rc = ctx.lib.dsim_adjacency(ctx.handle, ctx.stream_ptr(), n, st.view(), ctypes.byref(g), float(c["radius"]),
                                cnt[G:].data_ptr(), lst[G:].data_ptr() if max_k > 0 else None, max_k)
    torch.cuda.synchronize()
    for buf in (cnt, lst):
        assert bool((buf[:G] == -7).all()) and bool((buf[-G:] == -7).all())
    if rc != 0:
        assert bool((cnt == -7).all()) and bool((lst == -7).all())          # refused, not answered
        return rc, None, None
    assert bool((cnt[G + n: G + st.n_pad] == -7).all())
    lists = lst[G: G + max_k * st.n_pad].view(max_k, st.n_pad).cpu().numpy() if max_k > 0 else None
    if lists is not None:
        assert (lists[:, n:] == -7).all()
        lists = lists[:, :n]
    else:
        assert bool((lst == -7).all())
    return rc, cnt[G: G + n].cpu().numpy(), lists


def _check_adjacency(c, cnt, lists, max_k):
    """Equality with the exact brute force, no pair excluded.  count is exact whatever max_k.  The list of receiver i holds
    min(count, max_k) DISTINCT true neighbours as world indices, never i itself, -1 behind them, and is "in ascending grid order"
    (include/dronesim_amd.h): the cell index cy nx + cx of the listed neighbours never decreases along the list (the order inside
    one cell is not specified: slots of a cell are handed out by an atomic counter), and a list that had to be cut holds the
    neighbours of the LOWEST cells — no neighbour left out lies in a lower cell than one that was kept."""
    nb = adjacency_brute(c)
    np.testing.assert_array_equal(cnt, nb.sum(1))
    if lists is None:
        return
    cells = adjacency_cells(c)
    for i in range(nb.shape[0]):
        k = min(int(cnt[i]), max_k)
        l = lists[:k, i]
        assert (lists[k:, i] == -1).all(), i
        assert ((l >= 0) & (l < nb.shape[1])).all() and nb[i, l].all() and len(set(l.tolist())) == k, (i, l)
        assert (np.diff(cells[l]) >= 0).all(), (i, l, cells[l])
        left = np.setdiff1d(np.flatnonzero(nb[i]), l)
        assert (left.size == 0) == (cnt[i] <= max_k)
        if left.size:
            assert cells[left].min() >= cells[l].max(), i


@pytest.mark.parametrize("name", [c for c in ADJACENCY_CASES if c != "overflow"])
def test_adjacency_vs_exact_brute_force(gpu, name):
    """The strict `<` at exactly the radius (cell = radius), drones on cell borders, a grid over the middle of the fleet (a quarter
    of the drones clamped into border cells), the world form with the receivers in the middle slice, fleets of 1, 2, 65 and 700 in
    one cell with eight drones on one point."""
    nat, fleet = gpu
    ctx = fleet.Context([params.builtin_type("robobee")])
    c = adjacency_case(name)
    max_k = 64 if name != "one_cell_700" else 700
    rc, cnt, lists = _adjacency(gpu, ctx, c, max_k=max_k)
    assert rc == 0
    _check_adjacency(c, cnt, lists, max_k)
    ctx.close()


@pytest.mark.parametrize("layout", ["tile64", "tile256"])
@pytest.mark.parametrize("name", ["strict", "middle", "world"])
def test_adjacency_on_tiled_state_blocks(gpu, name, layout):
    nat, fleet = gpu
    ctx = fleet.Context([params.builtin_type("robobee")])
    c = adjacency_case(name)
    rc, cnt, lists = _adjacency(gpu, ctx, c, layout=layout)
    assert rc == 0
    _check_adjacency(c, cnt, lists, c["max_k"])
    ctx.close()


def test_adjacency_list_overflow_counts_only_and_refusal(gpu):
    """max_k = 8 where 300 drones have well over 20 neighbours each and 300 have fewer than 8: count exact, 8 distinct true
    neighbours from the lowest cells, -1 behind a short list.  max_k = 0 with a NULL list: counts alone.  cell < radius is
    refused with DSIM_E_ARG (include/dronesim_amd.h: "args->cell must be >= radius") and nothing is written."""
    nat, fleet = gpu
    ctx = fleet.Context([params.builtin_type("robobee")])
    c = adjacency_case("overflow")
    rc, cnt, lists = _adjacency(gpu, ctx, c)
    assert rc == 0 and (cnt >= 20).sum() >= 300 and ((cnt < 8) & (cnt > 0)).sum() >= 20
    _check_adjacency(c, cnt, lists, 8)
    rc, cnt0, none = _adjacency(gpu, ctx, c, max_k=0)
    assert rc == 0 and none is None
    np.testing.assert_array_equal(cnt0, cnt)
    rc, _, _ = _adjacency(gpu, ctx, c, cell=7.0)
    assert rc == -1 and b"argument" in ctx.lib.dsim_strerror(rc)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. fleet bounds
# ---------------------------------------------------------------------------------------------------------------------
def _bounds(gpu, ctx, rigid, mem, layout, out=None):
    nat, fleet = gpu
    st = fleet.FleetState(ctx, rigid.shape[0], layout, pad=64)
    st._data.fill_(1e30)                        # (a padding lane that leaked into the box would be its maximum)
    st.load_aos(rigid, mem)
    out = torch.full((5,), SENT, dtype=torch.float32, device=ctx.device) if out is None else out
    nat.check(ctx.lib.dsim_fleet_bounds(ctx.handle, ctx.stream_ptr(), rigid.shape[0], st.view(), out.data_ptr()))
    return st, out


@pytest.mark.parametrize("layout", ["soa", "tile64"])
@pytest.mark.parametrize("n", BOUNDS_SIZES)
def test_fleet_bounds_vs_numpy(gpu, n, layout):
    """xmin, ymin, xmax, ymax, max |coordinate velocity| BIT-equal to numpy's fp32 min / max: every coordinate negative (the ~u
    branch of the order-preserving keys alone), a box that straddles 0, magnitudes from 1e-30 to 1e6 of both signs, velocities
    whose largest component is negative; n = 1, one lane short of a wave, a wave, a wave and one, twenty workgroups.  One ctx
    serves every call: each relies on the last workgroup of the call before having reset the keys.
    Zeros of both signs as the extremes: values are compared (0.0 == -0.0); the kernel answers -0.0 for the minimum and +0.0
    for the maximum when both are in the fleet — fminf / fmaxf and the keys order -0.0 below +0.0 — which the test records.
    One drone with NaN x: fminf / fmaxf drop it, the box is that of the finite drones."""
    nat, fleet = gpu
    ctx = fleet.Context([params.builtin_type("robobee")])
    for kind in BOUNDS_KINDS:
        rigid, mem = bounds_fleet(kind, n)
        exp = bounds_expected(rigid)
        _, out = _bounds(gpu, ctx, rigid, mem, layout)
        got = out.cpu().numpy()
        if kind == "zeros":
            np.testing.assert_array_equal(got, exp)                                  # by value
            if n >= 3:
                print(f"fleet_bounds[zeros,{n},{layout}]: xmax is {'-' if np.signbit(got[2]) else '+'}0.0, "
                      f"ymin is {'-' if np.signbit(got[1]) else '+'}0.0")
                assert not np.signbit(got[2]) and np.signbit(got[1])                 # (as measured on the MI355X, every size and layout)
        else:
            np.testing.assert_array_equal(got.view(np.int32), exp.view(np.int32), err_msg=f"{kind}: {got} vs {exp}")
    ctx.close()


def test_fleet_bounds_calls_in_a_row_and_a_nan_drone(gpu):
    """Three calls in a row on one ctx with nothing in between — fleet A, fleet B, fleet A again — each answer its own fleet's.
    Then a fleet with one NaN x: the box ignores that drone, and the downwash grid Downwash._grid_box builds from the box places
    every finite drone in a cell of its own (unclamped)."""
    nat, fleet = gpu
    from dronesim_amd.downwash import Downwash
    ctx = fleet.Context([params.builtin_type("robobee")])
    A, B = bounds_fleet("negative", 5000), bounds_fleet("straddle", 65)
    outs = [torch.full((5,), SENT, dtype=torch.float32, device=ctx.device) for _ in range(3)]
    keep = [_bounds(gpu, ctx, *f, "soa", out=o) for f, o in zip((A, B, A), outs)]
    torch.cuda.synchronize()
    for f, o in zip((A, B, A), outs):
        np.testing.assert_array_equal(o.cpu().numpy().view(np.int32), bounds_expected(f[0]).view(np.int32))
    assert keep
    rigid, mem = bounds_fleet("nan_x", 5000)
    st, out = _bounds(gpu, ctx, rigid, mem, "tile64")
    b = out.cpu().numpy()
    np.testing.assert_array_equal(b.view(np.int32), bounds_expected(rigid).view(np.int32))
    assert np.isfinite(b).all()
    dw = Downwash(ctx, st)
    xmin, ymin, nx, ny = dw._grid_box(None, ((float(b[0]), float(b[1])), (float(b[2]), float(b[3]))))
    fin = np.isfinite(rigid[:, 0])
    assert fin.sum() == 4999
    cx = np.floor((rigid[fin, 0] - xmin) / dw.cell)
    cy = np.floor((rigid[fin, 1] - ymin) / dw.cell)
    assert cx.min() >= 0 and cx.max() <= nx - 1 and cy.min() >= 0 and cy.max() <= ny - 1
    ctx.close()
