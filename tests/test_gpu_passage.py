"""GPU tests of the gate passage watch (dsim_gate_passage, obstacles.Aperture / gate_passage / gate_prime,
CtrlAviary(gate_watch=...)) against the fp64 reference of tests/passage_ref.py.

Input rule: a chord within GUARD = 1e-4 m of a decision (a plane, a border of the aperture or of the outer rectangle, the travel) is
drawn again, at most 1 % of them (asserted on the reference alone by tests/test_passage_cpu.py).  Decisions — the three masks, due,
laps, the five counters, which passage times are written — are then compared EXACTLY; a passage time by |tau - tau_ref| |s1 - s0|,
metres along the normal, against 4 x the float32 restatement's recorded error (tests/README_passage.md).  Every case prints the
device's own worst figure before it asserts."""
import numpy as np
import pytest
import torch

from dronesim_amd import params
from tests import passage_ref as pr
from tests import scenes_ref as sr
from tests.test_gpu_obstacles import load, soa3
from tests.util import f32

pytestmark = pytest.mark.gpu
SENT, TSENT = -7, -5.0
COUNTERS = ("passes", "wrong_way", "out_of_order", "misses", "unswept")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product has no CPU fallback")
    from dronesim_amd import _native as nat
    from dronesim_amd import fleet
    return nat, fleet


def ids_tensor(sid, n_pad, dev):
    t = torch.full((n_pad,), -1, dtype=torch.int32)
    t[: len(sid)] = torch.from_numpy(np.clip(np.asarray(sid), -(2 ** 31), 2 ** 31 - 1).astype(np.int32))
    return t.to(dev)


class Course:
    """The tensors one drone fleet's queries read and write, with sentinels wherever the call must not write."""

    def __init__(self, ctx, st, G, prev, due, laps, clock=0):
        dev, n_pad, n = ctx.device, st.n_pad, len(due)
        self.ctx, self.st, self.n, self.G = ctx, st, n, G
        pad = lambda a, fill: torch.cat([torch.from_numpy(np.asarray(a, dtype=np.int32)),
                                         torch.full((n_pad - n,), fill, dtype=torch.int32)]).to(dev)
        self.prev = soa3(prev, n_pad, dev)
        self.prev[:, n:] = TSENT
        self.due, self.laps = pad(due, SENT), pad(laps, SENT)
        self.clock = torch.full((1,), clock, dtype=torch.int64, device=dev)
        self.time = torch.full((G, n_pad), TSENT, dtype=torch.float64, device=dev)
        self.fwd, self.back, self.miss = (torch.full((n_pad,), SENT, dtype=torch.int32, device=dev) for _ in range(3))
        self.counts = torch.zeros((5,), dtype=torch.int64, device=dev)

    def query(self, dev_scenes, ids, ap, off=None, wrap=False, keep=False, travel=pr.TRAVEL):
        from dronesim_amd import obstacles as obs
        c = self.counts
        obs.gate_passage(self.ctx, self.st, dev_scenes, ids, ap, travel, self.prev, self.due, self.laps, self.clock, self.time,
                         self.fwd, self.back, self.miss, off, c[0:1], c[1:2], c[2:3], c[3:4], c[4:5], wrap=wrap, keep_prev=keep)

    def snapshot(self):
        return {k: getattr(self, k).clone() for k in ("prev", "due", "laps", "time", "fwd", "back", "miss", "counts")}


def check(c, ref, before, pos32, what, keep=False):
    """Everything one query wrote against the reference; `before`: the snapshot taken ahead of it."""
    n, x = c.n, ref["x"]
    num = lambda t: t.cpu().numpy()
    w = ref["written"]
    for k in ("fwd", "back", "miss"):
        got = num(getattr(c, k)).astype(np.int64) & 0xFFFFFFFF
        np.testing.assert_array_equal(got[:n][w], ref[k][w], err_msg=f"{what}: {k}")
        assert np.array_equal(num(getattr(c, k))[:n][~w], num(before[k])[:n][~w]), f"{what}: {k} of a drone without a scene"
        assert bool((getattr(c, k)[n:] == SENT).all())
    if keep:
        for k in ("prev", "due", "laps", "time"):
            assert torch.equal(getattr(c, k), before[k]), f"{what}: {k} under KEEP_PREV"
    else:
        np.testing.assert_array_equal(num(c.due)[:n], ref["due"], err_msg=f"{what}: due")
        np.testing.assert_array_equal(num(c.laps)[:n], ref["laps"], err_msg=f"{what}: laps")
        assert bool((c.due[n:] == SENT).all()) and bool((c.laps[n:] == SENT).all())
        # prev moved on bit for bit (a NaN too), and not beyond n
        assert np.array_equal(num(c.prev)[:, :n].view(np.int32), np.ascontiguousarray(pos32.T.astype(np.float32)).view(np.int32))
        assert bool((c.prev[:, n:] == TSENT).all())
        t, t0 = num(c.time), num(before["time"])
        written = np.zeros(t.shape, dtype=bool)
        worst = 0.0
        clock = int(c.clock.item())
        for (g, i), want in ref["times"].items():
            written[g, i] = True
            worst = max(worst, abs((t[g, i] - clock) - (want - clock)) * x["span"][i, g])
        print(f"{what}: {len(ref['times'])} passage times, worst |tau - tau_ref| |s1 - s0| = {worst:.3e} m (granted {pr.TAU_TOL:.3e})")
        assert worst <= pr.TAU_TOL
        assert np.array_equal(t[~written], t0[~written]), f"{what}: a passage time written without an advance"
    got = dict(zip(COUNTERS, (num(c.counts) - num(before["counts"])).tolist()))
    print(f"{what}: {got}")
    assert got == {k: ref[k] for k in COUNTERS}, what


def set_pos(st, pos32):
    st.set_fields(0, torch.from_numpy(np.ascontiguousarray(pos32.T.astype(np.float32))).clone())


def finite(pos32):
    p = pos32.copy()
    p[~np.isfinite(p)] = 0.0
    return p


# ---- 1. one gate at the identity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["rect", "ellipse"])
def test_one_gate_at_the_identity(gpu, shape):
    """700 drones (three tiles, the last partial, n < n_pad): forward, backward, missing, parallel and zero-length chords, a NaN
    position, a teleport across the aperture (no event, unswept), and a state planted exactly on the plane — forward once over
    the two queries.  Both layouts."""
    nat, fleet = gpu
    from dronesim_amd import obstacles as obs
    d = pr.case_one(shape)
    n, ap, sc, sid = pr.ONE_N, d["ap"], d["scenes"], d["scene_id"]
    ctx = fleet.Context([params.builtin_type("robobee")])
    dev = sc.to_device(ctx, obs.watch_reach(ctx.types, 1.0))
    for layout in ("soa", "tile64"):
        st = load(fleet, ctx, finite(d["pos"]).astype(np.float32), layout)
        assert st.n_pad > n
        set_pos(st, d["pos"])
        ids = ids_tensor(sid, st.n_pad, ctx.device)
        c = Course(ctx, st, 1, d["prev"], np.zeros(n), np.zeros(n), clock=41)
        ref = pr.reference(d["prev"], d["pos"], None, sc, sid, ap, np.zeros(n), np.zeros(n), clock=41)
        assert ref["unswept"] == 2 and ref["fwd"][pr.ONE_PLANTED] == 1 and ref["fwd"][pr.ONE_TELEPORT] == 0
        before = c.snapshot()
        c.query(dev, ids, ap)
        check(c, ref, before, d["pos"], f"one gate {shape} {layout}")
        assert int(c.fwd[pr.ONE_NAN]) == 0 and int(c.fwd[pr.ONE_TELEPORT]) == 0 and int(c.due[pr.ONE_TELEPORT]) == 0
        assert int(c.fwd[pr.ONE_PLANTED]) == 1 and int(c.due[pr.ONE_PLANTED]) == 1 and float(c.time[0, pr.ONE_PLANTED]) == 42.0
        # onward from the state on the plane: s0 = 0 is no forward crossing
        set_pos(st, d["pos2"])
        c.clock += 1
        ref2 = pr.reference(d["pos"], d["pos2"], None, sc, sid, ap, ref["due"], ref["laps"], clock=42)
        before = c.snapshot()
        c.query(dev, ids, ap)
        check(c, ref2, before, d["pos2"], f"one gate {shape} {layout}, second query")
        assert int(c.fwd[pr.ONE_PLANTED]) == 0 and int(c.due[pr.ONE_PLANTED]) == 1 and ref2["unswept"] == 1   # (the NaN stays)
    dev.close()
    ctx.close()


# ---- 2. placed gates ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offsets", [False, True])
def test_placed_gates(gpu, offsets):
    """K = 64, G = 3, n = 2048, random due on entry; with offsets of +-128 m the wrap flag is on."""
    nat, fleet = gpu
    from dronesim_amd import obstacles as obs
    d = pr.case_placed(offsets)
    n, ap, sc, sid = len(d["scene_id"]), d["ap"], d["scenes"], d["scene_id"]
    ref = pr.reference(d["prev"], d["pos"], d["off"], sc, sid, ap, d["due"], d["laps"], wrap=offsets, clock=5)
    assert d["redrawn"] <= 0.01 and min(ref[k] for k in COUNTERS[:4]) >= 10
    ctx = fleet.Context([params.builtin_type("robobee")])
    dev = sc.to_device(ctx, obs.watch_reach(ctx.types, 0.5))
    for layout in ("soa", "tile64"):
        st = load(fleet, ctx, d["pos"].astype(np.float32), layout)
        off = soa3(d["off"], st.n_pad, ctx.device) if offsets else None
        c = Course(ctx, st, 3, d["prev"], d["due"], d["laps"], clock=5)
        before = c.snapshot()
        c.query(dev, ids_tensor(sid, st.n_pad, ctx.device), ap, off, wrap=offsets)
        check(c, ref, before, d["pos"], f"placed {layout} offsets={offsets}")
    dev.close()
    ctx.close()


# ---- 3. ragged and absent ----------------------------------------------------------------------------------------------------------
def test_ragged_counts_and_absent_scenes(gpu):
    """Counts (0, 1, 2, 3, 8) of G = 8, ids from -1 to K; then ids -1, K and +-2^31 for everybody: every per-drone tensor stays
    bit-identical, prev excepted, and no counter moves."""
    nat, fleet = gpu
    from dronesim_amd import obstacles as obs
    d = pr.case_ragged()
    n, ap, sc, sid = len(d["scene_id"]), d["ap"], d["scenes"], d["scene_id"]
    assert set(sid.tolist()) == set(range(-1, 6))
    ref = pr.reference(d["prev"], d["pos"], d["off"], sc, sid, ap, d["due"], d["laps"], clock=0)
    ctx = fleet.Context([params.builtin_type("robobee")])
    dev = sc.to_device(ctx, obs.watch_reach(ctx.types, 0.5))
    st = load(fleet, ctx, d["pos"].astype(np.float32))
    off = soa3(d["off"], st.n_pad, ctx.device)
    c = Course(ctx, st, 8, d["prev"], d["due"], d["laps"])
    before = c.snapshot()
    c.query(dev, ids_tensor(sid, st.n_pad, ctx.device), ap, off)
    check(c, ref, before, d["pos"], "ragged")
    wild = np.array([-1, 5, 2 ** 31 - 1, -(2 ** 31)])[np.arange(n) % 4]
    c = Course(ctx, st, 8, d["prev"], d["due"], d["laps"])
    before = c.snapshot()
    c.query(dev, ids_tensor(wild, st.n_pad, ctx.device), ap, off, wrap=True)
    after = c.snapshot()
    for k in ("due", "laps", "time", "fwd", "back", "miss", "counts"):
        assert torch.equal(after[k], before[k]), k
    assert torch.equal(after["prev"][:, :n], torch.from_numpy(np.ascontiguousarray(d["pos"].T)).float().to(ctx.device))
    dev.close()
    ctx.close()


# ---- 4. three in a row -------------------------------------------------------------------------------------------------------------
def test_three_gates_in_a_row(gpu):
    """One chord through three gates 0.2 m apart: +3 in order with ascending times, +1 out of order, the wrap with its lap, and a
    finished course staying put without the wrap flag."""
    nat, fleet = gpu
    from dronesim_amd import obstacles as obs
    d = pr.case_row()
    n, ap, sc, sid = len(d["scene_id"]), d["ap"], d["scenes"], d["scene_id"]
    ctx = fleet.Context([params.builtin_type("robobee")])
    dev = sc.to_device(ctx, obs.watch_reach(ctx.types, 0.5))
    st = load(fleet, ctx, d["pos"].astype(np.float32))
    ids = ids_tensor(sid, st.n_pad, ctx.device)
    for wrap, due, laps in ((False, [3, 1, 3, 3, 3, 3, 2, -1], [0] * 8), (True, [0, 1, 0, 3, 1, 0, 2, -1], [1, 0, 1, 0, 1, 1, 0, 0])):
        ref = pr.reference(d["prev"], d["pos"], None, sc, sid, ap, d["due"], d["laps"], wrap=wrap, clock=7)
        c = Course(ctx, st, 3, d["prev"], d["due"], d["laps"], clock=7)
        before = c.snapshot()
        c.query(dev, ids, ap, wrap=wrap)
        check(c, ref, before, d["pos"], f"row wrap={wrap}")
        assert c.due[:n].tolist() == due and c.laps[:n].tolist() == laps and c.fwd[:n].tolist() == [7] * n
        t = c.time[:, 0].tolist()
        assert 7 < t[0] < t[1] < t[2] < 8                                  # drone 0: in order, the times ascending
        assert c.time[:, 1].tolist()[1:] == [TSENT, TSENT] and 7 < float(c.time[0, 1]) < 8     # drone 1: its gate 0 only
        # back to where the chord started (0.6 m: within the travel): three backward crossings each and no progress; then the chord
        # once more: a finished course stays put without the wrap flag, and each of its crossings is out of order
        set_pos(st, d["prev"])
        c.clock += 1
        r2 = pr.reference(d["pos"], d["prev"], None, sc, sid, ap, ref["due"], ref["laps"], wrap=wrap, clock=8)
        before = c.snapshot()
        c.query(dev, ids, ap, wrap=wrap)
        check(c, r2, before, d["prev"], f"row wrap={wrap}, back")
        assert c.back[:n].tolist() == [7] * n and c.due[:n].tolist() == due and r2["wrong_way"] == 3 * n
        set_pos(st, d["pos"])
        c.clock += 1
        r3 = pr.reference(d["prev"], d["pos"], None, sc, sid, ap, r2["due"], r2["laps"], wrap=wrap, clock=9)
        before = c.snapshot()
        c.query(dev, ids, ap, wrap=wrap)
        check(c, r3, before, d["pos"], f"row wrap={wrap}, again")
        if not wrap:
            done = [i for i in range(n) if due[i] == 3]
            assert len(done) == 5 and all(int(c.due[i]) == 3 for i in done) and r3["out_of_order"] >= 3 * len(done)
        else:
            assert c.laps[:n].tolist()[0] == 2
    dev.close()
    ctx.close()


# ---- 5. history --------------------------------------------------------------------------------------------------------------------
def test_keep_prime_and_half_chords(gpu):
    nat, fleet = gpu
    from dronesim_amd import obstacles as obs
    d = pr.case_row()
    n, ap, sc, sid = len(d["scene_id"]), d["ap"], d["scenes"], d["scene_id"]
    a = (sc, sid, ap)
    ctx = fleet.Context([params.builtin_type("robobee")])
    dev = sc.to_device(ctx, obs.watch_reach(ctx.types, 0.5))
    st = load(fleet, ctx, d["pos"].astype(np.float32))
    ids = ids_tensor(sid, st.n_pad, ctx.device)
    whole = pr.reference(d["prev"], d["pos"], None, *a, d["due"], d["laps"])
    # KEEP_PREV: a look ahead — the events and counts of the query, prev and the course as they were
    c = Course(ctx, st, 3, d["prev"], d["due"], d["laps"])
    before = c.snapshot()
    c.query(dev, ids, ap, keep=True)
    check(c, whole, before, d["pos"], "row, KEEP_PREV", keep=True)
    c.query(dev, ids, ap)                                                   # ... and the query itself is still to come
    assert c.due[:n].tolist() == whole["due"].tolist() and int(c.counts[0]) == 2 * whole["passes"]
    # PRIME: prev only
    c = Course(ctx, st, 3, d["prev"], d["due"], d["laps"])
    before = c.snapshot()
    obs.gate_prime(ctx, st, c.prev)
    after = c.snapshot()
    for k in ("due", "laps", "time", "fwd", "back", "miss", "counts"):
        assert torch.equal(after[k], before[k]), k
    assert torch.equal(c.prev[:, :n], torch.from_numpy(np.ascontiguousarray(d["pos"].T)).float().to(ctx.device))
    assert bool((c.prev[:, n:] == TSENT).all())
    c.query(dev, ids, ap)                                                   # a chord of length zero: nothing
    assert not c.fwd[:n].any() and int(c.counts.sum()) == 0
    # two half-chords pass what the whole chord passes
    mid = f32(0.55 * d["prev"] + 0.45 * d["pos"])
    h1 = pr.reference(d["prev"], mid, None, *a, d["due"], d["laps"])
    h2 = pr.reference(mid, d["pos"], None, *a, h1["due"], h1["laps"], clock=1)
    c = Course(ctx, st, 3, d["prev"], d["due"], d["laps"])
    set_pos(st, mid)
    before = c.snapshot()
    c.query(dev, ids, ap)
    check(c, h1, before, mid, "row, first half")
    set_pos(st, d["pos"])
    c.clock += 1
    before = c.snapshot()
    c.query(dev, ids, ap)
    check(c, h2, before, d["pos"], "row, second half")
    assert c.due[:n].tolist() == whole["due"].tolist() and int(c.counts[0]) == whole["passes"] > h1["passes"] > 0
    dev.close()
    ctx.close()


# ---- 6. env ------------------------------------------------------------------------------------------------------------------------
def _env_world(n, K, seed, backward_every=4):
    """Robobee and tello interleaved, K scenes of 3 gates, a frame per drone; every drone 2 cm before the aperture of slot 1 of its
    scene (every fourth: behind it), flying at 3 m/s along the gate's normal (against it)."""
    from dronesim_amd.obstacles import ObstacleScenes
    rng = np.random.default_rng(seed)
    types = [params.builtin_type("robobee"), params.builtin_type("tello")]
    tid = (np.arange(n) % 2).astype(np.uint8)
    pos, rpy = sr.random_placements(rng, K, 3)
    scenes = ObstacleScenes(sr.gate(), pos, rpy)
    sid = (np.arange(n) * 5 + 3) % K
    side = int(np.ceil(np.sqrt(n)))
    off = np.stack([np.arange(n) % side, np.arange(n) // side, np.zeros(n)], 1).astype(np.float64) * 8.0
    sign = np.where(np.arange(n) % backward_every == 3, -1.0, 1.0)
    local = np.stack([-0.02 * sign, rng.uniform(-0.2, 0.2, n), rng.uniform(-0.12, 0.12, n)], 1)
    P = scenes.place[sid, 1].astype(np.float64)
    R, t = P[:, :9].reshape(-1, 3, 3), P[:, 9:]
    xyz = np.einsum("nij,nj->ni", R, local) + t + off
    vel = 3.0 * sign[:, None] * R[:, :, 0]
    goal = np.einsum("nij,nj->ni", R, local + np.array([1.0, 0, 0]) * sign[:, None]) + t + off
    return types, tid, scenes, sid, off, xyz, vel, goal, sign


def _env_check(env, ref_due, prev, sid, off32, ap, scenes, tainted, what):
    """One launch against the reference on the device's own recorded positions: exact where the reference is outside GUARD."""
    pos = env.state.pos.T.cpu().numpy().astype(np.float32)
    n = len(sid)
    ref = pr.reference(prev, pos, off32, scenes, sid, ap, ref_due, np.zeros(n), travel=env._gate_travel)
    tainted |= ref["x"]["bad"]
    ok = ~tainted
    fwd, back, miss = (t.cpu().numpy().astype(np.int64) for t in env.last_gate_events)
    for got, k in ((fwd, "fwd"), (back, "back"), (miss, "miss")):
        np.testing.assert_array_equal(got[ok], ref[k][ok], err_msg=f"{what}: {k}")
    due = env.gate_due.cpu().numpy().astype(np.int64)
    np.testing.assert_array_equal(due[ok], ref["due"][ok], err_msg=f"{what}: due")
    return pos, np.where(ok, ref["due"], due), ref


def test_env_mixed_fleet_in_caller_numbering_and_after_reset(gpu):
    nat, _ = gpu
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.fleet import Targets
    n, K = 128, 8
    types, tid, scenes, sid, off, xyz, vel, goal, sign = _env_world(n, K, 71)
    ap, off32 = pr.gate_aperture(), f32(off)
    env = CtrlAviary(types, n, initial_xyzs=xyz, initial_vels=vel, type_ids=tid, storage="auto", obstacle_offsets=off,
                     obstacle_scene_id=sid, gate_watch=ap, gate_scenes=scenes, gate_start=1, dict_io=False, noise_seed=0)
    assert env.order is not None and not np.array_equal(env.order.drone_np, np.arange(n))
    assert env.last_gate_events is None and env.gate_due.tolist() == [1] * n and bool(torch.isnan(env.gate_pass_time).all())
    tg = Targets(env.ctx, n)
    tg.set(pos=f32(goal).T, yaw=0.0)
    total = [0, 0]
    for rnd in range(2):
        prev = env.state.pos.T.cpu().numpy().astype(np.float32)
        assert np.array_equal(prev, xyz.astype(np.float32))
        due, tainted = np.ones(n, dtype=np.int64), np.zeros(n, dtype=bool)
        passes = wrong = 0
        for step in range(6):
            env.step_fused(tg)
            prev, due, ref = _env_check(env, due, prev, sid, off32, ap, scenes, tainted, f"round {rnd} step {step}")
            passes, wrong = passes + ref["passes"], wrong + ref["wrong_way"]
        print(f"env round {rnd}: {passes} passes, {wrong} wrong-way crossings by the reference, {int(tainted.sum())} drones within GUARD")
        assert tainted.sum() <= 2 and passes >= 0.7 * (sign > 0).sum() and wrong >= 0.7 * (sign < 0).sum()
        fly = (sign > 0) & ~tainted
        assert (env.gate_due.cpu().numpy()[fly] == 2).mean() >= 0.9 and (env.gate_due.cpu().numpy()[(sign < 0) & ~tainted] == 1).all()
        t = env.gate_pass_time.cpu().numpy()
        passed = env.gate_due.cpu().numpy() == 2
        assert np.isfinite(t[1][passed]).all() and np.isnan(t[1][~passed]).all() and np.isnan(t[[0, 2]]).all()
        assert ((t[1][passed] > 0) & (t[1][passed] < 6)).all()
        total = [total[0] + passes, total[1] + wrong]                       # (the counters are cumulative across reset())
        assert abs(env.gate_passes() - total[0]) <= 2 * (rnd + 1) and abs(env.gate_wrong_way() - total[1]) <= 2 * (rnd + 1)
        assert env.gate_unswept() == 0
        # negative control: the ids in the caller's order against the device's answer in storage order would not agree
        if rnd == 0:
            assert (sid[env.order.slot_np] != sid).sum() > n // 2
            env.reset()                                                     # every course starts again, and so do the chords
            assert env.gate_due.tolist() == [1] * n and env.last_gate_events is None
    env.close()


def test_env_eager_vs_captured_replay(gpu):
    nat, _ = gpu
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.fleet import Targets
    n, K = 256, 8
    _, _, scenes, sid, off, xyz, vel, goal, sign = _env_world(n, K, 81)
    ap = pr.gate_aperture()
    envs, tgts = [], []
    for _ in range(2):
        e = CtrlAviary(["robobee"], n, initial_xyzs=xyz, initial_vels=vel, obstacle_watch=scenes, obstacle_margin=0.5,
                       obstacle_offsets=off, obstacle_scene_id=sid, gate_watch=ap, gate_start=1, gate_laps=True, dict_io=False,
                       noise_seed=0)
        assert e._gate is e._obst                                           # (gate_scenes=None: the obstacle watch's device object)
        tg = Targets(e.ctx, n)
        tg.set(pos=f32(goal).T, yaw=0.0)
        envs.append(e)
        tgts.append(tg)
    for _ in range(4):
        envs[0].step_fused(tgts[0])
    g = envs[1].capture_fused(tgts[1], 4)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(envs[0].state.fields(0, 13), envs[1].state.fields(0, 13))
    assert torch.equal(envs[0].gate_due, envs[1].gate_due) and int((envs[1].gate_due == 2).sum()) > n // 2
    t0, t1 = envs[0].gate_pass_time, envs[1].gate_pass_time
    assert torch.equal(torch.isnan(t0), torch.isnan(t1)) and torch.equal(t0[~torch.isnan(t0)], t1[~torch.isnan(t1)])
    assert float(t1[~torch.isnan(t1)].max()) > 1.0                          # (stamped from the device clock: not all in the first chord)
    for a, b in zip(envs[0].last_gate_events, envs[1].last_gate_events):
        assert torch.equal(a, b)
    for f in ("gate_passes", "gate_wrong_way", "gate_out_of_order", "gate_misses", "gate_unswept"):
        assert getattr(envs[0], f)() == getattr(envs[1], f)(), f
    assert envs[1].gate_passes() > n // 2 and envs[1].gate_wrong_way() > n // 8
    g.replay()                                                              # once more: the clock went on, nobody passes twice
    assert int(envs[1]._gate_clock.item()) == 8 and envs[1].gate_passes() >= envs[0].gate_passes()
    for e in envs:
        e.close()
