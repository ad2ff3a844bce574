"""The range scanner on the device (dsim_range_scan, RangeScanner, the env's range_* keywords) against the fp64 brute-force reference of
tests/scan_ref.py, which walks no grid.  tests/README_scan.md.

Outside the reference's ambiguity mask (at most 1 % of a case's rays: asserted on the reference alone in tests/test_scan_cpu.py) hit /
no-hit and the hit id are equal EXACTLY and t is within SCAN_TOL in camera_ref.t_error's metric (4 x the measured error of the float32
restatement of the kernel's arithmetic).  Every case prefills the outputs with -7 and checks that lanes >= n kept it, and prints the
device's own worst error before it asserts."""
import ctypes

import numpy as np
import pytest
import torch

from dronesim_amd import params
from tests import scan_ref as sf
from tests.util import random_fleet

pytestmark = pytest.mark.gpu
T_MIN, T_MAX = sf.T_MIN, sf.T_MAX


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product has no CPU fallback")
    from dronesim_amd import _native as nat
    from dronesim_amd import fleet
    return nat, fleet


def load(fleet, ctx, st7, layout="soa"):
    """A fleet state with pos + quat = st7 [n, 7] float32 (stored in the caller's order)."""
    n = st7.shape[0]
    state = fleet.FleetState(ctx, n, layout)
    rigid, mem, _ = random_fleet(np.random.default_rng(5), n, n_act=ctx.n_act)
    rigid[:, 0:7] = st7
    state.load_aos(rigid, mem)
    return state


def tello_ctx(fleet):
    return fleet.Context([params.builtin_type("tello")])


def scan(scanner, hits=True):
    """One scan into outputs prefilled with -7: (t [B, n] float64, hit [B, n] or None); lanes >= n kept the prefill."""
    scanner.range_out.fill_(-7.0)
    scanner.hit_out.fill_(-7)
    r, h = scanner.scan(hits=hits)
    torch.cuda.synchronize()
    n = scanner.state.n
    assert bool((scanner.range_out[:, n:] == -7.0).all()) and bool((scanner.hit_out[:, n:] == -7).all())
    if not hits:
        assert h is None and bool((scanner.hit_out == -7).all())
    assert not bool((scanner.range_out[:, :n] == -7.0).any())
    return scanner.ranges.cpu().numpy().astype(np.float64), (scanner.hits.cpu().numpy() if hits else None)


def check(label, t, hit, ref, tol=None, miss=np.inf):
    tol = sf.SCAN_TOL if tol is None else tol
    ok = ~ref["ambiguous"]
    got = t < miss if np.isfinite(miss) else np.isfinite(t)
    tt = np.where(got, t, np.inf)
    err = sf.t_error(tt, ref)
    wrong = int((got != np.isfinite(ref["t"]))[ok].sum())
    wrong_id = int((hit != ref["hit"])[ok].sum()) if hit is not None else 0
    print(f"{label}: worst t_error {err:.3e} (tol {tol:.3e}), {wrong} hit / no-hit and {wrong_id} ids differ outside the mask of "
          f"{int(ref['ambiguous'].sum())} of {ref['t'].size} rays")
    differ = ok & ((got != np.isfinite(ref["t"])) | ((hit != ref["hit"]) if hit is not None else False))
    for b, i in np.argwhere(differ)[:8]:                       # the first few rays that differ: (beam, drone, got, reference)
        print(f"  beam {b}, drone {i}: got ({t[b, i]!r}, {hit[b, i] if hit is not None else None}), reference ({ref['t'][b, i]!r}, {ref['hit'][b, i]})")
    assert wrong == 0 and wrong_id == 0
    assert err <= tol
    if np.isfinite(miss):
        assert np.array_equal(t[~got], np.full(int((~got).sum()), miss))


# ---- cases 1 and 2: the set in LDS, the records through L2 --------------------------------------------------------------------------
@pytest.mark.parametrize("subdiv, layout, ground", [(0, "soa", False), (0, "tile64", True), (2, "soa", True), (2, "tile64", False)])
def test_fans_against_the_brute_force_reference(gpu, subdiv, layout, ground):
    nat, fleet = gpu
    from dronesim_amd.scanner import RangeScanner
    c = sf.case_main(subdiv)
    ref = c["ref"][1 if ground else 0]
    assert int((ref["hit"] >= 0).sum()) >= (300 if subdiv == 0 else 150) and set(np.unique(ref["hit"][ref["hit"] >= 0])) == {0, 1}
    ctx = tello_ctx(fleet)
    state = load(fleet, ctx, c["st"], layout)
    assert state.n_pad > state.n or subdiv == 2                # case 1: n = 500 leaves dead lanes
    sc = RangeScanner(ctx, state, c["sc"], c["beams"], T_MIN, T_MAX, ground=ground)
    t, hit = scan(sc)
    check(f"scene({subdiv}), {layout}, ground {ground}", t, hit, ref)
    t2, _ = scan(sc, hits=False)
    assert np.array_equal(t, t2)
    # offsets that are multiples of 1/4 m: p + offset is exact, and the scan is bit-identical
    off = sf.quarter_offsets(7, c["st"].shape[0])
    state_o = load(fleet, ctx, sf.with_offsets(c["st"], off), layout)
    so = RangeScanner(ctx, state_o, sc.set, c["beams"], T_MIN, T_MAX, ground=ground, offsets=off)
    to, ho = scan(so)
    assert np.array_equal(t, to) and np.array_equal(hit, ho)
    sc.close()


def test_the_plane_alone(gpu):
    """No set, no drones: the instance without triangles, every hit analytic."""
    nat, fleet = gpu
    from dronesim_amd.scanner import RangeScanner
    c = sf.case_main(0)
    ref = sf.scan_brute(c["st"], c["beams"], T_MIN, T_MAX, ground=True)
    assert int((ref["hit"] == -2).sum()) > 2000 and ref["ambiguous"].mean() <= sf.MASK_CAP
    ctx = tello_ctx(fleet)
    sc = RangeScanner(ctx, load(fleet, ctx, c["st"]), None, c["beams"], T_MIN, T_MAX, ground=True)
    check("the plane alone", *scan(sc), ref)


@pytest.mark.parametrize("n, chunks", [(65536, 4), (262144, 1)])
def test_beam_chunks_do_not_change_a_beam(gpu, n, chunks):
    """A small fleet spreads chunks of the beams over blockIdx.y (500 drones: one beam per workgroup); 65 536 drones cast the 18
    beams in chunks of 5, 5, 5 and 3, and from 262 144 drones on a workgroup casts them all.  The fleet is case 1's 500 poses over
    and over: drone i reads, bit for bit, what drone i mod 500 of the small fleet reads."""
    nat, fleet = gpu
    from dronesim_amd.scanner import RangeScanner
    c = sf.case_main(0)
    ctx = tello_ctx(fleet)
    dev = c["sc"].to_device(ctx, 1.0)
    t0, h0 = scan(RangeScanner(ctx, load(fleet, ctx, c["st"]), dev, c["beams"], T_MIN, T_MAX, ground=True))
    tiles = (n + 255) // 256
    want = min(18, -(-1024 // tiles)) if tiles < 1024 else 1
    assert -(-18 // -(-18 // want)) == chunks                  # the host's rule (dsim_scan.hip: scan_beams_per_block)
    idx = np.arange(n) % 500
    t, h = scan(RangeScanner(ctx, load(fleet, ctx, c["st"][idx]), dev, c["beams"], T_MIN, T_MAX, ground=True))
    assert np.array_equal(t, t0[:, idx]) and np.array_equal(h, h0[:, idx])
    dev.close()


# ---- case 3: edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subdiv", [0, 2])
def test_axis_beams_from_cell_planes_and_faces(gpu, subdiv):
    nat, fleet = gpu
    from dronesim_amd.scanner import RangeScanner
    c = sf.case_edges(subdiv)
    ref = c["ref"]
    assert int((ref["hit"] >= 0).sum()) >= 10
    ctx = tello_ctx(fleet)
    state = load(fleet, ctx, c["st"])
    sc = RangeScanner(ctx, state, c["sc"], c["beams"], 0.0, 1000.0)
    _, _, d = sf._rays32(c["st"], c["beams"], None)
    assert int((d == 0.0).sum()) == 2 * d.size // 3            # two components of every axis beam's d are exactly 0
    check(f"edges, scene({subdiv})", *scan(sc), ref)
    sc.close()


def test_one_beam_sixty_four_beams_one_drone(gpu):
    nat, fleet = gpu
    from dronesim_amd.scanner import RangeScanner
    c = sf.case_main(0)
    ctx = tello_ctx(fleet)
    dev = c["sc"].to_device(ctx, 1.0)
    for n, beams in ((500, sf.fan(0, down=True)), (40, sf.fan(16, elevations=(-0.6, -0.2, 0.2, 0.6))), (1, c["beams"])):
        st = c["st"][:n]
        ref = sf.scan_brute(st, beams, T_MIN, T_MAX, c["sc"].triangles, c["sc"].body, ground=True)
        assert ref["ambiguous"].mean() <= sf.MASK_CAP
        sc = RangeScanner(ctx, load(fleet, ctx, st), dev, beams, T_MIN, T_MAX, ground=True)
        assert sc.n_beams == beams.shape[0] and beams.shape[0] in (1, 64, 18)
        check(f"n = {n}, B = {beams.shape[0]}", *scan(sc), ref)
    dev.close()


# ---- case 4: range limits -----------------------------------------------------------------------------------------------------------
def test_range_limits_inside_nested_boxes(gpu):
    nat, fleet = gpu
    from dronesim_amd.obstacles import ObstacleSet
    from dronesim_amd.scanner import RangeScanner
    world = ObstacleSet.box((0.0, 0.0, 1.5), (2.0, 2.0, 2.0)) + ObstacleSet.box((0.0, 0.0, 1.5), (6.0, 6.0, 2.5))
    st = np.zeros((3, 7), dtype=np.float32)
    st[:, :3], st[:, 6] = [[0.25, 0.125, 1.8125], [0.375, 0.5, 1.0625], [-0.5, -0.25, 1.0]], 1.0     # (off the faces' diagonals)
    ctx = tello_ctx(fleet)
    state = load(fleet, ctx, st)
    dev = world.to_device(ctx, 1.0)

    def run(t_min, t_max, clamp=False):
        sc = RangeScanner(ctx, state, dev, sf.AXIS_BEAMS, t_min, t_max, clamp=clamp)
        t, h = scan(sc)
        ref = sf.scan_brute(st, sf.AXIS_BEAMS, t_min, t_max, world.triangles, world.body)
        assert not ref["ambiguous"].any()
        check(f"boxes, [{t_min}, {t_max}], clamp {clamp}", t, h, ref, miss=float(np.float32(t_max)) if clamp else np.inf)
        return t, h
    t, h = run(0.0, 10.0)                                      # the inner faces of the inner box
    assert np.array_equal(h, np.zeros((6, 3))) and abs(t[0, 0] - 0.75) < 1e-6 and abs(t[1, 0] - 1.25) < 1e-6
    t, h = run(1.4, 10.0)                                      # t_min beyond the near wall: the next surface
    assert h[0, 0] == 1 and abs(t[0, 0] - 2.75) < 1e-6
    t, h = run(1.4, 2.0)                                       # t_max cuts it
    assert h[0, 0] == -1 and np.isinf(t[0, 0])
    t, h = run(1.4, 2.0, clamp=True)
    assert h[0, 0] == -1 and t[0, 0] == float(np.float32(2.0))
    assert np.array_equal(t[h == -1], np.full(int((h == -1).sum()), 2.0))
    dev.close()


# ---- case 5: undefined poses --------------------------------------------------------------------------------------------------------
def test_undefined_poses_miss_and_disturb_nobody(gpu):
    nat, fleet = gpu
    from dronesim_amd.scanner import RangeScanner
    c = sf.case_main(0)
    ctx = tello_ctx(fleet)
    dev = c["sc"].to_device(ctx, 1.0)
    st = c["st"].copy()
    good = scan(RangeScanner(ctx, load(fleet, ctx, st), dev, c["beams"], T_MIN, T_MAX, ground=True))
    bad = [100, 101, 102, 103]                                 # in the middle of a wave of ordinary drones
    st[100, 1], st[101, 0], st[102, 3:], st[103, 5] = np.nan, np.inf, 0.0, np.nan
    state = load(fleet, ctx, st)
    assert np.isnan(state.rigid_aos()[100, 1]) and np.isinf(state.rigid_aos()[101, 0])
    t, h = scan(RangeScanner(ctx, state, dev, c["beams"], T_MIN, T_MAX, ground=True))
    assert np.isinf(t[:, bad]).all() and (t[:, bad] > 0).all() and (h[:, bad] == -1).all()
    rest = np.setdiff1d(np.arange(st.shape[0]), bad)
    assert np.array_equal(t[:, rest], good[0][:, rest]) and np.array_equal(h[:, rest], good[1][:, rest])
    dev.close()


# ---- case 6: scenes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ground", [False, True])
def test_scenes_against_the_brute_force_reference(gpu, ground):
    nat, fleet = gpu
    from dronesim_amd.scanner import RangeScanner
    c = sf.case_scenes()
    ref = c["ref"][1 if ground else 0]
    hit = ref["hit"]
    assert int((hit >= 0).sum()) >= 50 and set(np.unique(hit[hit >= 0])) == {0, 1, 2}       # every slot is hit (the gate is one body)
    ctx = tello_ctx(fleet)
    sc = RangeScanner(ctx, load(fleet, ctx, c["st"]), c["scenes"], c["beams"], T_MIN, T_MAX, ground=ground, scene_id=c["sid"])
    t, h = scan(sc)
    check(f"scenes, ground {ground}", t, h, ref)
    no_world = (c["sid"] < 0) | (c["sid"] >= c["scenes"].K) | (c["scenes"].count[np.clip(c["sid"], 0, c["scenes"].K - 1)] == 0)
    assert no_world.sum() > 50 and (h[:, no_world] < 0).all()
    sc.close()


@pytest.mark.parametrize("subdiv", [0, 2])
def test_the_identity_placement_is_the_unplaced_scan(gpu, subdiv):
    nat, fleet = gpu
    from dronesim_amd.obstacles import ObstacleScenes
    from dronesim_amd.scanner import RangeScanner
    c = sf.case_main(subdiv)
    ctx = tello_ctx(fleet)
    state = load(fleet, ctx, c["st"])
    plain = RangeScanner(ctx, state, c["sc"], c["beams"], T_MIN, T_MAX, ground=True)
    placed = RangeScanner(ctx, state, ObstacleScenes(c["sc"], np.zeros((1, 1, 3)), np.zeros((1, 1, 3))), c["beams"], T_MIN, T_MAX,
                          ground=True, scene_id=np.zeros(c["st"].shape[0], dtype=np.int64))
    (t0, h0), (t1, h1) = scan(plain), scan(placed)
    assert int((h0 >= 0).sum()) > 100
    assert np.array_equal(t0, t1) and np.array_equal(h0, h1)
    plain.close()
    placed.close()


def test_a_hit_in_the_last_slot_in_front_of_one_in_the_first(gpu):
    nat, fleet = gpu
    from dronesim_amd.scanner import RangeScanner
    c = sf.case_carry()
    assert int(c["carry"].sum()) >= 5                          # fails when best does not carry across placements
    ctx = tello_ctx(fleet)
    sc = RangeScanner(ctx, load(fleet, ctx, c["st"]), c["scenes"], c["beams"], T_MIN, 20.0, scene_id=c["sid"])
    t, h = scan(sc)
    check("scenes, carry", t, h, c["ref"])
    nb = c["scenes"].n_bodies
    ok = c["carry"] & ~c["ref"]["ambiguous"]
    assert (h[ok] // nb == 2).all()
    sc.close()


# ---- case 7: drones -----------------------------------------------------------------------------------------------------------------
def lattice_scanner(fleet, c, world, **kw):
    from dronesim_amd.scanner import RangeScanner
    ctx = tello_ctx(fleet)
    state = load(fleet, ctx, c["st"])
    return RangeScanner(ctx, state, world, c["beams"], T_MIN, T_MAX, drones=True, drone_range=sf.LATTICE_RANGE, **kw)


def test_drones_alone(gpu):
    nat, fleet = gpu
    from dronesim_amd.scanner import RangeScanner
    c = sf.case_lattice(None)
    ref = c["ref"]
    assert int((ref["hit"] <= -3).sum()) >= 200
    sc = lattice_scanner(fleet, c, None)
    t, h = scan(sc)
    check("lattice, drones alone", t, h, ref)
    who = RangeScanner.hit_drone(h)
    assert not (who == np.arange(256)[None, :]).any()          # nobody sees itself
    assert np.array_equal(RangeScanner.hit_drone(sc.hits).cpu().numpy(), who)
    assert (t[who >= 0] <= sf.LATTICE_RANGE).all() and sc.drones_outside() == 0
    # a pinned box that leaves the last rows of the lattice outside: those drones are still seen
    pinned = lattice_scanner(fleet, c, None, drone_box=(-0.5, -0.5, 11.75, 8.0))
    tp, hp = scan(pinned)
    assert pinned.drones_outside() >= 16
    assert np.array_equal(t, tp) and np.array_equal(h, hp)
    assert int((who >= 240).sum()) > 0                         # the last row is among what is seen


@pytest.mark.parametrize("world", ["set", "set2"])
def test_drones_with_the_set_standing_in_the_lattice(gpu, world):
    nat, fleet = gpu
    c = sf.case_lattice(world)
    ref, alone = c["ref"], sf.case_lattice(None)["ref"]
    sc_set = sf.lattice_scene(0 if world == "set" else 2)
    bare = sf.scan_brute(c["st"], c["beams"], T_MIN, T_MAX, tri=sc_set.triangles, body=sc_set.body) if world == "set" else None
    front = int(((ref["hit"] >= 0) & (alone["hit"] <= -3)).sum())
    assert front >= 3                                          # triangles in front of spheres
    if bare is not None:
        assert int(((ref["hit"] <= -3) & (bare["hit"] >= 0)).sum()) >= 3        # and spheres in front of triangles
    sc = lattice_scanner(fleet, c, sc_set)
    check(f"lattice, {world}", *scan(sc), ref)
    sc.close()


@pytest.mark.parametrize("world", ["scenes", "scenes2"])
def test_scenes_and_drones_together(gpu, world):
    """The camera refuses this pair; the scanner serves it."""
    nat, fleet = gpu
    c = sf.case_lattice(world)
    ref = c["ref"]
    assert int((ref["hit"] >= 0).sum()) >= 50 and int((ref["hit"] <= -3).sum()) >= 200
    sc = lattice_scanner(fleet, c, c["scenes"], scene_id=c["scene_id"])
    check(f"lattice, {world}", *scan(sc), ref)
    sc.close()


def mixed_env(**kw):
    from dronesim_amd.envs import CtrlAviary
    c = sf.case_lattice(None, True)
    env = CtrlAviary(c["models"], 256, initial_xyzs=c["st"][:, :3].astype(np.float64), noise_seed=0, dict_io=False,
                     ground_plane=False, **kw)
    env.state.set_fields(0, torch.from_numpy(np.ascontiguousarray(c["st"].T)))
    return env, c


def test_a_mixed_fleet_stored_type_major_names_drones_as_the_caller_does(gpu):
    nat, fleet = gpu
    from dronesim_amd.scanner import RangeScanner
    env, c = mixed_env()
    assert env.order is not None                               # type-major storage: not the caller's order
    sc = RangeScanner(env.ctx, env.state, None, c["beams"], T_MIN, T_MAX, type_id=env._type_id, drones=True, drone_range=sf.LATTICE_RANGE)
    t, h = scan(sc)
    check("lattice, mixed fleet", t, h, c["ref"])
    assert not (RangeScanner.hit_drone(h) == np.arange(256)[None, :]).any()
    env.close()


# ---- case 8: refusals ---------------------------------------------------------------------------------------------------------------
def raw_call(nat, ctx, st, table, rng_out, hit_out, h=None, c_="ctx", n=None, null_args=False, drones=None, grid=None, outside=None, **kw):
    """dsim_range_scan through the raw ABI: table [B, 3] a device tensor of beams used as they are, t in [0.05, 8] and no flags unless kw (fields
    of dsim_scan_args) says otherwise; h the set's handle or None; drones: None, or fields of dsim_camera_drones over grid (range 6,
    outside_out = outside).  Returns the call's status."""
    a = nat.ScanArgs()
    a.beams, a.n_beams, a.t_min, a.t_max, a.flags = table.data_ptr(), table.shape[0], 0.05, 8.0, 0
    a.range_out, a.hit_out = rng_out.data_ptr(), hit_out.data_ptr()
    for k, v in kw.items():
        setattr(a, k, v)
    d = None
    if drones is not None:
        d = nat.CameraDrones()
        d.grid, d.range, d.outside_out = ctypes.addressof(grid), 6.0, outside.data_ptr()
        for k, v in drones.items():
            setattr(d, k, v)
        a.drones = ctypes.addressof(d)
    return ctx.lib.dsim_range_scan(ctx.handle if c_ == "ctx" else c_, ctx.stream_ptr(), st.n if n is None else n, st.view(), h,
                                   None if null_args else ctypes.byref(a))


def test_refusals_leave_the_outputs_untouched(gpu):
    nat, fleet = gpu
    from dronesim_amd.downwash import Downwash
    from dronesim_amd.obstacles import ObstacleScenes
    c = sf.case_main(0)
    types = [params.builtin_type("tello"), params.builtin_type("hexa_6DOF_simple")]
    ctx = fleet.Context(types)
    st = load(fleet, ctx, c["st"][:64])
    dev, cold = c["sc"].to_device(ctx, 1.0).enable_rays(), c["sc"].to_device(ctx, 1.0)       # cold: rays not enabled
    scenes = ObstacleScenes(c["sc"], np.zeros((1, 1, 3)), np.zeros((1, 1, 3))).to_device(ctx, 1.0).enable_rays()
    beams = torch.from_numpy(c["beams"]).to(ctx.device)
    rng_out = torch.full((18, st.n_pad), -7.0, dtype=torch.float32, device=ctx.device)
    hit_out = torch.full((18, st.n_pad), -7, dtype=torch.int32, device=ctx.device)
    sid = torch.zeros((st.n_pad,), dtype=torch.int32, device=ctx.device)
    tid = torch.zeros((st.n_pad,), dtype=torch.uint8, device=ctx.device)
    outside = torch.zeros((1,), dtype=torch.int64, device=ctx.device)
    grid = Downwash(ctx, st, tid, None).sphere_grid(None)
    before = [ctx.query(q) for q in (nat.QUERY_DRONE_CONTACTS, nat.QUERY_OBSTACLE_CONTACTS)]

    def call(h="set", **kw):
        return raw_call(nat, ctx, st, beams, rng_out, hit_out, h=dev.handle if h == "set" else h, grid=grid, outside=outside, **kw)
    inf, nan = float("inf"), float("nan")
    assert call(c_=None) == -1 and call(null_args=True) == -1 and call(beams=None) == -1 and call(range_out=None) == -1
    assert call(n=0) == -1 and call(n=-3) == -1 and call(n=st.n_pad + 1) == -1
    assert call(n_beams=0) == -1 and call(n_beams=65) == -1
    assert call(t_min=-0.1) == -1 and call(t_max=0.05) == -1 and call(t_max=0.01) == -1
    assert call(t_min=nan) == -1 and call(t_max=nan) == -1 and call(t_max=inf) == -1 and call(t_min=inf) == -1
    assert call(flags=4) == -1 and call(flags=1 << 31) == -1
    assert call(h=cold.handle) == -1                           # rays not enabled
    assert call(h=None, scenes=scenes.handle) == -1 and call(h=None, scene_id=sid.data_ptr()) == -1
    assert call(scenes=scenes.handle, scene_id=sid.data_ptr()) == -1              # scenes together with a set
    assert call(h=None) == -1                                  # no world at all
    assert call(h=None, drones={}) == -1                       # several types, drones, no type_id
    assert call(drones={"grid": None}, type_id=tid.data_ptr()) == -1
    assert call(drones={"range": 0.0}, type_id=tid.data_ptr()) == -1 and call(drones={"range": nan}, type_id=tid.data_ptr()) == -1
    plan = nat.HaloPlan()
    grid.halo = ctypes.addressof(plan)
    assert call(drones={}, type_id=tid.data_ptr()) == -5       # a halo plan: DSIM_E_UNSUPPORTED
    grid.halo = None
    ws, grid.workspace = grid.workspace, None
    assert call(drones={}, type_id=tid.data_ptr()) == -1       # what dsim_depth_image_drones refuses about the grid
    grid.workspace = ws
    cell, grid.cell = grid.cell, 0.0
    assert call(drones={}, type_id=tid.data_ptr()) == -1
    grid.cell = cell
    torch.cuda.synchronize()
    assert bool((rng_out == -7.0).all()) and bool((hit_out == -7).all()) and int(outside.item()) == 0
    assert [ctx.query(q) for q in (nat.QUERY_DRONE_CONTACTS, nat.QUERY_OBSTACLE_CONTACTS)] == before
    # and the calls that are in order are served
    assert call() == 0 and call(flags=3) == 0 and call(h=None, flags=1) == 0 and call(drones={}, type_id=tid.data_ptr()) == 0
    assert call(h=None, scenes=scenes.handle, scene_id=sid.data_ptr(), drones={}, type_id=tid.data_ptr()) == 0
    torch.cuda.synchronize()
    assert not bool((rng_out[:, : st.n] == -7.0).any()) and bool((rng_out[:, st.n:] == -7.0).all())
    for d in (dev, cold, scenes):
        d.close()


# ---- case 9: the env ----------------------------------------------------------------------------------------------------------------
def test_the_env_scans_behind_every_step(gpu):
    nat, fleet = gpu
    from dronesim_amd.fleet import Targets
    from dronesim_amd.scanner import RangeScanner
    world = sf.lattice_scene(0)
    kw = dict(range_scan=sf.fan(8, down=True), range_scene=world, range_max=6.0, range_min=0.05, range_see_drones=True)
    env, c = mixed_env(**kw)
    twin, _ = mixed_env()
    assert env.ranges is None and env.range_hits is None
    tg, tg2 = Targets(env.ctx, 256), Targets(twin.ctx, 256)
    for t_ in (tg, tg2):
        t_.set(pos=c["st"][:, :3].astype(np.float64).T, yaw=np.zeros(256))
    for _ in range(3):
        env.step_fused(tg)
        twin.step_fused(tg2)
    torch.cuda.synchronize()
    assert torch.equal(env.state.raw_fields(0, 13), twin.state.raw_fields(0, 13))       # the scan disturbs nothing
    r, h = env.ranges.clone(), env.range_hits.clone()
    assert r.shape == (9, 256) and int((h <= -3).sum()) > 50 and int((h == -2).sum()) > 100
    alone = RangeScanner(env.ctx, env.state, world, kw["range_scan"], 0.05, 6.0, ground=True, type_id=env._type_id, drones=True)
    alone.scan()
    assert torch.equal(alone.ranges, r) and torch.equal(alone.hits, h)
    r2, h2 = env.range_scan()
    assert torch.equal(r2, r) and torch.equal(h2, h)
    # ... and against the reference on the env's own state, in the caller's numbering
    st = env.state.rigid_aos()[:, :7].astype(np.float32)
    ref = sf.scan_brute(st, kw["range_scan"], 0.05, 6.0, world.triangles, world.body, ground=True, radius=c["rad"])
    assert ref["ambiguous"].mean() <= sf.MASK_CAP
    check("the env's scan", r.cpu().numpy().astype(np.float64), h.cpu().numpy(), ref)
    alone.close()
    env.close()
    twin.close()


@pytest.mark.parametrize("see_drones", [False, True])
def test_captured_steps_scan_as_eager_steps_do(gpu, see_drones):
    nat, fleet = gpu
    from dronesim_amd.fleet import Targets
    kw = dict(range_scan=sf.fan(8, down=True), range_scene=sf.lattice_scene(0), range_max=6.0, range_see_drones=see_drones)
    out = []
    for captured in (False, True):
        env, c = mixed_env(**kw)
        tg = Targets(env.ctx, 256)
        tg.set(pos=(c["st"][:, :3].astype(np.float64) + [0.2, 0.0, 0.1]).T, yaw=np.zeros(256))
        if captured:
            graph = env.capture_fused(tg, 4)
            for _ in range(6):
                graph.replay()
        else:
            for _ in range(24):
                env.step_fused(tg)
        torch.cuda.synchronize()
        out.append((env.state.raw_fields(0, 13).clone(), env.ranges.clone(), env.range_hits.clone()))
        env.close()
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert int((out[0][2] != -1).sum()) > 100


def test_the_adaptor_envs_take_the_keywords(gpu):
    from dronesim_amd.envs import VelocityAviary
    n = 64
    xyz = np.stack([np.arange(n) % 8, np.arange(n) // 8, np.full(n, 1.0)], 1).astype(np.float64)
    env = VelocityAviary(["tello"], n, initial_xyzs=xyz, noise_seed=0, dict_io=False, range_scan=sf.fan(4, down=True), range_max=5.0)
    assert env.ranges is None
    env.step(torch.zeros((n, 4), dtype=torch.float32, device=env.ctx.device))
    torch.cuda.synchronize()
    r, h = env.ranges, env.range_hits
    assert r.shape == (5, n) and bool((h[4] == -2).all()) and bool((h[:4] == -1).all())
    assert bool(((r[4] - env.state.pos[2]).abs() < 1e-5).all())          # the altimeter reads the height
    env.close()
