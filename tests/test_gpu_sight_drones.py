"""Line of sight among the drones on the device (dsim_line_of_sight_drones, LineOfSight(drones=True), the env's
neighbor_sight_drones keyword) against the fp64 brute-force reference of tests/sight_drones_ref.py, which walks no grid.
tests/README_sight_drones.md names which test launches which kernel instance.

Outside the reference's ambiguity mask (at most 1 % of a case's cast segments: asserted on the reference alone in
tests/test_sight_drones_cpu.py) visible and blocker are equal EXACTLY and frac is within SIGHT_DRONES_TOL in camera_ref.t_error's
metric (4 x the measured error of the float32 restatement of the kernel's arithmetic).  Every case prefills the outputs with -7 and
checks that lanes >= n kept it, and prints the device's own worst error before it asserts."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest
import torch

from dronesim_amd import params
from tests import camera_ref as cr
from tests import scan_ref as sf
from tests import sight_drones_ref as sd
from tests import sight_ref as sg
from tests.test_gpu_sight import gpu, load, padded, same  # noqa: F401  (gpu: the fixture)

pytestmark = pytest.mark.gpu
TOL = sd.SIGHT_DRONES_TOL
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sight_no_drones.npz")


def mixed_ctx(fleet, zero_type=False):
    """The two-type context of sight_drones_ref.MODELS; zero_type: the first type's collision_sphere is 0."""
    types = [params.builtin_type(m) for m in sd.MODELS]
    if zero_type:
        types[0] = dataclasses.replace(types[0], collision_sphere=0.0)
    return fleet.Context(types)


def type_tensor(ctx, state, types):
    tid = torch.zeros((state.n_pad,), dtype=torch.uint8, device=ctx.device)
    tid[: state.n] = torch.from_numpy(np.asarray(types, dtype=np.uint8)).to(ctx.device)
    return tid


def sight(fleet, c, types, world=None, layout="soa", zero_type=False, **kw):
    """A LineOfSight(drones=True) over a case: the mixed context, the fleet stored in the caller's order with its type_id."""
    from dronesim_amd.sight import LineOfSight
    ctx = mixed_ctx(fleet, zero_type)
    state = load(fleet, ctx, c["pos"], layout)
    los = LineOfSight(ctx, state, world, c["rel"].shape[0], drones=True, type_id=type_tensor(ctx, state, types), **kw)
    assert los.drones and los.args.k == c["rel"].shape[0]
    return los


def query(los, rel, index=None, blocker=True, frac=True):
    """test_gpu_sight.query for a world with drones: one query into outputs prefilled with -7 -> (visible, blocker or None, frac or
    None) [k, n] as numpy (frac float64); lanes >= n kept the prefill, and so did an output that was not asked for.  Among the
    lanes < n a blocker of -7 is drone 4 (DSIM_SEG_DRONE(4)), so that no lane kept the prefill is asked of visible and frac, and
    the blocker is held against the reference."""
    n, n_pad, dev = los.state.n, los.state.n_pad, los.visible_out.device
    los.visible_out.fill_(-7)
    los.blocker_out.fill_(-7)
    los.frac_out.fill_(-7.0)
    rel = padded(rel, n_pad, 1.0, dev)                         # (a valid segment behind n: it must not be cast)
    index = padded(index, n_pad, 1, dev) if index is not None else None
    s = los.query(rel, index, blocker=blocker, frac=frac)
    torch.cuda.synchronize()
    for t, asked, legal in ((los.visible_out, True, False), (los.blocker_out, blocker, True), (los.frac_out, frac, False)):
        assert bool((t[:, n:] == -7).all())
        if not asked:
            assert bool((t == -7).all())
        elif not legal:
            assert not bool((t[:, :n] == -7).any())
    assert (s.blocker is None) == (not blocker) and (s.frac is None) == (not frac)
    return (s.visible.cpu().numpy(), s.blocker.cpu().numpy() if blocker else None,
            s.frac.cpu().numpy().astype(np.float64) if frac else None)


def check(label, got, ref):
    vis, blk, frac = got
    ok = ~ref["ambiguous"]
    assert set(np.unique(vis)) <= {0, 1}
    wrong = int((vis != ref["visible"])[ok].sum())
    wrong_id = int((blk != ref["blocker"])[ok].sum())
    err = sd.t_error(frac, ref)
    print(f"{label}: worst t_error {err:.3e} (tol {TOL:.3e}), {wrong} visible and {wrong_id} blockers differ outside the mask of "
          f"{int(ref['ambiguous'].sum())} of {int(ref['cast'].sum())} cast segments; drones block {int((ref['blocker'] <= -3).sum())}")
    differ = ok & ((vis != ref["visible"]) | (blk != ref["blocker"]))
    for t, i in np.argwhere(differ)[:8]:                       # the first few that differ: (slot, drone, got, reference)
        print(f"  slot {t}, drone {i}: got ({vis[t, i]}, {blk[t, i]}, {frac[t, i]}), "
              f"reference ({ref['visible'][t, i]}, {ref['blocker'][t, i]}, {ref['frac'][t, i]!r})")
    assert wrong == 0 and wrong_id == 0
    assert err <= TOL
    assert np.array_equal(np.isfinite(frac)[ok], np.isfinite(ref["frac"])[ok]) and np.all(frac[~np.isfinite(frac)] == np.inf)
    nc = ~ref["cast"]                                          # a slot that is not cast reads 0 / -1 / +inf, mask or no mask
    assert not vis[nc].any() and np.all(blk[nc] == -1) and np.all(frac[nc] == np.inf)
    n = vis.shape[1]
    assert not (blk == -3 - np.arange(n)[None, :]).any()       # nobody hides a neighbour from itself


# ---- the column of three: drones alone, drones and the plane ---------------------------------------------------------------------------
@pytest.mark.parametrize("ground", [False, True])
def test_a_column_of_three(gpu, ground):
    nat, fleet = gpu
    c = sd.case_column(ground)
    types = [sd.MODELS.index(m) for m in c["models"]]
    los = sight(fleet, c, types, ground=ground)
    got = query(los, c["rel"], c["index"])
    check(f"column, ground {ground}", got, c["ref"])
    vis, blk, frac = got
    R = float(c["rad"][1])
    assert vis[0, 0] == 1 and blk[0, 0] == -1                                   # A -> B: the target is left out
    assert vis[1, 0] == 0 and blk[1, 0] == -3 - 1 and abs(frac[1, 0] - (1.0 - R) / 2.5) <= TOL      # A -> C: B hides C
    assert not vis[:, 3].any() and np.all(frac[:, 3] == 0.0) and np.all(blk[:, 3] == -3 - 1)        # D stands inside B's ball
    if ground:
        assert blk[1, 4] == sg.SEG_GROUND and frac[1, 4] == 0.5
    # the same rel as goal segments: nobody but the drone itself is left out, B hides itself
    ref = sd.sight_drones_brute(c["pos"], c["rel"], None, c["rad"], ground=ground)
    goal = query(los, c["rel"], None)
    check("column, no index", goal, ref)
    assert goal[0][0, 0] == 0 and goal[1][0, 0] == -3 - 1 and abs(goal[2][0, 0] - (1.0 - R)) <= TOL
    assert los.drones_outside() == 0
    los.close()


# ---- the main case: a set and drones, records in LDS and through L2 -------------------------------------------------------------------------
@pytest.mark.parametrize("which, layout", [(0, "soa"), (1, "tile64"), (2, "tile64"), (3, "soa"), (4, "tile64")])
def test_segments_against_the_brute_force_reference(gpu, which, layout):
    nat, fleet = gpu
    from dronesim_amd.downwash import Downwash
    kind, subdiv, offsets = sd.MAIN[which]
    c = sd.case_main(which)
    los = sight(fleet, c, sd.main_types(), c["sc"], layout, offsets=c.get("offsets"))
    assert los.state.n == 300 and los.state.n_pad > 300        # two tiles, the second with 44 live lanes
    rel, index, ref = c["rel"], c["index"], c["ref"]
    if kind != "goal32" and not offsets:
        # the device's own record goes straight in, and the reference is worked out from what it holds
        k = rel.shape[0]
        nb = Downwash(los.ctx, los.state, los._type_id, None).nearest(1.0, k, rel_vel=False)
        rel, index = nb.rel_pos.cpu().numpy(), nb.index.cpu().numpy()
        ref = sd.sight_drones_brute(c["pos"], rel, index, c["rad"], tri=c["tri"], body=c["body"])
        assert sd.mask_share(ref) <= sd.MASK_CAP
    got = query(los, rel, index)
    check(f"main {sd.MAIN[which]}, {layout}", got, ref)
    drones, tris = ref["blocker"] <= -3, ref["blocker"] >= 0
    floors = sd.FLOORS[kind]
    print(f"  drones block {int(drones.sum())}, triangles {int(tris.sum())}, a triangle in front of a drone {int((tris & ref['both']).sum())}, "
          f"a drone in front of a triangle {int((drones & ref['both']).sum())}")
    assert int(drones.sum()) >= floors[0] and int(tris.sum()) >= floors[1]
    assert int((tris & ref["both"]).sum()) >= floors[2] and int((drones & ref["both"]).sum()) >= floors[3]
    if kind != "knn1":                                         # the second tile sees, and is seen
        assert int((got[1][:, 256:] <= -3).sum()) >= 20 and int(((got[1] <= -3) & (-3 - got[1] >= 256)).sum()) >= 20
    if which == 0:
        # one common offset: the fleet stored 64 m away, the world and the balls where they were — bit for bit
        m = sd.common_offset_case(0)
        lo = sight(fleet, m, sd.main_types(), los.set, layout, offsets=m["offsets"])
        idx = index.copy()
        assert same(got, query(lo, rel, idx))
        # ... and without drones the same object's world alone: fewer segments are blocked
        from dronesim_amd.sight import LineOfSight
        plain = query(LineOfSight(los.ctx, los.state, los.set, rel.shape[0]), rel, index)
        assert int(plain[0].sum()) > int(got[0].sum()) and not (plain[1] <= -3).any()
    los.close()


# ---- the walk's edges --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zero_type", [False, True])
@pytest.mark.parametrize("box", ["measured", "pinned"])
def test_the_walk_at_its_edges(gpu, box, zero_type):
    """Level drones in lines: segments with dx = 0, dy = 0 and both, a second and ragged tile, a pinned box that leaves rows on the
    outside list, a drone whose position is not finite, a type of radius 0."""
    nat, fleet = gpu
    c = sd.case_edges(zero_type)
    types = np.arange(300) % 2
    los = sight(fleet, c, types, zero_type=zero_type)
    got = query(los, c["rel"], None)
    assert los.drones_outside() == 0
    if box == "pinned":
        pinned = sight(fleet, c, types, zero_type=zero_type, drone_box=sf.stack_pinned_box())
        gp = query(pinned, c["rel"], None)
        assert pinned.drones_outside() >= 20
        assert same(gp, got)                                   # bit-equal to the measured box's
        got = gp
    check(f"edges, {box} box, zero type {zero_type}", got, c["ref"])
    vis, blk, frac = got
    lost = sd.EDGE_LOST
    assert not vis[:, lost].any() and np.all(blk[:, lost] == -1) and np.all(np.isinf(frac[:, lost])) and not (blk == -3 - lost).any()
    assert int((blk[:, 256:] <= -3).sum()) >= 100 and int(((blk <= -3) & (-3 - blk >= 256)).sum()) >= 100
    if zero_type:
        who = -3 - blk[blk <= -3]
        assert (who % 2 == 1).all() and int((blk[:, 0::2] <= -3).sum()) >= 300      # no tello hides, every tello looks
    # the up segment of a bottom-layer drone on an unshifted column: the drone 0.75 m above it, at 0.75 m less that drone's radius
    i = np.nonzero((np.arange(100) % 5 != 3) & (c["rad"][np.arange(100) + 100] > 0) & (np.arange(100) + 100 != lost))[0]
    want = (0.75 - c["rad"][i + 100].astype(np.float64)) / sd.EDGE_LEN
    assert np.array_equal(blk[4, i], -3 - (i + 100)) and (np.abs(frac[4, i] - want) / want).max() <= TOL


# ---- scenes and drones ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subdiv", [None, 0, 2])
def test_scenes_and_drones(gpu, subdiv):
    nat, fleet = gpu
    c = sd.case_scenes(subdiv)
    n = c["pos"].shape[0]
    los = sight(fleet, c, np.arange(n) % 2, c["scenes"], scene_id=c["scene_id"])
    got = query(los, c["rel"], c["index"])
    check(f"scenes {subdiv}", got, c["ref"])
    assert int((got[1] <= -3).sum()) >= 1000 and int((got[1] >= 0).sum()) >= 30
    los.close()


def test_drones_and_the_plane(gpu):
    nat, fleet = gpu
    c = sd.case_plane()
    los = sight(fleet, c, sd.main_types(), ground=True)
    got = query(los, c["rel"], c["index"])
    check("drones and the plane", got, c["ref"])
    assert int((got[1] == sg.SEG_GROUND).sum()) >= 500 and int((got[1] <= -3).sum()) >= 500
    # blocker_out and frac_out are optional here too
    assert np.array_equal(got[0], query(los, c["rel"], c["index"], blocker=False, frac=False)[0])


# ---- chunks of the slots over blockIdx.y ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, chunks", [(65536, 4), (262144, 1)])
def test_slot_chunks_do_not_change_a_slot(gpu, n, chunks):
    """The main fleet laid out over n drones in copies 64 m apart, each stored with its shift as its offset: drone i reads what drone
    i mod 300 of the small fleet reads — visible and frac bit for bit, the blocker (moved into the copy) outside the reference's
    mask, where an exact tie between two balls goes to whichever the walk meets first."""
    nat, fleet = gpu
    k = sd.CHUNK_K
    tiles = (n + 255) // 256
    want = min(k, -(-1024 // tiles)) if tiles < 1024 else 1
    assert -(-k // -(-k // want)) == chunks                    # the host's rule (dsim_scan.hip: scan_beams_per_block)
    rel, index = sd.chunk_record()
    sc = cr.scene(0)
    small_c = {"pos": sd.main_pos(), "rel": rel}
    los = sight(fleet, small_c, sd.main_types(), sc)
    small = query(los, rel, index)
    ref = sd.sight_drones_brute(sd.main_pos(), rel, index, sd.main_radii(), tri=sc.triangles, body=sc.body)
    check("the small fleet", small, ref)
    pos, off, brel, bindex, j = sd.chunk_layout(n)
    big_los = sight(fleet, {"pos": pos, "rel": brel}, sd.main_types()[j], los.set, offsets=off)
    big = query(big_los, brel, bindex)
    whole = np.arange(n) < (n // 300) * 300                    # (the last, partial copy misses neighbours)
    assert np.array_equal(big[0][:, whole], small[0][:, j][:, whole])
    assert np.array_equal(big[2][:, whole], small[2][:, j][:, whole])
    sb = small[1][:, j]
    moved = np.where(sb <= -3, sb - (np.arange(n) // 300 * 300)[None, :], sb)
    ok = (~ref["ambiguous"])[:, j] & whole[None, :]
    assert np.array_equal(big[1][ok], moved[ok]) and int((big[1] <= -3).sum()) >= n // 2
    los.close()


# ---- without drones: the parent's four instances, bit for bit ------------------------------------------------------------------------------
def golden_cases():
    """(name, case of sight_ref, LineOfSight keywords): set in LDS, set through L2, scenes in LDS, scenes through L2."""
    yield "main0", sg.case_main(0), {}
    yield "main2", sg.case_main(2), {}
    c = sg.case_scenes()
    yield "scenes", c, {"scene_id": c["scene_id"]}
    c = sg.case_lattice_scenes(2)
    yield "lattice2", c, {"scene_id": c["scene_id"]}


def test_without_drones_nothing_changed(gpu):
    """LineOfSight without drones launches the four instances it launched before, and they give what they gave: the outputs of
    the commit before dsim_line_of_sight_drones, recorded on an MI355X (tests/golden/sight_no_drones.npz), bit for bit."""
    nat, fleet = gpu
    from dronesim_amd.sight import LineOfSight
    gold = np.load(GOLDEN)
    for name, c, kw in golden_cases():
        ctx = fleet.Context([params.builtin_type("tello")])
        los = LineOfSight(ctx, load(fleet, ctx, c["pos"]), c.get("sc", c.get("scenes")), c["rel"].shape[0], **kw)
        assert not los.drones
        vis, blk, frac = query(los, c["rel"], c["index"])
        assert np.array_equal(vis, gold[name + "_visible"]), name
        assert np.array_equal(blk, gold[name + "_blocker"]), name
        assert np.array_equal(frac.astype(np.float32).view(np.uint32), gold[name + "_frac"].view(np.uint32)), name
        assert int((blk >= 0).sum()) >= 20
        los.close()


# ---- the env --------------------------------------------------------------------------------------------------------------------------------
def host(s):
    return (s.visible.cpu().numpy(), s.blocker.cpu().numpy(), s.frac.cpu().numpy().astype(np.float64))


@pytest.mark.parametrize("gate", [False, True])
def test_env_in_the_callers_numbering(gpu, gate):
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.sight import LineOfSight
    sc = cr.scene(0)
    pos = sf.draw_fleet(171, 300, lo=sg.BOX_LO, hi=sg.BOX_HI)[:, :3].astype(np.float64)
    n, k, R = pos.shape[0], 8, 1.0
    tid = (np.arange(n) % 8 == 0).astype(np.uint8)             # a hexa, seven tellos, a hexa, ...: stored type-major
    models = ["tello", "hexa_6DOF"]
    rad = np.array([params.builtin_type(models[t]).collision_sphere for t in tid], dtype=np.float32)
    assert rad.min() > 0.0
    kw = dict(initial_xyzs=pos, type_ids=tid, dict_io=False, noise_seed=0, neighbor_obs=k, neighbor_radius=R, neighbor_sight=True,
              neighbor_sight_drones=True)
    if gate:
        kw["obstacle_watch"] = sc
    env = CtrlAviary(models, n, **kw)
    assert env.order is not None and env.last_neighbor_sight is None and env._sight.drones
    assert (env._sight.set is env._obst) if gate else (env._sight.set is None)
    world = dict(tri=sc.triangles, body=sc.body) if gate else {}

    def check_env(nb, s, what, floor):
        p32 = env.state.rigid_aos()[:, 0:3].astype(np.float32)                      # (the caller's numbering)
        rel, index = nb.rel_pos.cpu().numpy(), nb.index.cpu().numpy()
        ref = sd.sight_drones_brute(p32, rel, index, rad, **world)
        assert sd.mask_share(ref) <= sd.MASK_CAP and int((ref["blocker"] <= -3).sum()) >= floor
        check(what, host(s), ref)
        who = LineOfSight.seg_drone(s.blocker).cpu().numpy()
        assert np.array_equal(who >= 0, ref["blocker"] <= -3) and who.max() >= 256

    nb, s = env.neighbor_sight()
    check_env(nb, s, f"env on demand, gate {gate}", 100)
    assert env.last_neighbor_sight is None and env.last_neighbors is None        # (an on-demand query is not a step)
    nb3, s3 = env.neighbor_sight(k=3, radius=2.0)
    assert tuple(s3.visible.shape) == (3, n)
    check_env(nb3, s3, "env on demand, k = 3", 10)
    assert env._sight_demand[3]._targets is env._sight._targets and env._sight_demand[k]._targets is env._sight._targets
    env.step(torch.zeros((n, env.n_act), dtype=torch.float32, device=env.ctx.device))
    check_env(env.last_neighbors, env.last_neighbor_sight, "env behind step()", 100)
    last = host(env.last_neighbor_sight)
    env.neighbor_sight()                                                         # ... leaves last_* alone
    env.neighbor_sight(k=3, radius=2.0)
    assert same(last, host(env.last_neighbor_sight))
    assert env._sight.drones_outside() == 0
    env.close()


# ---- refusals through the raw ABI ------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(gpu):
    nat, fleet = gpu
    c = sd.case_column(False)
    types = [sd.MODELS.index(m) for m in c["models"]]
    los = sight(fleet, c, types)
    ctx, state = los.ctx, los.state
    rel, index = padded(c["rel"], state.n_pad, 1.0, ctx.device), padded(c["index"], state.n_pad, 1, ctx.device)
    good = query(los, c["rel"], c["index"])                                      # (fills the args; the call works)
    a = los.args
    a.rel, a.index = rel.data_ptr(), index.data_ptr()
    a.blocker_out, a.frac_out = los.blocker_out.data_ptr(), los.frac_out.data_ptr()
    for t in (los.visible_out, los.blocker_out):
        t.fill_(-7)
    los.frac_out.fill_(-7.0)
    los._targets.grid_args()
    dr_ok = los._targets.dr
    call = lambda tid, drones: ctx.lib.dsim_line_of_sight_drones(ctx.handle, ctx.stream_ptr(), state.n, state.view(), None,
                                                                 ctypes.byref(a), tid, drones)
    tid = los._type_id.data_ptr()
    assert call(tid, None) == -1                                                 # null drones
    assert call(None, ctypes.byref(dr_ok)) == -1                                 # two types and no type_id
    for bad in (0.0, -1.0, float("nan")):
        dr_bad = nat.CameraDrones()
        ctypes.memmove(ctypes.byref(dr_bad), ctypes.byref(dr_ok), ctypes.sizeof(dr_ok))
        dr_bad.range = bad
        assert call(tid, ctypes.byref(dr_bad)) == -1, bad                        # a range that is not positive
    dr_bad = nat.CameraDrones()
    ctypes.memmove(ctypes.byref(dr_bad), ctypes.byref(dr_ok), ctypes.sizeof(dr_ok))
    dr_bad.grid = None
    assert call(tid, ctypes.byref(dr_bad)) == -1                                 # no grid
    torch.cuda.synchronize()
    assert bool((los.visible_out == -7).all()) and bool((los.blocker_out == -7).all()) and bool((los.frac_out == -7.0).all())
    assert call(tid, ctypes.byref(dr_ok)) == 0                                   # ... and the same call with everything in place runs
    torch.cuda.synchronize()
    n = state.n
    assert np.array_equal(los.visible_out[:, :n].cpu().numpy(), good[0]) and np.array_equal(los.blocker_out[:, :n].cpu().numpy(), good[1])
    los.close()
