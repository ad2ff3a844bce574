"""Line of sight on the device (dsim_line_of_sight, LineOfSight, the env's neighbor_sight keyword) against the fp64 brute-force reference
of tests/sight_ref.py, which walks no grid.  tests/README_sight.md.

Outside the reference's ambiguity mask (at most 1 % of a case's cast segments: asserted on the reference alone in
tests/test_sight_cpu.py) visible and blocker are equal EXACTLY and frac is within SIGHT_TOL in camera_ref.t_error's metric (4 x the
measured error of the float32 restatement of the kernel's arithmetic).  Every case prefills the outputs with -7 and checks that lanes
>= n kept it, and prints the device's own worst error before it asserts."""
import numpy as np
import pytest
import torch

from dronesim_amd import params
from tests import camera_ref as cr
from tests import scan_ref as sf
from tests import sight_ref as sg
from tests.util import random_fleet

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product has no CPU fallback")
    from dronesim_amd import _native as nat
    from dronesim_amd import fleet
    return nat, fleet


def load(fleet, ctx, pos, layout="soa"):
    """A fleet state with the positions pos [n, 3] float32 (stored in the caller's order)."""
    n = pos.shape[0]
    state = fleet.FleetState(ctx, n, layout)
    rigid, mem, _ = random_fleet(np.random.default_rng(5), n, n_act=ctx.n_act)
    rigid[:, 0:3] = pos
    state.load_aos(rigid, mem)
    return state


def tello_ctx(fleet):
    return fleet.Context([params.builtin_type("tello")])


def padded(a, n_pad, fill, dev):
    """[..., n] numpy -> the contiguous device tensor [..., n_pad], `fill` behind n."""
    t = torch.full(a.shape[:-1] + (n_pad,), fill, dtype=torch.from_numpy(a[..., :1].copy()).dtype)
    t[..., : a.shape[-1]] = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(dev)


def query(los, rel, index=None, blocker=True, frac=True, raw=False):
    """One query into outputs prefilled with -7: (visible, blocker or None, frac or None) [k, n] as numpy (frac float64); lanes
    >= n kept the prefill, and so did an output that was not asked for."""
    n, n_pad, dev = los.state.n, los.state.n_pad, los.visible_out.device
    los.visible_out.fill_(-7)
    los.blocker_out.fill_(-7)
    los.frac_out.fill_(-7.0)
    if not raw:
        rel = padded(rel, n_pad, 1.0, dev)                     # (a valid segment behind n: it must not be cast)
        index = padded(index, n_pad, 1, dev) if index is not None else None
    s = los.query(rel, index, blocker=blocker, frac=frac)
    torch.cuda.synchronize()
    for t, asked in ((los.visible_out, True), (los.blocker_out, blocker), (los.frac_out, frac)):
        assert bool((t[:, n:] == -7).all())
        assert not bool((t[:, :n] == -7).any()) if asked else bool((t == -7).all())
    assert (s.blocker is None) == (not blocker) and (s.frac is None) == (not frac)
    return (s.visible.cpu().numpy(), s.blocker.cpu().numpy() if blocker else None,
            s.frac.cpu().numpy().astype(np.float64) if frac else None)


def check(label, got, ref):
    vis, blk, frac = got
    ok = ~ref["ambiguous"]
    assert set(np.unique(vis)) <= {0, 1}
    wrong = int((vis != ref["visible"])[ok].sum())
    wrong_id = int((blk != ref["blocker"])[ok].sum()) if blk is not None else 0
    err = cr.t_error(frac, ref) if frac is not None else 0.0
    print(f"{label}: worst t_error {err:.3e} (tol {sg.SIGHT_TOL:.3e}), {wrong} visible and {wrong_id} blockers differ outside the mask of "
          f"{int(ref['ambiguous'].sum())} of {int(ref['cast'].sum())} cast segments")
    differ = ok & ((vis != ref["visible"]) | ((blk != ref["blocker"]) if blk is not None else False))
    for t, i in np.argwhere(differ)[:8]:                       # the first few that differ: (slot, drone, got, reference)
        print(f"  slot {t}, drone {i}: got ({vis[t, i]}, {blk[t, i] if blk is not None else None}, {frac[t, i] if frac is not None else None}), "
              f"reference ({ref['visible'][t, i]}, {ref['blocker'][t, i]}, {ref['frac'][t, i]!r})")
    assert wrong == 0 and wrong_id == 0
    assert err <= sg.SIGHT_TOL
    if frac is not None:
        assert np.array_equal(np.isfinite(frac)[ok], np.isfinite(ref["frac"])[ok]) and np.all(frac[~np.isfinite(frac)] == np.inf)
        assert np.array_equal(np.isfinite(frac), vis == 0) or not ref["cast"].all()
    # a slot that is not cast reads 0 / -1 / +inf, mask or no mask
    nc = ~ref["cast"]
    assert not vis[nc].any() and (blk is None or np.all(blk[nc] == -1)) and (frac is None or np.all(frac[nc] == np.inf))


def same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


# ---- case 1: the set in LDS, the records through L2 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which, layout", [(0, "soa"), (1, "tile64"), (2, "soa")])
def test_segments_against_the_brute_force_reference(gpu, which, layout):
    nat, fleet = gpu
    from dronesim_amd.sight import LineOfSight
    c = sg.case_main(which)
    subdiv, k, _, _, floor = sg.MAIN[which]
    blocked = c["ref"]["blocker"] >= 0
    assert int(blocked.sum()) >= floor and set(np.unique(c["ref"]["blocker"][blocked])) == {0, 1}
    ctx = tello_ctx(fleet)
    state = load(fleet, ctx, c["pos"], layout)
    assert state.n_pad > state.n or subdiv == 2                # n = 300 leaves dead lanes
    los = LineOfSight(ctx, state, c["sc"], k)
    got = query(los, c["rel"], c["index"])
    check(f"scene({subdiv}), k {k}, {layout}", got, c["ref"])
    assert np.array_equal(los.query(padded(c["rel"], state.n_pad, 1.0, ctx.device)).mask().cpu().numpy().astype(np.int64) & 0xFFFFFFFF,
                          (got[0].astype(np.int64) << np.arange(k)[:, None]).sum(0))
    # without blocker_out / frac_out, and without an index (every slot of this case is used): the same answers
    v2 = query(los, c["rel"], c["index"], blocker=False, frac=False)
    assert np.array_equal(got[0], v2[0])
    assert same(got, query(los, c["rel"], None))
    assert same(got[:2], query(los, c["rel"], c["index"], frac=False)[:2])
    # case 4, offsets that are multiples of 1/4 m: p + offset is exact, and the query is bit-identical
    off = sf.quarter_offsets(7, c["pos"].shape[0])
    moved = (c["pos"].astype(np.float64) + off).astype(np.float32)
    assert np.array_equal(moved - off.astype(np.float32), c["pos"])
    lo = LineOfSight(ctx, load(fleet, ctx, moved, layout), los.set, k, offsets=off)
    assert same(got, query(lo, c["rel"], c["index"]))
    los.close()


# ---- case 2: a real knn record -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_a_knn_record_goes_straight_in(gpu, which):
    nat, fleet = gpu
    from dronesim_amd.downwash import Downwash
    from dronesim_amd.sight import LineOfSight
    radius, k = sg.KNN[which]
    c = sg.case_knn(which)
    if which == 0:
        assert int((c["index"] < 0).sum()) >= 10               # sparse drones: unused slots are among them
    ctx = tello_ctx(fleet)
    state = load(fleet, ctx, c["pos"])
    nb = Downwash(ctx, state, None, None).nearest(radius, k, rel_vel=False)
    los = LineOfSight(ctx, state, c["sc"], k)
    for t in (los.visible_out, los.blocker_out):
        t.fill_(-7)
    los.frac_out.fill_(-7.0)
    s = los.query_neighbors(nb)
    torch.cuda.synchronize()
    assert bool((los.visible_out[:, state.n:] == -7).all()) and bool((los.frac_out[:, state.n:] == -7).all())
    rel, index = nb.rel_pos.cpu().numpy(), nb.index.cpu().numpy()
    if which == 0:
        assert int((index < 0).sum()) >= 10                    # ... in the device's own record too
    ref = sg.sight_brute(c["pos"], rel, index, c["tri"], c["body"])
    assert sg.mask_share(ref) <= sg.MASK_CAP
    check(f"knn record, radius {radius}, k {k}", (s.visible.cpu().numpy(), s.blocker.cpu().numpy(), s.frac.cpu().numpy().astype(np.float64)), ref)
    unused = index < 0
    assert not s.visible.cpu().numpy()[unused].any() and np.all(s.frac.cpu().numpy()[unused] == np.inf)
    los.close()


# ---- case 3: edges ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subdiv", [0, 2])
def test_edges(gpu, subdiv):
    """Axis segments from cell planes and faces, the wall's two sides, segments outside the box, and every kind of slot that is
    not cast: nothing faults, and those slots read 0 / -1 / +inf."""
    nat, fleet = gpu
    from dronesim_amd.sight import LineOfSight
    c = sg.case_edges(subdiv)
    ctx = tello_ctx(fleet)
    los = LineOfSight(ctx, load(fleet, ctx, c["pos"]), c["sc"], sg.EDGE_K)
    got = query(los, c["rel"], c["index"])
    check(f"edges, scene({subdiv})", got, c["ref"])
    assert int((~c["ref"]["cast"]).sum()) >= 30
    los.close()


# ---- case 5: scenes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["scenes", "lattice", "lattice2"])
def test_scenes_against_the_placed_reference(gpu, name):
    nat, fleet = gpu
    from dronesim_amd.sight import LineOfSight
    c = {"scenes": sg.case_scenes, "lattice": lambda: sg.case_lattice_scenes(0), "lattice2": lambda: sg.case_lattice_scenes(2)}[name]()
    ctx = tello_ctx(fleet)
    los = LineOfSight(ctx, load(fleet, ctx, c["pos"]), c["scenes"], 8, scene_id=c["scene_id"])
    got = query(los, c["rel"], c["index"])
    check(name, got, c["ref"])
    sid = np.asarray(c["scene_id"])
    none = (sid < 0) | (sid >= c["scenes"].K)
    assert none.sum() >= 50 and got[0][:, none].all() and np.all(got[1][:, none] == -1)
    los.close()


@pytest.mark.parametrize("which", [0, 2])
def test_identity_placement_is_the_unplaced_query(gpu, which):
    """The two PLACED instances against their unplaced siblings: one placement at the origin, unrotated — bit for bit."""
    nat, fleet = gpu
    from dronesim_amd.sight import LineOfSight
    c = sg.case_main(which)
    k = sg.MAIN[which][1]
    ctx = tello_ctx(fleet)
    state = load(fleet, ctx, c["pos"])
    plain = LineOfSight(ctx, state, c["sc"], k)
    placed = LineOfSight(ctx, state, sg.identity_scenes(c["subdiv"]), k, scene_id=np.zeros(c["pos"].shape[0], dtype=np.int64))
    a, b = query(plain, c["rel"], c["index"]), query(placed, c["rel"], c["index"])
    assert int((a[1] >= 0).sum()) >= sg.MAIN[which][4] and same(a, b)
    plain.close()
    placed.close()


# ---- case 6: the ground -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_set", [True, False])
def test_the_plane_hides_what_lies_below_it(gpu, with_set):
    nat, fleet = gpu
    from dronesim_amd.sight import LineOfSight
    c = sg.case_ground(with_set)
    ctx = tello_ctx(fleet)
    los = LineOfSight(ctx, load(fleet, ctx, c["pos"]), c["sc"] if with_set else None, 8, ground=True)
    got = query(los, c["rel"])
    check(f"ground, set {with_set}", got, c["ref"])
    below = c["below"]
    assert not got[0][below].any() and not (got[1][~below] == sg.SEG_GROUND).any()
    if not with_set:
        assert np.all(got[1][below] == sg.SEG_GROUND) and got[0][~below].all()
    los.close()


# ---- case 7: chunks of the slots over blockIdx.y -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, chunks", [(65536, 4), (262144, 1)])
def test_slot_chunks_do_not_change_a_slot(gpu, n, chunks):
    """A small fleet spreads chunks of the slots over blockIdx.y (300 drones: one slot per workgroup); 65 536 drones cast the 8
    slots in chunks of 2, and from 262 144 drones on a workgroup casts them all.  The fleet is case 1's 300 drones over and over:
    drone i reads, bit for bit, what drone i mod 300 of the small fleet reads."""
    nat, fleet = gpu
    from dronesim_amd.sight import LineOfSight
    c = sg.case_main(0)
    k = 8
    ctx = tello_ctx(fleet)
    dev = c["sc"].to_device(ctx, 1.0)
    small = query(LineOfSight(ctx, load(fleet, ctx, c["pos"]), dev, k), c["rel"], c["index"])
    tiles = (n + 255) // 256
    want = min(k, -(-1024 // tiles)) if tiles < 1024 else 1
    assert -(-k // -(-k // want)) == chunks                    # the host's rule (dsim_scan.hip: scan_beams_per_block)
    idx = np.arange(n) % 300
    big = query(LineOfSight(ctx, load(fleet, ctx, c["pos"][idx]), dev, k), c["rel"][:, :, idx], c["index"][:, idx])
    assert same(tuple(x[:, idx] for x in small), big)
    dev.close()


# ---- case 8: the env ----------------------------------------------------------------------------------------------------------------------
def host(s):
    return (s.visible.cpu().numpy(), s.blocker.cpu().numpy(), s.frac.cpu().numpy().astype(np.float64))


def test_env_in_the_callers_numbering(gpu):
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.fleet import Targets
    sc = cr.scene(0)
    pos = sf.draw_fleet(171, 300, lo=sg.BOX_LO, hi=sg.BOX_HI)[:, :3].astype(np.float64)
    n, k, R = pos.shape[0], 8, 3.0
    tid = (np.arange(n) % 2).astype(np.uint8)                  # tello, hexa, tello, ...: handed over interleaved
    kw = dict(initial_xyzs=pos, type_ids=tid, dict_io=False, noise_seed=0, neighbor_obs=k, neighbor_radius=R, obstacle_watch=sc)
    env = CtrlAviary(["tello", "hexa_6DOF"], n, neighbor_sight=True, **kw)
    twin = CtrlAviary(["tello", "hexa_6DOF"], n, **kw)
    assert env.order is not None and env.last_neighbor_sight is None and env._sight.set is env._obst
    assert twin._sight is None and twin.last_neighbor_sight is None

    def check_env(nb, s, what, floor=30):
        # (the record holds the NEAREST drones, half a metre away in this crowd: few of its segments are cut, the floor says some are)
        p32 = env.state.rigid_aos()[:, 0:3].astype(np.float32)                      # (the caller's numbering)
        rel, index = nb.rel_pos.cpu().numpy(), nb.index.cpu().numpy()
        ref = sg.sight_brute(p32, rel, index, sc.triangles, sc.body)
        assert sg.mask_share(ref) <= sg.MASK_CAP and int((ref["blocker"] >= 0).sum()) >= floor
        check(what, host(s), ref)

    nb, s = env.neighbor_sight()
    check_env(nb, s, "env on demand")
    assert env.last_neighbor_sight is None and env.last_neighbors is None        # (an on-demand query is not a step)
    nb3, s3 = env.neighbor_sight(k=3, radius=2.0)
    assert tuple(s3.visible.shape) == (3, n)
    check_env(nb3, s3, "env on demand, k = 3", 3)
    for e in (env, twin):
        e.step(torch.zeros((n, e.n_act), dtype=torch.float32, device=e.ctx.device))
    check_env(env.last_neighbors, env.last_neighbor_sight, "env behind step()")
    last = host(env.last_neighbor_sight)
    env.neighbor_sight()                                                         # ... leaves last_* alone
    env.neighbor_sight(k=3, radius=2.0)
    assert same(last, host(env.last_neighbor_sight))
    for e in (env, twin):
        tg = Targets(e.ctx, n)
        tg.set(pos=pos.astype(np.float32).astype(np.float64).T, yaw=0.0)
        e.step_fused(tg, n_steps=3)
    check_env(env.last_neighbors, env.last_neighbor_sight, "env behind step_fused(n_steps=3)")
    # the twin without the keyword flew the same states and saw the same neighbours
    torch.cuda.synchronize()
    assert np.array_equal(env.state.rigid_aos(), twin.state.rigid_aos()) and np.array_equal(env.state.mem_aos(), twin.state.mem_aos())
    for a, b in zip(env.last_neighbors, twin.last_neighbors):
        assert torch.equal(a, b)
    with pytest.raises(NotImplementedError):
        env.capture_fused(tg, 2)
    env.close()
    twin.close()


def test_env_on_scenes(gpu):
    from dronesim_amd.envs import CtrlAviary
    scenes = sf.lattice_scenes(0)
    pos = sf.lattice()[0][:, :3].astype(np.float64)
    n = pos.shape[0]
    env = CtrlAviary(["tello"], n, initial_xyzs=pos, dict_io=False, noise_seed=0, neighbor_obs=8, neighbor_radius=3.0,
                     neighbor_sight=True, neighbor_sight_scene=scenes, obstacle_scene_id=sf.LATTICE_SCENE_ID)
    env.step(torch.zeros((n, env.n_act), dtype=torch.float32, device=env.ctx.device))
    nb, s = env.last_neighbors, env.last_neighbor_sight
    p32 = env.state.rigid_aos()[:, 0:3].astype(np.float32)
    ref = sg.sight_brute(p32, nb.rel_pos.cpu().numpy(), nb.index.cpu().numpy(), scenes=scenes, scene_id=sf.LATTICE_SCENE_ID)
    assert sg.mask_share(ref) <= sg.MASK_CAP and int((ref["blocker"] >= 0).sum()) >= 5       # (nearest neighbours: few are hidden, some are)
    check("env on scenes", host(s), ref)
    env.close()
    # off by default: nothing behind a step
    env = CtrlAviary(["tello"], 4, initial_xyzs=pos[:4], dict_io=False, noise_seed=0, neighbor_obs=2, neighbor_radius=1.0)
    env.step(torch.zeros((4, 4), dtype=torch.float32, device=env.ctx.device))
    assert env.last_neighbor_sight is None and env._sight is None
    with pytest.raises(ValueError):
        env.neighbor_sight()
    env.close()
