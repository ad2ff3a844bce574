"""GPU tests of the obstacle witness (dsim_obstacle_witness, dsim_obstacle_witness_scenes, obstacles.witness / witness_scenes,
CtrlAviary(obstacle_witness=...)) against the fp64 reference of tests/witness_ref.py.

Three things are asked of a witness (tests/README_witness.md): it lies ON the triangle it names (TOL_ON), it is near-OPTIMAL
(| |rel| - d_ref | and, without any reference, | |rel| - (clearance + R) | within TOL_OPT), and its POSITION is the reference's
outside a tie mask computed on the reference alone (2 (2 sqrt(2 d E) + E)) and, outside the strict mask, within TOL_POS.  The
tolerances are 4 x the float32 restatement's recorded errors; the masks' caps are asserted on the reference by
tests/test_witness_cpu.py.  clearance, nearest and the counters are the point watch's bit for bit.  Every case prints the device's
own worst figures before it asserts."""
import ctypes

import numpy as np
import pytest
import torch

from dronesim_amd import params
from tests import scenes_ref as sr
from tests import witness_ref as wr
from tests.test_gpu_obstacles import _gate_fleet, _gate_world, _mixed_types, load, many_tiles_far, soa3
from tests.test_gpu_scenes import ids_tensor
from tests.util import f32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product has no CPU fallback")
    from dronesim_amd import _native as nat
    from dronesim_amd import fleet
    return nat, fleet


def run(ctx, st, dev, margin, off=None, tid=None, counter=None, ids=None, body=False, triangle=True):
    """-> clearance, nearest, rel [3, n_pad], triangle over the whole padded length, filled with sentinels first."""
    from dronesim_amd import obstacles as obs
    clr = torch.full((st.n_pad,), -7.0, dtype=torch.float32, device=ctx.device)
    near = torch.full((st.n_pad,), -7, dtype=torch.int32, device=ctx.device)
    rel = torch.full((3, st.n_pad), -7.0, dtype=torch.float32, device=ctx.device)
    tri = torch.full((st.n_pad,), -7, dtype=torch.int32, device=ctx.device) if triangle else None
    if ids is None:
        obs.witness(ctx, st, dev, margin, clr, near, rel, tri, off, tid, counter, body_frame=body)
    else:
        obs.witness_scenes(ctx, st, dev, ids, margin, clr, near, rel, tri, off, tid, counter, body_frame=body)
    return clr, near, rel, tri


def check(got, ref, rad, what, obst=None, scenes=None, scene_id=None, sure=None, pos_everywhere=False):
    """The three properties over the first n lanes of `got` (clearance, nearest, rel [3, .], triangle) against a reference dict.
    sure: the drones whose in / out status the reference decides (all, for inputs drawn by the input rule)."""
    n = len(ref["in"])
    clr, near, rel = (x[..., :n].cpu().numpy() for x in got[:3])
    named = got[3] is not None                  # (the env hands out no triangles: no on-surface check there)
    tri = got[3][:n].cpu().numpy() if named else np.where(near >= 0, ref["tri"], -1)
    rel = rel.T.astype(np.float64)
    sure = np.ones(n, bool) if sure is None else sure
    has = near >= 0
    np.testing.assert_array_equal(has[sure], ref["in"][sure])
    assert np.all(rel[~has] == 0.0) and np.all(tri[~has] == -1) and np.all(tri[has] >= 0)
    both = has & ref["in"]
    proto = obst if scenes is None else scenes.prototype
    T, nb = proto.n_tri, proto.n_bodies
    if named:
        np.testing.assert_array_equal(near[has], (tri[has] // T) * nb + proto.body[tri[has] % T])  # the triangle is of the body
    on, opt, pos, ratio = wr.errors(rel, np.where(both, tri, 0), dict(ref, **{"in": both}), obst, scenes, scene_id)
    on = on if named else 0.0
    r = np.asarray(rad, dtype=np.float32).astype(np.float64)
    inv = float(np.abs(np.linalg.norm(rel[has], axis=1) - (clr[has].astype(np.float64) + r[has])).max(initial=0.0))
    tie, strict = wr.mask_shares(ref)
    print(f"witness {what}: on-surface {on:.3e} (TOL_ON {wr.TOL_ON:.3e}), | |rel| - d_ref | {opt:.3e}, | |rel| - (c + R) | {inv:.3e} "
          f"(TOL_OPT {wr.TOL_OPT:.3e}), position outside the strict mask {pos:.3e} (TOL_POS {wr.TOL_POS:.3e}), position / tie bound "
          f"{ratio:.3f}; {int(both.sum())} with a witness of {n}, tie mask {tie:.4f}, strict mask {strict:.4f}")
    assert tie <= wr.TIE_CAP and strict <= wr.STRICT_CAP
    assert on <= wr.TOL_ON and opt <= wr.TOL_OPT and inv <= wr.TOL_OPT and ratio <= 1.0 and pos <= wr.TOL_POS
    if pos_everywhere:
        assert not ref["strict"].any() and not ref["tie"].any()
    np.testing.assert_allclose(clr.astype(np.float64)[sure], ref["clr"][sure], rtol=0, atol=wr.TOL_OPT)
    return both


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 1. one triangle: every region, both sides -----------------------------------------------------------------------------------
def test_one_triangle_every_region(gpu):
    nat, fleet = gpu
    from dronesim_amd.obstacles import watch_reach
    from tests.obstacle_ref import region
    d = wr.case_one_triangle()
    s, ref, margin = d["set"], d["ref"], d["margin"]
    reg, side = region(d["pos"].astype(np.float64), s.triangles[0])
    for k in range(7):
        for sg in (-1.0, 1.0):
            assert ((reg == k) & (side == sg) & ref["in"]).sum() >= 3, (k, sg)
    ctx = fleet.Context([params.builtin_type("robobee")])
    dev = s.to_device(ctx, watch_reach(ctx.types, margin))
    st = load(fleet, ctx, d["pos"])
    got = run(ctx, st, dev, margin)
    check(got, ref, d["rad"], "one triangle", obst=s, pos_everywhere=True)      # (no rivals: TOL_POS holds for every drone)
    assert ctx.query(nat.QUERY_OBSTACLE_CONTACTS) == ref["contacts"] > 10
    dev.close()
    ctx.close()


# ---- 2. identity with the point watch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["soa", "tile64"])
def test_clearance_nearest_and_counter_are_the_point_watch_bit_for_bit(gpu, layout):
    """The gate, 700 robobees (three tiles, the last partial, n < n_pad), one position NaN."""
    nat, fleet = gpu
    from dronesim_amd import obstacles as obs
    d = wr.case_gate(False)
    s, n, margin = d["set"], 700, d["margin"]
    ctx = fleet.Context([params.builtin_type("robobee")])
    dev = s.to_device(ctx, obs.watch_reach(ctx.types, margin))
    st = load(fleet, ctx, d["pos"], layout)
    assert st.n_pad > n
    nan_at = 333
    p = torch.from_numpy(np.ascontiguousarray(d["pos"].T)).clone()
    p[0, nan_at] = float("nan")
    st.set_fields(0, p)
    want_clr = torch.full((st.n_pad,), -7.0, dtype=torch.float32, device=ctx.device)
    want_near = torch.full((st.n_pad,), -7, dtype=torch.int32, device=ctx.device)
    c0, c1 = (torch.zeros((1,), dtype=torch.int64, device=ctx.device) for _ in range(2))
    obs.query(ctx, st, dev, margin, want_clr, want_near, None, None, c0)
    before = ctx.query(nat.QUERY_OBSTACLE_CONTACTS)
    clr, near, rel, tri = run(ctx, st, dev, margin, counter=c1)
    assert same_bits(clr, want_clr) and torch.equal(near, want_near)
    assert int(c1.item()) == int(c0.item()) == ctx.query(nat.QUERY_OBSTACLE_CONTACTS) - before > 50
    none = near[:n] < 0
    assert int(none.sum()) >= 1 and int(near[nan_at]) == -1 and float(clr[nan_at]) == np.float32(margin)
    assert bool((rel[:, :n][:, none] == 0.0).all()) and bool((tri[:n][none] == -1).all()) and bool((tri[:n][~none] >= 0).all())
    assert bool((clr[n:] == -7.0).all()) and bool((near[n:] == -7).all()) and bool((rel[:, n:] == -7.0).all()) and bool((tri[n:] == -7).all())
    # without triangle_out: the same answers
    clr2, near2, rel2, _ = run(ctx, st, dev, margin, triangle=False)
    assert same_bits(clr2, clr) and torch.equal(near2, near) and same_bits(rel2, rel)
    dev.close()
    ctx.close()


# ---- 3. the gate with offsets of +-128 m: the LDS instance ---------------------------------------------------------------------------
@pytest.mark.parametrize("offsets", [False, True])
def test_gate_vs_bruteforce(gpu, offsets):
    nat, fleet = gpu
    from dronesim_amd.obstacles import watch_reach
    d = wr.case_gate(offsets)
    s, ref, margin = d["set"], d["ref"], d["margin"]
    assert s.n_tri <= 512 and ref["contacts"] > 50
    ctx = fleet.Context([params.builtin_type("robobee")])
    dev = s.to_device(ctx, watch_reach(ctx.types, margin))
    for layout in ("soa", "tile64"):
        st = load(fleet, ctx, d["pos"], layout)
        before = ctx.query(nat.QUERY_OBSTACLE_CONTACTS)
        got = run(ctx, st, dev, margin, soa3(d["off"], st.n_pad, ctx.device) if offsets else None)
        check(got, ref, d["rad"], f"gate {layout} offsets={offsets}", obst=s)
        assert ctx.query(nat.QUERY_OBSTACLE_CONTACTS) - before == ref["contacts"]
    dev.close()
    ctx.close()


# ---- 4. the soup: the L2 instance ----------------------------------------------------------------------------------------------------
def test_soup_four_bodies_records_through_l2(gpu):
    nat, fleet = gpu
    from dronesim_amd.obstacles import watch_reach
    d = wr.case_soup()
    s, ref, margin = d["set"], d["ref"], d["margin"]
    assert s.n_tri > 512 and set(ref["near"][ref["in"]]) == set(range(4)) and not ref["in"][768:].any()
    ctx = fleet.Context([params.builtin_type("hexa_6DOF")])
    dev = s.to_device(ctx, watch_reach(ctx.types, margin))
    st = load(fleet, ctx, d["pos"])
    got = run(ctx, st, dev, margin)
    check(got, ref, d["rad"], "soup", obst=s)
    assert ctx.query(nat.QUERY_OBSTACLE_CONTACTS) == ref["contacts"] > 10
    dev.close()
    ctx.close()


@pytest.mark.parametrize("placed", [False, True])
def test_soup_is_the_point_watch_bit_for_bit_records_through_l2(gpu, placed):
    """Case 2's identity on the instances that read the records through L2 (the 3 000-triangle soup): case 4's inputs unplaced,
    scenes_ref.case_soup (512 drones, K = 4, G = 2) placed.  The witness is the point watch's kernel with a tail, and this is
    the check that the tail changes nothing in front of it."""
    nat, fleet = gpu
    from dronesim_amd import obstacles as obs
    d = sr.case_soup() if placed else wr.case_soup()
    world, margin, n = d["scenes"] if placed else d["set"], d["margin"], len(d["pos"])
    assert (world.prototype if placed else world).n_tri > 512
    ctx = fleet.Context([params.builtin_type("hexa_6DOF")])
    dev = world.to_device(ctx, obs.watch_reach(ctx.types, margin))
    st = load(fleet, ctx, d["pos"])
    ids = ids_tensor(d["scene_id"], st.n_pad, ctx.device) if placed else None
    want_clr = torch.full((st.n_pad,), -7.0, dtype=torch.float32, device=ctx.device)
    want_near = torch.full((st.n_pad,), -7, dtype=torch.int32, device=ctx.device)
    c0, c1 = (torch.zeros((1,), dtype=torch.int64, device=ctx.device) for _ in range(2))
    if placed:
        obs.query_scenes(ctx, st, dev, ids, margin, want_clr, want_near, None, None, c0)
    else:
        obs.query(ctx, st, dev, margin, want_clr, want_near, None, None, c0)
    clr, near, rel, tri = run(ctx, st, dev, margin, counter=c1, ids=ids)
    none = near[:n] < 0
    print(f"soup through L2 placed={placed}: {int((~none).sum())} of {n} with a witness, {int(c1.item())} contacts")
    assert same_bits(clr, want_clr) and torch.equal(near, want_near) and int(c1.item()) == int(c0.item())
    assert int((~none).sum()) >= int((d["ref"]["near"] >= 0).sum()) // 2 > 0 and int(none.sum()) > 0
    assert bool((rel[:, :n][:, none] == 0.0).all()) and bool((rel[:, :n][:, ~none] != 0.0).any(0).all())
    assert bool((tri[:n][none] == -1).all()) and bool((tri[:n][~none] >= 0).all())
    dev.close()
    ctx.close()


# ---- 5. scenes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,offsets,model", [("gates", False, "robobee"), ("gates", True, "robobee"), ("ragged", True, "robobee"),
                                                ("soup", False, "hexa_6DOF")])
def test_scenes_vs_bruteforce(gpu, name, offsets, model):
    """case_gates with and without offsets (the placed LDS instance), case_ragged (an empty scene and ids out of range give
    zeros), case_soup (the placed L2 instance): the cases of tests/scenes_ref.py."""
    nat, fleet = gpu
    from dronesim_amd.obstacles import watch_reach
    d, ref = wr.scene_ref(name, offsets)
    scenes, sid, margin, n = d["scenes"], d["scene_id"], d["margin"], len(d["scene_id"])
    ctx = fleet.Context([params.builtin_type(model)])
    dev = scenes.to_device(ctx, watch_reach(ctx.types, margin))
    st = load(fleet, ctx, d["pos"])
    off = soa3(d["off"], st.n_pad, ctx.device) if d["off"] is not None else None
    cnt = torch.zeros((1,), dtype=torch.int64, device=ctx.device)
    got = run(ctx, st, dev, margin, off, None, cnt, ids=ids_tensor(sid, st.n_pad, ctx.device))
    both = check(got, ref, d["rad"], f"scenes {name} offsets={offsets}", scenes=scenes, scene_id=sid)
    assert int(cnt.item()) == ref["contacts"] == d["ref"]["contacts"] == ctx.query(nat.QUERY_OBSTACLE_CONTACTS)
    tri = got[3][:n].cpu().numpy()
    if name == "gates":
        assert len(set(tri[both] // scenes.prototype.n_tri)) == 3                       # every slot holds somebody's witness
    if name == "ragged":
        none = (sid < 1) | (sid >= 5)
        rel = got[2][:, :n].cpu().numpy()
        assert none.sum() > 50 and np.all(rel[:, none] == 0.0) and np.all(tri[none] == -1)
    dev.close()
    ctx.close()


def test_identity_scene_is_the_unplaced_witness(gpu):
    """K = 1, G = 1, R = I, t = 0: every product with 0 and 1 is exact, so the placed call gives the unplaced call's bits
    (rel compared as numbers: 1 x + 0 y + 0 z turns a -0.0 into +0.0)."""
    nat, fleet = gpu
    from dronesim_amd import obstacles as obs
    d = wr.case_gate(False)
    s, margin = d["set"], d["margin"]
    ctx = fleet.Context([params.builtin_type("robobee")])
    scenes = obs.ObstacleScenes(s, np.zeros((1, 1, 3)), np.zeros((1, 1, 3)))
    dev = scenes.to_device(ctx, obs.watch_reach(ctx.types, margin))
    st = load(fleet, ctx, d["pos"])
    a = run(ctx, st, dev.set, margin)
    b = run(ctx, st, dev, margin, ids=ids_tensor(np.zeros(700, dtype=int), st.n_pad, ctx.device))
    assert same_bits(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    assert int((a[1] >= 0).sum()) > 300
    dev.close()
    ctx.close()


# ---- 6. the body frame ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placed", [False, True])
def test_body_frame_is_the_world_vector_through_the_attitude(gpu, placed):
    """Random attitudes (tests.util.random_fleet: tilts of +-0.5 rad, any yaw).  rel_body against R(quat)^T rel_world in fp64 on
    the device's own world vector.  The bar: every entry of the float32 R carries at most 4 roundings, a component is a three-term
    sum of products with 3 more, so a component errs by at most 15 x 2^-24 |rel| and the vector by sqrt(3) times that; |rel| <=
    margin + R."""
    nat, fleet = gpu
    from dronesim_amd.obstacles import watch_reach
    if placed:
        d, _ = wr.scene_ref("gates", True)
        world, ids_np, model = d["scenes"], d["scene_id"], "robobee"
    else:
        d = wr.case_gate(True)
        world, ids_np, model = d["set"], None, "robobee"
    margin, n = d["margin"], len(d["pos"])
    ctx = fleet.Context([params.builtin_type(model)])
    dev = world.to_device(ctx, watch_reach(ctx.types, margin))
    for layout in ("soa", "tile64"):
        st = load(fleet, ctx, d["pos"], layout)
        ids = ids_tensor(ids_np, st.n_pad, ctx.device) if placed else None
        off = soa3(d["off"], st.n_pad, ctx.device)
        w = run(ctx, st, dev, margin, off, ids=ids)
        b = run(ctx, st, dev, margin, off, ids=ids, body=True)
        assert same_bits(w[0], b[0]) and torch.equal(w[1], b[1]) and torch.equal(w[3], b[3])
        quat = st.rigid_aos()[:, 3:7].astype(np.float32)
        Rq = wr.body_rotation(quat)
        rw, rb = (x[2][:, :n].cpu().numpy().T.astype(np.float64) for x in (w, b))
        want = np.einsum("nji,nj->ni", Rq, rw)
        has = w[1][:n].cpu().numpy() >= 0
        bar = np.sqrt(3.0) * 15.0 * 2.0 ** -24 * (margin + float(d["rad"].max()))
        err = float(np.linalg.norm(rb - want, axis=1).max())
        nrm = float(np.abs(np.linalg.norm(rb, axis=1) - np.linalg.norm(rw, axis=1)).max())
        print(f"body frame placed={placed} {layout}: |rel_body - R^T rel_world| {err:.3e}, norms differ by {nrm:.3e} (bar {bar:.3e})")
        assert has.sum() > n // 5 and np.all(rb[~has] == 0.0)
        assert np.abs(rb - rw)[has].max() > 0.05                                    # (it is another frame)
        assert err <= bar and nrm <= bar
    dev.close()
    ctx.close()


# ---- 7 / 8. the env ------------------------------------------------------------------------------------------------------------------
def _positions(env):
    return env.state.pos.T.cpu().numpy().astype(np.float32)


def test_env_mixed_fleet_with_an_invisible_type_in_caller_numbering(gpu):
    """Robobee, tello, hexa and a type of R = 0 interleaved (type-major storage), K = 8 scenes of 3 gates, a frame per drone."""
    nat, _ = gpu
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.obstacles import ObstacleScenes
    n, K, margin = 96, 8, 0.5
    types = _mixed_types()
    tid = (np.arange(n) % 4).astype(np.uint8)
    rad = np.array([np.float32(t.collision_sphere) for t in types])[tid]
    ppos, prpy = sr.random_placements(np.random.default_rng(51), K, 3)
    scenes = ObstacleScenes(sr.gate(), ppos, prpy)
    sid = (np.arange(n) * 5 + 3) % K
    side = int(np.ceil(np.sqrt(n)))
    off = np.stack([np.arange(n) % side, np.arange(n) // side, np.zeros(n)], 1).astype(np.float64) * 8.0
    off32 = f32(off)

    def draw(rng, idx):
        q = scenes.position[sid[idx], rng.integers(0, 3, len(idx))] + rng.uniform(-0.8, 0.8, (len(idx), 3))
        return f32(q + off[idx]), off32[idx].copy()
    decide = lambda p, o: (sr.brute_scenes(p, scenes, sid, rad, margin, o)["raw"], margin)
    pos, _, frac = sr.settle(np.random.default_rng(52), draw, n, decide)
    assert frac <= 0.02
    rpy = np.tile(np.array([0.0, 0.0, np.pi / 2]), (n, 1))                       # every drone yawed a quarter turn
    env = CtrlAviary(types, n, initial_xyzs=pos.astype(np.float64), initial_rpys=rpy, type_ids=tid, storage="auto",
                     obstacle_watch=scenes, obstacle_margin=margin, obstacle_offsets=off, obstacle_scene_id=sid,
                     obstacle_witness="world", dict_io=False, noise_seed=0)
    assert env.order is not None and not np.array_equal(env.order.drone_np, np.arange(n))
    assert np.array_equal(_positions(env), pos) and env.last_obstacle_witness is None
    ref = wr.brute_witness_scenes(pos, scenes, sid, rad, margin, off32)
    assert ref["contacts"] >= 3 and ref["in"].sum() > n // 4 and not ref["in"][rad == 0].any()
    clr, near, rel = env.obstacle_witness()
    assert rel.shape == (3, n)
    c2, n2 = env.obstacle_clearance()
    assert same_bits(clr, c2) and torch.equal(near, n2)
    check((clr, near, rel, None), ref, rad, "env, type-major storage", scenes=scenes, scene_id=sid)
    assert bool((rel[:, torch.from_numpy(rad == 0).to(rel.device)] == 0.0).all())
    assert int(env._obst_on_demand.item()) == 2 * ref["contacts"] and env.obstacle_contacts() == 0
    # negative control: ids left in the caller's order would hand drone d the id of drone slot[d]
    wrong = wr.brute_witness_scenes(pos, scenes, sid[env.order.slot_np], rad, margin, off32)
    assert (sid[env.order.slot_np] != sid).sum() > n // 2
    with pytest.raises(AssertionError):
        check((clr, near, rel, None), wrong, rad,
              "env, ids in the caller's order (must fail)", scenes=scenes, scene_id=sid[env.order.slot_np])
    # the body frame on demand: at a yaw of a quarter turn R^T (x, y, z) = (y, -x, z); the bar of the body-frame case
    _, _, rel_b = env.obstacle_witness(frame="body")
    bar = np.sqrt(3.0) * 15.0 * 2.0 ** -24 * (margin + float(rad.max()))
    want = torch.stack([rel[1], -rel[0], rel[2]])
    print(f"env, body frame at yaw pi / 2: |rel_body - (y, -x, z)| {float((rel_b - want).norm(dim=0).max()):.3e} (bar {bar:.3e})")
    assert float((rel_b - want).norm(dim=0).max()) <= bar and float((rel_b - rel).abs().max()) > 0.1
    env.close()


def _flown_sure(ref, rad, margin):
    """A flown state cannot be re-drawn: the in / out status is compared where the reference's clearance is not within TOL_OPT of
    the margin."""
    raw = ref["d"] - np.asarray(rad, dtype=np.float64)
    return ~(np.abs(raw - margin) < wr.TOL_OPT)


def test_env_last_witness_after_ten_steps_and_contacts_unchanged(gpu):
    nat, _ = gpu
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.fleet import Targets
    n, margin = 512, 1.0
    s, xyz, off = _gate_fleet(n)
    kw = dict(initial_xyzs=xyz, obstacle_watch=s, obstacle_margin=margin, obstacle_offsets=off, dict_io=False, noise_seed=0)
    env, plain = CtrlAviary(["robobee"], n, obstacle_witness="world", **kw), CtrlAviary(["robobee"], n, **kw)
    assert env.last_obstacle_witness is None and env.last_obstacle_clearance is None and plain.last_obstacle_witness is None
    rad = np.full(n, np.float32(env.ctx.types[0].collision_sphere))
    for e in (env, plain):
        tg = Targets(e.ctx, n)
        tg.set(pos=f32(xyz).T, yaw=0.0)
        for _ in range(10):
            e.step_fused(tg)
    assert torch.equal(env.state.fields(0, 13), plain.state.fields(0, 13))
    assert env.obstacle_contacts() == plain.obstacle_contacts() > 10 * (n // 20)
    (c0, n0), (c1, n1) = env.last_obstacle_clearance, plain.last_obstacle_clearance
    assert same_bits(c0, c1) and torch.equal(n0, n1)
    rel = env.last_obstacle_witness
    assert rel.shape == (3, n)
    ref = wr.brute_witness(_positions(env), s, rad, margin, f32(off))
    check((c0, n0, rel, None), ref, rad, "env after 10 steps", obst=s, sure=_flown_sure(ref, rad, margin))
    # on demand: the same answer, not an Env.step, counted where on-demand queries count
    before = env.obstacle_contacts()
    c2, n2, r2 = env.obstacle_witness()
    assert same_bits(c2, c0) and torch.equal(n2, n0) and same_bits(r2, rel) and env.obstacle_contacts() == before
    assert int(env._obst_on_demand.item()) == int((c0 < 0).sum())
    with pytest.raises(ValueError, match="frame"):
        env.obstacle_witness(frame="wind")
    env.close()
    plain.close()


def test_env_eager_vs_captured_replay(gpu):
    nat, _ = gpu
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.fleet import Targets
    n, margin = 256, 1.0
    s, xyz, off = _gate_fleet(n, seed=43)
    envs, tgts = [], []
    for _ in range(2):
        e = CtrlAviary(["robobee"], n, initial_xyzs=xyz, obstacle_watch=s, obstacle_margin=margin, obstacle_offsets=off,
                       obstacle_witness="body", dict_io=False, noise_seed=0)
        tg = Targets(e.ctx, n)
        tg.set(pos=f32(xyz).T, yaw=0.0)
        envs.append(e)
        tgts.append(tg)
    for _ in range(4):
        envs[0].step_fused(tgts[0])
    g = envs[1].capture_fused(tgts[1], 4)
    g.replay()
    torch.cuda.synchronize()
    assert envs[0]._env_steps == envs[1]._env_steps == 4
    assert torch.equal(envs[0].state.fields(0, 13), envs[1].state.fields(0, 13))
    a, b = envs[0].obstacle_contacts(), envs[1].obstacle_contacts()
    assert a == b > 4 * (n // 20), (a, b)
    (c0, n0), (c1, n1) = envs[0].last_obstacle_clearance, envs[1].last_obstacle_clearance
    r0, r1 = envs[0].last_obstacle_witness, envs[1].last_obstacle_witness
    assert same_bits(c0, c1) and torch.equal(n0, n1) and same_bits(r0, r1) and int((n1 >= 0).sum()) > n // 4
    assert float(r1.abs().max()) > 0.1
    for e in envs:
        e.close()


# ---- 9. more tiles than workgroups ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placed", [False, True])
def test_many_tiles_per_workgroup(gpu, placed):
    """2 049 tiles on 2 048 workgroups: workgroup 0 walks tiles 0 and 2 048.  Everybody stands far off but tile 1 and tile 2 048.
    Identity with the point watch and the reference-free invariant only."""
    nat, fleet = gpu
    from dronesim_amd import obstacles as obs
    n, margin = 2049 * 256, 1.0
    near_ix = np.concatenate([np.arange(256, 512), np.arange(2048 * 256, n)])
    t = params.builtin_type("robobee")
    s, rad, p_near, _ = _gate_world(len(near_ix), margin, [t], np.zeros(len(near_ix), dtype=int), False, 71)
    pos = many_tiles_far(np.random.default_rng(72), n)
    pos[near_ix] = p_near
    ctx = fleet.Context([t])
    if placed:
        dev = obs.ObstacleScenes(s, np.zeros((2, 2, 3)), np.array([[[0, 0, 0], [0, 0, np.pi / 2]]] * 2)).to_device(
            ctx, obs.watch_reach(ctx.types, margin))
    else:
        dev = s.to_device(ctx, obs.watch_reach(ctx.types, margin))
    st = load(fleet, ctx, pos)
    ids = ids_tensor(np.arange(n) % 2, st.n_pad, ctx.device) if placed else None
    want_clr = torch.full((st.n_pad,), -7.0, dtype=torch.float32, device=ctx.device)
    want_near = torch.full((st.n_pad,), -7, dtype=torch.int32, device=ctx.device)
    c0, c1 = (torch.zeros((1,), dtype=torch.int64, device=ctx.device) for _ in range(2))
    if placed:
        obs.query_scenes(ctx, st, dev, ids, margin, want_clr, want_near, None, None, c0)
    else:
        obs.query(ctx, st, dev, margin, want_clr, want_near, None, None, c0)
    clr, near, rel, tri = run(ctx, st, dev, margin, counter=c1, ids=ids)
    assert same_bits(clr, want_clr) and torch.equal(near, want_near) and int(c0.item()) == int(c1.item()) > 20
    has = (near >= 0).cpu().numpy()
    ix = np.zeros(st.n_pad, bool)
    ix[near_ix] = True
    assert not has[~ix].any() and has[256:512].sum() > 50 and has[2048 * 256:n].sum() > 50
    rel_, tri_ = rel.cpu().numpy(), tri.cpu().numpy()
    assert np.all(rel_[:, :n][:, ~has[:n]] == 0.0) and np.all(tri_[:n][~has[:n]] == -1)
    inv = np.abs(np.linalg.norm(rel_[:, has].astype(np.float64), axis=0) - (clr.cpu().numpy()[has].astype(np.float64) + float(rad[0])))
    print(f"many tiles placed={placed}: | |rel| - (c + R) | {inv.max():.3e} over {int(has.sum())} drones (TOL_OPT {wr.TOL_OPT:.3e})")
    assert inv.max() <= wr.TOL_OPT
    dev.close()
    ctx.close()


# ---- 10. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(gpu):
    nat, fleet = gpu
    from dronesim_amd.obstacles import ObstacleScenes, watch_reach
    ctx = fleet.Context([params.builtin_type("robobee")])
    margin = 0.5
    scenes = ObstacleScenes(sr.gate(), np.zeros((2, 2, 3)), np.zeros((2, 2, 3)))
    dev = scenes.to_device(ctx, watch_reach(ctx.types, margin))
    st = load(fleet, ctx, f32(np.zeros((64, 3))))
    clr = torch.full((st.n_pad,), -7.0, dtype=torch.float32, device=ctx.device)
    near = torch.full((st.n_pad,), -7, dtype=torch.int32, device=ctx.device)
    rel = torch.full((3, st.n_pad), -7.0, dtype=torch.float32, device=ctx.device)
    tri = torch.full((st.n_pad,), -7, dtype=torch.int32, device=ctx.device)
    cnt = torch.zeros((1,), dtype=torch.int64, device=ctx.device)
    ids = ids_tensor(np.zeros(64, dtype=int), st.n_pad, ctx.device)

    def calls(m, flags=0, rel_ptr=rel.data_ptr(), clr_ptr=clr.data_ptr()):
        a = nat.WitnessArgs(None, None, m, flags, clr_ptr, near.data_ptr(), rel_ptr, tri.data_ptr(), cnt.data_ptr())
        return (ctx.lib.dsim_obstacle_witness(ctx.handle, ctx.stream_ptr(), st.n, st.view(), dev.set.handle, ctypes.byref(a)),
                ctx.lib.dsim_obstacle_witness_scenes(ctx.handle, ctx.stream_ptr(), st.n, st.view(), dev.handle, ids.data_ptr(),
                                                     ctypes.byref(a)))
    assert calls(margin, rel_ptr=None) == (-1, -1)                     # a null rel_out
    assert calls(margin, flags=2) == (-1, -1) and calls(margin, flags=-1) == (-1, -1)      # an unknown flag
    assert calls(margin * 1.01) == (-1, -1)                            # R_max + margin > reach of the set
    assert calls(0.0) == (-1, -1) and calls(float("nan")) == (-1, -1) and calls(margin, clr_ptr=None) == (-1, -1)
    a = nat.WitnessArgs(None, None, margin, 0, clr.data_ptr(), near.data_ptr(), rel.data_ptr(), tri.data_ptr(), cnt.data_ptr())
    assert ctx.lib.dsim_obstacle_witness(ctx.handle, ctx.stream_ptr(), st.n, st.view(), dev.set.handle, None) == -1
    assert ctx.lib.dsim_obstacle_witness_scenes(ctx.handle, ctx.stream_ptr(), st.n, st.view(), None, ids.data_ptr(), ctypes.byref(a)) == -1
    assert ctx.lib.dsim_obstacle_witness_scenes(ctx.handle, ctx.stream_ptr(), st.n, st.view(), dev.handle, None, ctypes.byref(a)) == -1
    torch.cuda.synchronize()
    assert bool((clr == -7.0).all()) and bool((near == -7).all()) and bool((rel == -7.0).all()) and bool((tri == -7).all())
    assert int(cnt.item()) == 0 and ctx.query(nat.QUERY_OBSTACLE_CONTACTS) == 0
    assert calls(margin) == (0, 0) and calls(0.25, flags=nat.WITNESS_BODY_FRAME) == (0, 0)
    torch.cuda.synchronize()
    assert bool((clr[:64] != -7.0).all())
    dev.close()
    ctx.close()
