"""GPU tests of the velocity safety filter (dsim_velocity_filter, avoid.VelocityFilter, CtrlAviary(velocity_filter=...),
VelocityAviary.step_velocity) against the fp64 brute-force reference of tests/filter_ref.py on the records and the state as read
back.  Four assertions per case (tests/README_filter.md): the kept set is the reference's outside the decision mask; v meets every
kept row within the bar, for all drones; |v - u| <= |v_ref - u| + bar, for all drones; |v - v_ref|_inf <= bar outside the value
mask.  The masks' caps are asserted on the reference before the kernel's answer is looked at.

Measured on an MI355X (bar 5.32e-05 = 4 x the float32 figure 1.33e-05): see the table in tests/README_filter.md."""
import numpy as np
import pytest
import torch

from dronesim_amd import params
from tests import filter_ref as fr
from tests import scenes_ref as sr
from tests.util import f32, random_fleet

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product has no CPU fallback")
    from dronesim_amd import _native as nat
    from dronesim_amd import fleet
    return nat, fleet


@pytest.fixture(scope="module")
def tello(gpu):
    nat, fleet = gpu
    ctx = fleet.Context([params.builtin_type("tello")])
    yield ctx, float(np.float32(ctx.types[0].collision_sphere))
    ctx.close()


def load(fleet, ctx, pos, vel):
    n = pos.shape[0]
    st = fleet.FleetState(ctx, n, "soa")
    rigid, mem, _ = random_fleet(np.random.default_rng(5), n, n_act=ctx.n_act)
    rigid[:, 0:3] = pos.astype(np.float32).astype(np.float64)      # (not through f32(): a planted NaN stays one)
    rigid[:, 7:10] = vel.astype(np.float32).astype(np.float64)
    st.load_aos(rigid, mem)
    return st


def held(st):
    r = st.rigid_aos()
    return r[:, 0:3].astype(np.float32), r[:, 7:10].astype(np.float32)


def padded(a, n_pad, dev, fill=0):
    """[..., n] numpy -> [..., n_pad] device tensor, `fill` beyond n."""
    out = np.full(a.shape[:-1] + (n_pad,), fill, dtype=a.dtype)
    out[..., : a.shape[-1]] = a
    return torch.from_numpy(out).to(dev)


def records(case, n_pad, dev, vel=True):
    from dronesim_amd.downwash import Neighbors
    from dronesim_amd.obstacles import ObstacleWitnesses
    nb = wit = None
    if case.get("nb") is not None:
        i, d, rp, rv = case["nb"]
        nb = Neighbors(padded(i, n_pad, dev, -1), padded(d, n_pad, dev, np.inf), padded(rp, n_pad, dev), padded(rv, n_pad, dev), None)
    if case.get("wit") is not None:
        c, b, r, v = case["wit"]
        wit = ObstacleWitnesses(padded(c, n_pad, dev), padded(b, n_pad, dev, -1), padded(r, n_pad, dev),
                                padded(v, n_pad, dev) if (vel and v is not None) else None, None)
    return nb, wit


def run_case(gpu, ctx, case, what, caps=(fr.DECISION_CAP, fr.VALUE_CAP), vel=True, out=None):
    """The case's records through VelocityFilter.apply on a fresh state; the reference on what the device holds; the four assertions.
    -> (Filtered on the host, Ref, the filter)."""
    nat, fleet = gpu
    from dronesim_amd.avoid import VelocityFilter
    st = load(fleet, ctx, case["pos"], case["vel"])
    p32, v32 = held(st)
    if not vel and case.get("wit") is not None:
        case = dict(case, wit=case["wit"][:3] + (None,))
    ref = fr.case_ref(case, pos=p32, vel=v32)
    decision, value = ref.shares()
    assert decision <= caps[0] and value <= caps[1], (what, decision, value)          # on the reference alone, before the kernel
    assert np.abs(ref.v[np.isfinite(ref.u).all(1)]).max() <= fr.V_CAP, what           # ... and so is the cap on how far a vertex may run
    f = VelocityFilter(ctx, st, fr.ALPHA, fr.BUF_D, fr.BUF_O, fr.SHARE, floor=case.get("floor"))
    nb, wit = records(case, st.n_pad, ctx.device, vel)
    u = padded(np.ascontiguousarray(case["u"].T), st.n_pad, ctx.device)
    got = f.apply(u, nb, wit, out=out)
    assert got.vel.shape == (3, st.n) and got.dropped.shape == (st.n,) and got.dropped.dtype == torch.int32
    v, dropped = got.vel.cpu().numpy().T, got.dropped.cpu().numpy()
    ref.check(v, dropped, what=what)
    # the two bit-exact guarantees, wherever they apply, and the counters
    same = (ref.v == ref.u).all(1) & ~ref.decision
    assert np.array_equal(v[same].view(np.uint32), case["u"][same].view(np.uint32))
    changed, lost = f.counters()
    sane = np.isfinite(case["u"]).all(1)
    assert changed == int((v[sane] != case["u"][sane]).any(1).sum()) and lost == int((dropped != 0).sum())
    return (v, dropped), ref, f


# ---- 1. / 2. random rows: nine of them, and the full width -----------------------------------------------------------------------------
@pytest.mark.parametrize("spec", fr.RANDOM_CASES, ids=lambda s: f"{s[0]}-{s[4]}")
def test_random_rows(gpu, tello, spec):
    ctx, rad = tello
    case = fr.random_case(*spec, rad=rad)
    assert case["n"] == 320 and (case["k"], case["m"]) in ((6, 3), (16, 8))
    (v, dropped), ref, f = run_case(gpu, ctx, case, case["name"])
    assert ref.valid.sum(1).max() == (25 if spec[0] == "full" else 9)
    assert (np.abs(ref.v - ref.u).max(1) > 0).mean() > 0.5 and (ref.dropped != 0).any()
    # again: deterministic, and the counters add up
    before = f.counters()
    nb, wit = records(case, f.state.n_pad, ctx.device)
    again = f.apply(padded(np.ascontiguousarray(case["u"].T), f.state.n_pad, ctx.device), nb, wit)
    assert np.array_equal(again.vel.cpu().numpy().T.view(np.uint32), v.view(np.uint32)) and np.array_equal(again.dropped.cpu().numpy(), dropped)
    assert f.counters() == (2 * before[0], 2 * before[1])


# ---- 4. bit-exact pass-through ------------------------------------------------------------------------------------------------------------
def test_pass_through_is_bit_exact(gpu, tello):
    ctx, rad = tello
    from dronesim_amd.avoid import Filtered
    case = fr.random_case(*fr.RANDOM_CASES[0], rad=rad)
    n = case["n"]
    # no rows at all: every slot unused
    i, d, rp, rv = case["nb"]
    c, b, r, wv = case["wit"]
    empty = dict(case, nb=(np.full_like(i, -1), d, rp, rv), wit=(c, np.full_like(b, -1), r, wv))
    sent = Filtered(torch.full((3, 512), -7.0, device=ctx.device), torch.full((512,), -7, dtype=torch.int32, device=ctx.device))
    (v, dropped), ref, f = run_case(gpu, ctx, empty, "no rows", out=sent)
    assert not ref.valid.any() and np.array_equal(v.view(np.uint32), case["u"].view(np.uint32)) and not dropped.any()
    assert f.counters() == (0, 0)
    assert bool((sent.vel[:, n:] == -7.0).all()) and bool((sent.dropped[n:] == -7).all())          # lanes i >= n are not written
    # rows all met by u: every obstacle far enough and receding, every neighbour far away
    rng = np.random.default_rng(31)
    a = rng.normal(size=(n, 3))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    rad_n = case["rad"]
    one_w = fr.synth_witness(rng, a, np.full(n, -50.0), rad_n)
    one_n = fr.synth_neighbor(rng, a, np.full(n, -50.0), case["vel"].astype(np.float64), rad_n, rad_n)
    met = dict(case, wit=tuple(np.stack([one_w[q]] * 3) for q in range(4)), nb=tuple(np.stack([one_n[q]] * 6) for q in range(4)))
    (v, dropped), ref, f = run_case(gpu, ctx, met, "rows all met")
    assert ref.valid.sum() == 9 * n and np.array_equal(v.view(np.uint32), case["u"].view(np.uint32)) and not dropped.any()
    assert f.counters() == (0, 0)


# ---- 5. squeezed drones -------------------------------------------------------------------------------------------------------------------
def test_squeezed_drones_drop_what_the_reference_drops(gpu, tello):
    ctx, rad = tello
    case = fr.squeezed_case(rad=rad)
    (v, dropped), ref, _ = run_case(gpu, ctx, case, "squeezed", caps=(fr.GEO_DECISION_CAP, fr.GEO_VALUE_CAP))
    keep = ~ref.decision
    assert np.array_equal(dropped[keep], ref.dropped[keep])
    four, tilted = np.arange(case["n"]) % 4 == 0, np.arange(case["n"]) % 2 == 1
    assert not (dropped & 0b0011).any() and np.all(dropped & 0b0100)                 # the floor and slot 0 stay, the opposed slot 1 goes
    assert np.array_equal((dropped & 0b1000) != 0, four)                              # the floor wins over the obstacle above
    assert np.array_equal((dropped >> fr.NB_BIT) & 1 == 1, tilted)                    # obstacle rows win over the neighbour row


# ---- 6. edges -----------------------------------------------------------------------------------------------------------------------------
def _planted(base, rad):
    """The edges planted into a random case's records, u and positions (whatever of the two records it has)."""
    n = base["n"]
    u, pos = base["u"].copy(), base["pos"].copy()
    case = dict(base)
    if base.get("nb") is not None:
        i, d, rp, rv = (x.copy() for x in base["nb"])
        i[0, 0:40] = -1                                          # unused neighbour slots, in the first slot of all
        i[3, 10:50] = n + 5                                      # ... and an index beyond the fleet
        d[2, 60:80] = 0.0                                        # a slot at no distance
        rp[2, :, 60:80] = 0.0
        rv[4, 1, 90:100] = np.nan                                # a non-finite entry
        case["nb"] = (i, d, rp, rv)
    if base.get("wit") is not None:
        c, b, r, wv = (x.copy() for x in base["wit"])
        b[1, 20:60] = -1                                         # unused obstacle slots
        c[0, 80:90] = -np.float32(rad)                           # an obstacle point at the centre
        c[2, 100:110] = np.inf
        case["wit"] = (c, b, r, wv)
    u[120, 1] = np.nan                                           # a NaN in u
    u[121, 0] = np.inf
    pos[200, 2] = np.nan                                         # a NaN position in a drone with every slot filled
    return dict(case, u=u, pos=pos)


def test_edges_read_as_the_contract_says(gpu, tello):
    ctx, rad = tello
    case = _planted(fr.random_case(*fr.RANDOM_CASES[0], rad=rad), rad)
    u, busiest = case["u"], 200
    (v, dropped), ref, _ = run_case(gpu, ctx, case, "edges")
    assert not ref.valid[busiest].any() and not ref.valid[120].any() and not ref.valid[:40, fr.NB_BIT].any()
    assert not ref.valid[10:50, fr.NB_BIT + 3].any() and not ref.valid[60:80, fr.NB_BIT + 2].any() and not ref.valid[80:90, fr.OBST_BIT].any()
    assert not ref.valid[20:60, fr.OBST_BIT + 1].any() and not ref.valid[90:100, fr.NB_BIT + 4].any() and not ref.valid[100:110, fr.OBST_BIT + 2].any()
    for lost in (120, 121, busiest):
        assert np.array_equal(v[lost].view(np.uint32), u[lost].view(np.uint32)) and dropped[lost] == 0
    # k = 0 with m > 0, the reverse (a case of neighbour rows alone), and a null vel
    run_case(gpu, ctx, dict(case, nb=None, k=0), "edges, m alone")
    (vk, dk), refk, _ = run_case(gpu, ctx, _planted(fr.random_case(*fr.K_ALONE, rad=rad), rad), "edges, k alone")
    assert not refk.valid[:, :fr.NB_BIT].any() and refk.valid[:, fr.NB_BIT:].sum() > 5 * 300
    (v0, _), ref0, _ = run_case(gpu, ctx, case, "edges, static world", vel=False)
    assert np.abs(ref0.b - ref.b).max() > 0.1                     # (the obstacles' velocities were part of the rows)


# ---- 3. geometry: the env's own records -----------------------------------------------------------------------------------------------------
def _env_rows(env, u, rad, nb, wit, opts):
    """The reference on the records and the state read back, everything in the caller's numbering."""
    h = lambda t: None if t is None else t.cpu().numpy()
    pos, vel = h(env.state.pos).T, h(env.state.vel).T
    nbr = None if nb is None else (h(nb.index), h(nb.dist), h(nb.rel_pos), h(nb.rel_vel))
    wr = None if wit is None else (h(wit.clearance), h(wit.body), h(wit.rel), h(wit.vel))
    A, b, valid = fr.build_rows(pos, vel, u, rad, rad, opts["alpha"], opts.get("share", 0.5), opts.get("buffer_drone", 0.0),
                                opts.get("buffer_obstacle", 0.0), opts.get("floor"), None, nbr, wr)
    return fr.Ref(A, b, valid, u)


@pytest.mark.parametrize("mixed", [False, True], ids=["robobees", "type-major"])
def test_env_crowd_around_the_moving_gates(gpu, mixed):
    """A CtrlAviary crowd about the committed gate on moving scenes, neighbor_obs = 6 and obstacle_witnesses = 3 with their
    velocities, a few steps: filter_velocity(u) against the reference on the records and the state read back, in the caller's
    numbering; with two types of different bounding sphere in type-major storage R_j goes through the index."""
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.fleet import Targets
    from tests import witness_velocity_ref as vr
    d, motion = vr.moving_case("gates")
    n = 320
    rng = np.random.default_rng(61)
    sid = d["scene_id"][:n]
    # a crowd: every drone about its own scene's gates, the scenes' frames 1.5 m apart on a 4 x 4 grid of one world, so that the drones
    # are each other's neighbours (all frames on one spot put drones of different scenes inside each other: 2 % must drop rows, and
    # the reference's masks stand at 0.6 % and 3.4 %, over the caps)
    group = sid % 16
    off = np.stack([(group % 4) * 1.5, (group // 4) * 1.5, np.zeros(n)], 1)
    pos = d["pos"][:n].astype(np.float64) + off
    types = [params.builtin_type("robobee"), params.builtin_type("tello")] if mixed else [params.builtin_type("robobee")]
    tid = (np.arange(n) % 2).astype(np.uint8) if mixed else np.zeros(n, dtype=np.uint8)
    rad = np.array([np.float64(np.float32(t.collision_sphere)) for t in types])[tid]
    opts = dict(alpha=2.0, buffer_drone=0.05, buffer_obstacle=0.1, share=0.5, floor=0.0)
    kw = dict(initial_xyzs=pos, obstacle_watch=d["scenes"], obstacle_margin=d["margin"], obstacle_scene_id=sid, obstacle_motion=motion,
              obstacle_offsets=off, obstacle_witness="world", obstacle_witness_velocity=True, obstacle_witnesses=3, neighbor_obs=6, neighbor_radius=1.5,
              dict_io=False, noise_seed=0)
    if mixed:
        kw.update(type_ids=tid, storage="auto")
    env = CtrlAviary(types, n, velocity_filter=opts, **kw)
    assert (env.order is not None) == mixed and env.last_filter_dropped is None and env.filter_counts() == (0, 0)
    u = (rng.normal(size=(n, 3)) * 1.5 / np.sqrt(3.0)).astype(np.float32)
    ut = torch.from_numpy(np.ascontiguousarray(u.T)).to(env.ctx.device)
    # before the first step: the on-demand queries, which leave last_* alone
    v0 = env.filter_velocity(ut).clone()
    assert env.last_neighbors is None and env.last_obstacle_witnesses is None and v0.shape == (3, n)
    ref0 = _env_rows(env, u, rad, env.nearest_neighbors(), env.obstacle_witnesses(), opts)
    ref0.check(v0.cpu().numpy().T, env.last_filter_dropped.cpu().numpy(), what=f"env before the first step, mixed={mixed}")
    tg = Targets(env.ctx, n)
    tg.set(pos=f32(pos).T, yaw=0.0)
    for _ in range(4):
        env.step_fused(tg)
    nb, wit = env.last_neighbors, env.last_obstacle_witnesses
    keep = [t.clone() for t in (nb.index, nb.dist, nb.rel_pos, nb.rel_vel, wit.clearance, wit.body, wit.rel, wit.vel)]
    ref = _env_rows(env, u, rad, nb, wit, opts)
    decision, value = ref.shares()
    print(f"env crowd mixed={mixed}: rows per drone {ref.valid.sum(1).mean():.2f}, neighbour rows {int(ref.valid[:, fr.NB_BIT:].sum())}, "
          f"obstacle rows {int(ref.valid[:, 1:9].sum())}")
    assert ref.valid[:, fr.NB_BIT:].sum() > n and ref.valid[:, 1:9].sum() > n // 4 and float(wit.vel.abs().max()) > 1e-3
    assert decision <= fr.GEO_DECISION_CAP and value <= fr.GEO_VALUE_CAP, (decision, value)
    assert np.abs(ref.v).max() <= fr.V_CAP
    v = env.filter_velocity(ut)
    ref.check(v.cpu().numpy().T, env.last_filter_dropped.cpu().numpy(), what=f"env crowd, mixed={mixed}")
    assert (ref.v != ref.u).any(1).sum() > n // 10
    # the filter reads the records and leaves them alone, bit for bit
    now = (nb.index, nb.dist, nb.rel_pos, nb.rel_vel, wit.clearance, wit.body, wit.rel, wit.vel)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(keep, now))
    changed, lost = env.filter_counts()
    assert changed >= int((ref.v != ref.u).any(1).sum()) - int(ref.decision.sum()) and lost >= 0
    if mixed:
        # negative control: every radius taken as the first type's gives other rows
        wrong = _env_rows(env, u, np.full(n, rad[0]), nb, wit, opts)
        assert np.abs(wrong.b - ref.b).max() > 1e-2
    env.close()


def test_env_without_the_keyword_has_no_filter(gpu):
    from dronesim_amd.envs import VelocityAviary
    env = VelocityAviary(["tello"], 4, initial_xyzs=np.array([[0.0, i, 1.0] for i in range(4)]), neighbor_obs=2, neighbor_radius=2.0,
                         dict_io=False)
    assert env._filter is None and not hasattr(env, "_filter_u") and env.last_filter_dropped is None
    with pytest.raises(ValueError, match="velocity_filter"):
        env.filter_velocity(torch.zeros((3, 4), device=env.ctx.device))
    with pytest.raises(ValueError, match="velocity_filter"):
        env.step_velocity(torch.zeros((3, 4), device=env.ctx.device))
    env.step_velocity(torch.ones((3, 4), device=env.ctx.device), filter=False)         # the encoding alone works without it
    assert float(env._vel_action[:, 3].max()) <= 1.0 and env._env_steps == 1
    env.close()


# ---- 7. VelocityAviary.step_velocity ------------------------------------------------------------------------------------------------------
def _pass_and_gate():
    """Four tellos: two head-on at 2 m/s a few centimetres off each other's line, two flown at the committed gate's frame."""
    gate = sr.gate()
    lo, hi = (np.asarray(x, dtype=np.float64) for x in gate.aabb)
    mid = 0.5 * (lo + hi)
    xyz = np.array([[-1.2, 6.0, 1.0], [1.2, 6.04, 1.0], [lo[0] - 0.8, mid[1], hi[2] - 0.02], [lo[0] - 0.8, lo[1] + 0.02, mid[2]]])
    u = np.array([[2.0, 0.0, 0.0], [-2.0, 0.0, 0.0], [1.5, 0.0, 0.0], [1.5, 0.0, 0.0]], dtype=np.float32)
    return gate, xyz, u


def _fly(filtered, actions=None, steps=40):
    from dronesim_amd.envs import VelocityAviary
    gate, xyz, u = _pass_and_gate()
    opts = dict(alpha=3.0, buffer_drone=0.1, buffer_obstacle=0.05, share=0.5, floor=0.0)
    kw = dict(initial_xyzs=xyz, aggregate_phy_steps=5, freq=240, dict_io=False, obstacle_watch=gate, obstacle_margin=1.0,
              obstacle_witness="world", obstacle_witnesses=2, neighbor_obs=2, neighbor_radius=4.0, noise_seed=0)
    env = VelocityAviary(["tello"], 4, velocity_filter=opts if filtered else None, **kw)
    rad = np.full(4, np.float64(np.float32(env.ctx.types[0].collision_sphere)))
    ut = torch.from_numpy(np.ascontiguousarray(u.T)).to(env.ctx.device)
    log = []
    for t in range(steps):
        if filtered:
            if env.last_neighbors is None:
                nb, wit = env.nearest_neighbors(), env.obstacle_witnesses()
            else:
                nb, wit = env.last_neighbors, env.last_obstacle_witnesses
            ref = _env_rows(env, u, rad, nb, wit, opts)
            env.step_velocity(ut)
            v, dropped = env._filter_out.vel[:, :4].cpu().numpy().T.copy(), env.last_filter_dropped.cpu().numpy().copy()
            log.append(dict(ref=ref, v=v, dropped=dropped, action=env._vel_action.clone()))
        else:
            # (as the filtering env goes: the same host reads, and the action in one buffer at a fixed address)
            env.state.pos.cpu(), env.state.vel.cpu()
            if t == 0:
                buf = torch.zeros_like(actions[0])
            buf.copy_(actions[t])
            env.step(buf)
            log.append(dict())
        nb, wit = env.last_neighbors, env.last_obstacle_witnesses
        log[-1]["records"] = [x.clone() for x in (nb.index, nb.dist, nb.rel_pos, nb.rel_vel, wit.clearance, wit.body, wit.rel)]
        log[-1]["state"] = env.state.fields(0, 13).clone()
    state = env.state.fields(0, 13).clone()
    counts = env.filter_counts() if filtered else None
    env.close()
    return log, state, counts


def test_step_velocity_head_on_pass_and_a_flight_at_the_gate(gpu):
    log, state, counts = _fly(True)
    slack_min, least_gap, least_clr, changed = np.inf, np.inf, np.inf, 0
    for t, s in enumerate(log):
        ref, v, dropped = s["ref"], s["v"], s["dropped"]
        ref.check(v, dropped, what=f"step {t}")
        ok = dropped == 0
        slack = np.where(ref.valid & ok[:, None], np.einsum("nmk,nk->nm", ref.A, v.astype(np.float64)) - ref.b, np.inf)
        slack_min = min(slack_min, float(slack.min()))              # every row rebuilt from the records, met by the v that was given
        changed += int((v != ref.u).any(1).sum())
        least_gap = min(least_gap, float(s["records"][1][0, :2].min()))
        least_clr = min(least_clr, float(s["records"][4][0, 2:].min()))
        a = s["action"].cpu().numpy()
        speed = np.linalg.norm(v, axis=1)
        np.testing.assert_allclose(a[:, :3] * speed[:, None], v, atol=1e-5)
        np.testing.assert_allclose(a[:, 3], np.minimum(speed / (30.0 / 3.6), 1.0), rtol=1e-6)
    print(f"step_velocity: least slack of a kept row {slack_min:.3e}, least distance of the pair {least_gap:.3f} m, least clearance to the "
          f"gate {least_clr:.3f} m, drone x steps changed {changed}, filter_counts {counts}")
    assert slack_min >= -fr.BAR
    assert changed > 10 and counts[0] == changed                  # the filter acted: on the pair and at the gate
    assert least_gap < 2.0 and least_clr < 1.0                    # ... because the pair met and the gate was reached
    # a twin that does not filter, fed the same actions: the same records behind every step, bit for bit
    twin, state2, _ = _fly(False, actions=[s["action"] for s in log])
    for t, (s, w) in enumerate(zip(log, twin)):
        assert torch.equal(s["state"], w["state"]), (t, float((s["state"] - w["state"]).abs().max()))
        for name, a, b in zip(("index", "dist", "rel_pos", "rel_vel", "clearance", "body", "rel"), s["records"], w["records"]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (t, name, a, b)
    assert torch.equal(state, state2)
    # two runs are bit-identical
    again, state3, counts3 = _fly(True)
    assert torch.equal(state, state3) and counts3 == counts
    for s, w in zip(log, again):
        assert np.array_equal(s["v"].view(np.uint32), w["v"].view(np.uint32)) and np.array_equal(s["dropped"], w["dropped"])
