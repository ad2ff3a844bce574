"""GPU tests of corridor clearance (dsim_corridor_clearance, corridor.Corridor, the env's corridor keyword) against a brute-force
fp64 segment-triangle computation (tests/corridor_ref.py) on the fp32 positions, rel rows, offsets, vertices and placements the
device holds.  tests/README_corridor.md.

Input rule, as tests/README_sweep.md: GUARD = 1e-4 m, ATOL = 1e-5 m, positions within 16 m, offsets within 128 m.  A segment whose
reference clearance lies within GUARD of 0 or of the margin gets a new rel row, at most 1 % of a case's slots (asserted on the
reference alone).  The -inf / unserved status and the `body != -1` status are then compared EXACTLY, clearances with atol ATOL, and
`body` may differ only where two bodies' reference minima are within ATOL, on at most 1 % of a case's slots.  Every case prints the
device's own worst |clearance - fp64| before it asserts."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from dronesim_amd import params
from tests import motion_ref as mr
from tests import scenes_ref as sr
from tests.corridor_ref import GROUND, corridor_brute, pieces
from tests.test_gpu_obstacles import ATOL, GUARD, _mixed_types, load, soa3, soup
from tests.util import f32

pytestmark = pytest.mark.gpu

assert GUARD == 1e-4 and ATOL == 1e-5


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product has no CPU fallback")
    from dronesim_amd import _native as nat
    from dronesim_amd import fleet
    return nat, fleet


# ---- what the cases share -------------------------------------------------------------------------------------------------------------
def half_of(types, reach, margin, sag):
    """reach - (R_max + sag + margin) in the library's numbers."""
    r_max = max(float(np.float32(t.collision_sphere)) for t in types)
    return float(np.float32(reach)) - (r_max + float(np.float32(sag)) + float(np.float32(margin)))


def brute(w, rel, index=None, sel=None):
    """The reference on the world dict ``w`` (pos, rad, margin, sag, off, half, kw); ``sel`` = (t, i): the raw clearance of those slots only."""
    if sel is None:
        return corridor_brute(w["pos"], rel, w["rad"], w["margin"], w.get("sag", 0.0), w.get("off"), index=index, half=w["half"], **w["kw"])
    t, i = sel
    kw = dict(w["kw"])
    if "scene_id" in kw:
        kw["scene_id"] = np.asarray(kw["scene_id"])[i]
    off = w["off"][i] if w.get("off") is not None else None
    return corridor_brute(w["pos"][i], rel[t, :, i].T[None], w["rad"][i], w["margin"], w.get("sag", 0.0), off, half=w["half"], **kw)["raw"][0]


def settle(rng, w, rel, draw):
    """The input rule: slots whose raw clearance sits within GUARD of 0 or of the margin get a new row draw(rng, t, i) -> [m, 3];
    -> (rel, fraction re-drawn, the reference of the first world on the settled rows).  Only the re-drawn slots are evaluated
    again.  ``w`` may be a list of worlds the same segments are asked in: a slot is re-drawn when it sits in the band of any."""
    ws = w if isinstance(w, list) else [w]
    first = [brute(x, rel) for x in ws]
    raws = [r["raw"].copy() for r in first]
    redrawn = np.zeros(raws[0].shape, dtype=bool)
    for _ in range(50):
        bad = np.zeros(redrawn.shape, dtype=bool)
        for x, raw in zip(ws, raws):
            bad |= (np.abs(raw) < GUARD) | (np.abs(raw - x["margin"]) < GUARD)
        if not bad.any():
            return rel, float(redrawn.mean()), (brute(ws[0], rel) if redrawn.any() else first[0])
        redrawn |= bad
        t, i = np.nonzero(bad)
        rel[t, :, i] = draw(rng, t, i)
        for x, raw in zip(ws, raws):
            raw[t, i] = brute(x, rel, sel=(t, i))
    raise AssertionError("the input rule did not settle")


def uniform_rows(len_lo, len_hi):
    def draw(rng, t, i):
        v = rng.normal(size=(len(i), 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        return f32(v * rng.uniform(len_lo, len_hi, (len(i), 1)))
    return draw


def first_rows(rng, k, n, draw):
    t, i = np.divmod(np.arange(k * n), n)
    rel = np.zeros((k, 3, n), dtype=np.float32)
    rel[t, :, i] = draw(rng, t, i)
    return rel


def rel_tensor(rel, n_pad, dev):
    k, _, n = rel.shape
    t = torch.zeros((k, 3, n_pad), dtype=torch.float32)
    t[:, :, :n] = torch.from_numpy(np.ascontiguousarray(rel))
    return t.to(dev)


def check(out, ref, margin, what):
    """-> the device's worst |clearance - fp64| over the served slots."""
    got, gb = out.clearance.cpu().numpy().astype(np.float64), out.body.cpu().numpy().astype(np.int64)
    served = ref["served"]
    np.testing.assert_array_equal(np.isneginf(got), ~served)
    err = float(np.abs(got[served] - ref["clr"][served]).max()) if served.any() else 0.0
    tie = (ref["body"] != -1) & (ref["gap"] < ATOL)
    print(f"corridor {what}: max |got - ref| = {err:.3e} m over {int(served.sum())} served slots of {served.size}, "
          f"{int((ref['body'] != -1).sum())} within the margin, {int((ref['raw'] < 0).sum())} blocked, {int(tie.sum())} ties")
    np.testing.assert_array_equal(gb != -1, ref["body"] != -1)
    np.testing.assert_allclose(got[served], ref["clr"][served], rtol=0, atol=ATOL)
    assert np.all(got[served & (ref["body"] == -1)] == np.float32(margin))
    assert tie.mean() <= 0.01, tie.mean()
    np.testing.assert_array_equal(gb[~tie], ref["body"][~tie])
    return err


def one_type(model):
    t = params.builtin_type(model)
    return t, np.float32(t.collision_sphere)


# ---- 1. one triangle: piercing, minimum at an end, minimum inside against an edge, the point query ------------------------------------
def test_one_triangle_every_class(gpu):
    nat, fleet = gpu
    from dronesim_amd import obstacles as obs
    from dronesim_amd.corridor import Corridor
    t, R = one_type("robobee")
    n, k, margin = 5, 4, 0.75
    tri = np.array([[[0.0, 0.0, 1.0], [2.0, 0.0, 1.0], [0.5, 1.5, 1.3]]])
    s = obs.ObstacleSet(tri, 0)
    jit = np.random.default_rng(5).uniform(-0.05, 0.05, (n, 3)) * [1, 1, 0]
    pos = f32(np.array([1.0, -0.4, 1.5]) + jit)                          # beside the edge AB (y = 0, z = 1) and above it, 0.64 m off
    rel = np.zeros((k, 3, n), dtype=np.float32)
    rel[0] = (f32(np.array([5.0 / 6.0, 0.7, 0.5]) + jit) - pos).T        # to a point below the face: through it, both ends clear
    rel[1] = np.array([[0.0], [-0.3], [0.4]], dtype=np.float32)          # away from the edge: the minimum at the near end
    rel[2, 2] = -1.0                                                     # straight down past the edge, which it passes at 0.4 m
    # (slot 3: a zero row, the point query)
    types = [t]
    reach = obs.corridor_reach(types, margin, 0.0, 0.5)
    w = dict(pos=pos, rad=np.full(n, R), margin=margin, half=half_of(types, reach, margin, 0.0), kw=dict(tri32=s.triangles, body=s.body))
    ref = brute(w, rel)
    assert ref["served"].all() and np.all(np.abs(ref["raw"]) > GUARD) and np.all(np.abs(ref["raw"] - margin) > GUARD)
    assert np.all(np.abs(ref["raw"][0] + float(R)) < 1e-12)              # piercing: exactly -Rs
    ends = brute(w, np.zeros_like(rel))["raw"][0]
    far = brute(dict(w, pos=f32(pos + rel[0].T)), np.zeros_like(rel))["raw"][0]
    assert np.all(ends > 0.1) and np.all(far > 0.1)                      # ... with both ends clear
    assert np.all(np.abs(ref["raw"][1] - ends) < 1e-12)                  # the minimum at an end
    e2 = brute(dict(w, pos=f32(pos + rel[2].T)), np.zeros_like(rel))["raw"][0]
    assert np.all(ref["raw"][2] < np.minimum(ends, e2) - 0.05)           # the minimum inside the segment ...
    assert np.all(np.abs(ref["raw"][2] + float(R) - 0.4) < 0.06)         # ... against the edge
    assert np.all(np.abs(ref["raw"][3] - ends) < 1e-12)                  # the zero row is the point query
    ctx = fleet.Context(types)
    dev = s.to_device(ctx, reach)
    st = load(fleet, ctx, pos)
    cor = Corridor(ctx, st, dev, k, margin)
    out = cor.query(rel_tensor(rel, st.n_pad, ctx.device))
    check(out, ref, margin, "one triangle, n = 5, k = 4 (one slot per workgroup)")
    got = out.clearance.cpu().numpy()
    assert np.all(got[0] == -R)                                          # exactly: sqrt(0) - Rs
    # the zero row against dsim_obstacle_clearance
    clr = torch.full((st.n_pad,), -7.0, dtype=torch.float32, device=ctx.device)
    near = torch.full((st.n_pad,), -7, dtype=torch.int32, device=ctx.device)
    obs.query(ctx, st, dev, margin, clr, near)
    d = float(np.abs(got[3].astype(np.float64) - clr[:n].cpu().numpy()).max())
    print(f"zero-length segments against the point query: {d:.3e} m")
    assert d <= ATOL and np.array_equal(out.body.cpu().numpy()[3], near[:n].cpu().numpy())
    assert cor.unserved() == 0 and ctx.query(nat.QUERY_OBSTACLE_CONTACTS) == int((clr[:n] < 0).sum())      # (the query counts nothing)
    cor.close()
    dev.close()
    ctx.close()


# ---- 2. the gate: the LDS instance, two tiles, segments that cross the box from outside ----------------------------------------------
GATE_N, GATE_K, GATE_MARGIN, GATE_PIECE = 300, 8, 0.5, 0.5


@functools.lru_cache(maxsize=None)
def _gate_case(offsets):
    """Computed once per offsets (shared by both layouts, never written to).  Slots 0 .. 6: a uniform direction, 0 - 1.5 m.  Slot
    7: from 1.2 - 1.5 m in front of the gate's plane straight to the other side, both ends outside the grown box."""
    from dronesim_amd.obstacles import corridor_reach
    t, R = one_type("robobee")
    s = sr.gate()
    n, k, margin = GATE_N, GATE_K, GATE_MARGIN
    reach = corridor_reach([t], margin, 0.0, GATE_PIECE)
    rng = np.random.default_rng(211)
    q = rng.uniform([-1.5, -1.2, -1.0], [-1.2, 1.2, 1.0], (n, 3))
    q[n // 2:] = rng.uniform([-1.0, -1.4, -1.2], [1.0, 1.4, 1.2], (n - n // 2, 3))
    pos, off = sr.with_offsets(rng, q) if offsets else (f32(q), None)
    through = np.arange(n) < n // 2
    e = pos.astype(np.float64) - (off.astype(np.float64) if offsets else 0.0)
    uni = uniform_rows(0.0, 1.5)

    def draw(rg, tt, ii):
        rows = uni(rg, tt, ii)
        cross = (tt == k - 1) & through[ii]
        to = np.stack([rg.uniform(1.2, 1.5, len(ii)), rg.uniform(-0.6, 0.6, len(ii)), rg.uniform(-0.45, 0.45, len(ii))], 1)
        return np.where(cross[:, None], f32(to - e[ii]), rows)
    w = dict(pos=pos, off=off, rad=np.full(n, R), margin=margin, half=half_of([t], reach, margin, 0.0),
             kw=dict(tri32=s.triangles, body=s.body))
    rel, frac, ref = settle(rng, w, first_rows(rng, k, n, draw), draw)
    assert frac <= 0.01, frac
    # slot 7 of the first half: both ends outside the grown box, the middle through the gate's plane
    g, _, _ = s.grid(reach)
    far = e[through] + rel[k - 1].T.astype(np.float64)[through]
    assert np.all(e[through, 0] < g.lo[0]) and np.all(far[:, 0] > g.hi[0])
    crossing = ref["body"][k - 1][through] >= 0
    print(f"gate offsets={offsets}: re-drawn {frac:.4f}; {int(crossing.sum())} of {int(through.sum())} segments from outside the grown "
          f"box to outside it come within the margin, {int((ref['raw'][k - 1][through] < 0).sum())} are blocked")
    assert crossing.sum() >= 50 and (ref["raw"][k - 1][through] < 0).sum() >= 20
    assert pieces(np.linalg.norm(rel[k - 1].T[through], axis=1), w["half"]).min() >= 5
    return s, reach, w, rel, ref


@pytest.mark.parametrize("layout", ["soa", "tile64"])
@pytest.mark.parametrize("offsets", [False, True])
def test_gate_vs_bruteforce(gpu, layout, offsets):
    nat, fleet = gpu
    from dronesim_amd.corridor import Corridor
    s, reach, w, rel, ref = _gate_case(offsets)
    assert s.n_tri <= 512                                                # the LDS instance
    ctx = fleet.Context([params.builtin_type("robobee")])
    dev = s.to_device(ctx, reach)
    st = load(fleet, ctx, w["pos"], layout)
    cor = Corridor(ctx, st, dev, GATE_K, GATE_MARGIN, offsets=w["off"])
    out = cor.query(rel_tensor(rel, st.n_pad, ctx.device))
    check(out, ref, GATE_MARGIN, f"gate {layout} offsets={offsets}")
    assert cor.unserved() == 0 and ctx.query(nat.QUERY_OBSTACLE_CONTACTS) == 0
    assert bool(torch.isneginf(cor.clearance_out[:, GATE_N:]).all()) and bool((cor.body_out[:, GATE_N:] == -1).all())   # (lanes >= n: not written)
    cor.close()
    dev.close()
    ctx.close()


# ---- 3. the soup: records through L2, up to 6 pieces; the same segments in one piece ---------------------------------------------------
def test_soup_results_do_not_depend_on_the_piece_count(gpu):
    nat, fleet = gpu
    from dronesim_amd.corridor import Corridor
    from dronesim_amd.obstacles import corridor_reach
    s = soup()
    t, R = one_type("hexa_6DOF")
    n, k, margin = 300, 3, 0.6
    reach_a, reach_b = corridor_reach([t], margin, 0.0, 0.5), corridor_reach([t], margin, 0.0, 3.0)
    rng = np.random.default_rng(229)
    pos = f32(rng.uniform(-10.0, 10.0, (n, 3)))
    draw = uniform_rows(0.0, 3.0)
    w = dict(pos=pos, rad=np.full(n, R), margin=margin, half=half_of([t], reach_a, margin, 0.0), kw=dict(tri32=s.triangles, body=s.body))
    rel, frac, ref = settle(rng, w, first_rows(rng, k, n, draw), draw)
    assert frac <= 0.01, frac
    assert np.abs(pos).max() <= 16.0 and np.abs(pos + rel.transpose(0, 2, 1)).max() <= 16.0 and s.n_tri == 3000
    K = pieces(np.linalg.norm(rel, axis=1), w["half"])
    print(f"soup: re-drawn {frac:.4f}; pieces at 0.5 m: max {int(K.max())}, {int((K >= 3).sum())} slots with 3 or more; "
          f"{int((ref['raw'] < 0).sum())} blocked")
    assert K.max() == 6 and (K >= 3).sum() > 300 and (ref["body"] >= 0).sum() > 200 and (ref["raw"] < 0).sum() > 30
    assert pieces(np.linalg.norm(rel, axis=1), half_of([t], reach_b, margin, 0.0)).max() == 1
    ctx = fleet.Context([t])
    st = load(fleet, ctx, pos)
    d_rel = rel_tensor(rel, st.n_pad, ctx.device)
    got = []
    for reach, what in ((reach_a, "up to 6 pieces"), (reach_b, "one piece")):
        dev = s.to_device(ctx, reach)
        cor = Corridor(ctx, st, dev, k, margin)
        out = cor.query(d_rel)
        check(out, ref, margin, f"soup, {what}")
        assert cor.unserved() == 0
        got.append(out.clearance.cpu().numpy().astype(np.float64))
        cor.close()
        dev.close()
    d = float(np.abs(got[0] - got[1]).max())
    print(f"soup: pieces against one piece: {d:.3e} m")
    assert d <= ATOL
    ctx.close()


# ---- 4. against the swept watch: the same chord, traversed the other way round --------------------------------------------------------
def test_gate_against_the_swept_watch(gpu):
    nat, fleet = gpu
    from dronesim_amd import obstacles as obs
    from dronesim_amd.corridor import Corridor
    from tests.test_gpu_sweep import _gate_chords
    t, R = one_type("robobee")
    n, margin = 700, 1.0
    s = sr.gate()
    prev, pos, _, ref, _ = _gate_chords(False)
    ctx = fleet.Context([t])
    dev = s.to_device(ctx, obs.sweep_reach(ctx.types, margin, 0.0, 0.3))
    st = load(fleet, ctx, pos)
    clr = torch.full((st.n_pad,), -7.0, dtype=torch.float32, device=ctx.device)
    near = torch.full((st.n_pad,), -7, dtype=torch.int32, device=ctx.device)
    d_prev = soa3(prev, st.n_pad, ctx.device)
    obs.sweep(ctx, st, dev, margin, 0.0, d_prev, clr, near, keep_prev=True)
    rel = (prev - pos).astype(np.float32).T[None]                        # from the current position back to prev
    cor = Corridor(ctx, st, dev, 1, margin)
    out = cor.query(rel_tensor(rel, st.n_pad, ctx.device))
    a, b = out.clearance[0].cpu().numpy().astype(np.float64), clr[:n].cpu().numpy().astype(np.float64)
    print(f"corridor against the swept watch on {n} gate chords: max difference {np.abs(a - b).max():.3e} m, "
          f"{int((b < margin).sum())} within the margin")
    np.testing.assert_allclose(a, b, rtol=0, atol=ATOL)
    gb, nb = out.body[0].cpu().numpy(), near[:n].cpu().numpy()
    tie = (ref[1] >= 0) & (ref[2] < ATOL)
    assert np.array_equal(gb >= 0, nb >= 0) and np.array_equal(gb[~tie], nb[~tie]) and (b < margin).sum() > 100
    cor.close()
    dev.close()
    ctx.close()


# ---- 5. scenes ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene_case(name):
    from dronesim_amd.obstacles import corridor_reach
    c, k, seed = {"gates": (sr.case_gates(True), 2, 241), "ragged": (sr.case_ragged(), 3, 251)}[name]
    t, _ = one_type("robobee")
    reach = corridor_reach([t], c["margin"], 0.0, 0.5)
    rng = np.random.default_rng(seed)
    draw = uniform_rows(0.0, 1.5)
    w = dict(pos=c["pos"], off=c["off"], rad=c["rad"], margin=c["margin"], half=half_of([t], reach, c["margin"], 0.0),
             kw=dict(scenes=c["scenes"], scene_id=c["scene_id"]))
    rel, frac, ref = settle(rng, w, first_rows(rng, k, len(c["rad"]), draw), draw)
    assert frac <= 0.01, frac
    return c, k, reach, w, rel, ref, frac


@pytest.mark.parametrize("name", ["gates", "ragged"])
def test_scenes_vs_bruteforce(gpu, name):
    nat, fleet = gpu
    from dronesim_amd.corridor import Corridor
    c, k, reach, w, rel, ref, frac = _scene_case(name)
    sid, sc = np.asarray(c["scene_id"]), c["scenes"]
    print(f"scenes {name}: re-drawn {frac:.4f}; {int(((sid < 0) | (sid >= sc.K)).sum())} drones with an id outside [0, K), "
          f"counts {sorted(set(sc.count.tolist()))} of G = {sc.G}")
    if name == "ragged":
        out_of_range = (sid < 0) | (sid >= sc.K)
        assert out_of_range.sum() >= 20 and sc.count.min() == 0 and sc.count.max() == sc.G
        assert np.all(ref["body"][:, out_of_range | (sc.count[np.clip(sid, 0, sc.K - 1)] == 0)] == -1)
        assert (ref["body"] >= 2 * sc.n_bodies).sum() > 10              # winners in the later slots of the full scene
    assert (ref["raw"] < 0).sum() > 20
    ctx = fleet.Context([params.builtin_type("robobee")])
    dev = sc.to_device(ctx, reach)
    st = load(fleet, ctx, w["pos"])
    cor = Corridor(ctx, st, dev, k, w["margin"], offsets=w["off"], scene_id=sid)
    out = cor.query(rel_tensor(rel, st.n_pad, ctx.device))
    check(out, ref, w["margin"], f"scenes {name}, offsets up to 128 m")
    assert cor.unserved() == 0
    cor.close()
    dev.close()
    ctx.close()


def test_one_scene_of_one_placement_is_the_plain_query_on_the_flattened_set(gpu):
    nat, fleet = gpu
    from dronesim_amd.corridor import Corridor
    from dronesim_amd.obstacles import ObstacleScenes, corridor_reach
    t, R = one_type("robobee")
    n, k, margin = 300, 3, 0.5
    rng = np.random.default_rng(261)
    p, rpy = sr.random_placements(rng, 1, 1)
    sc = ObstacleScenes(sr.gate(), p, rpy)
    pos = f32(p[0, 0] + rng.uniform(-1.2, 1.2, (n, 3)))
    rel = first_rows(rng, k, n, uniform_rows(0.0, 1.5))
    reach = corridor_reach([t], margin, 0.0, 0.5)
    ctx = fleet.Context([t])
    st = load(fleet, ctx, pos)
    d_rel = rel_tensor(rel, st.n_pad, ctx.device)
    placed, flat = sc.to_device(ctx, reach), sc.flatten(0).to_device(ctx, reach)
    a = Corridor(ctx, st, placed, k, margin, scene_id=np.zeros(n, dtype=np.int64))
    b = Corridor(ctx, st, flat, k, margin)
    oa, ob = a.query(d_rel), b.query(d_rel)
    ca, cb = oa.clearance.cpu().numpy().astype(np.float64), ob.clearance.cpu().numpy().astype(np.float64)
    print(f"K = 1, G = 1 against the flattened set: max difference {np.abs(ca - cb).max():.3e} m, {int((cb < margin).sum())} within the margin")
    np.testing.assert_allclose(ca, cb, rtol=0, atol=ATOL)
    near_edge = np.abs(cb - margin) < ATOL
    assert np.array_equal(oa.body.cpu().numpy()[~near_edge], ob.body.cpu().numpy()[~near_edge]) and (cb < margin).sum() > 200
    for x in (a, b, placed, flat):
        x.close()
    ctx.close()


# ---- 6. moving scenes: the table where it stands now -------------------------------------------------------------------------------------
def test_moved_scenes_are_seen_where_they_stand(gpu):
    nat, fleet = gpu
    from dronesim_amd.corridor import Corridor
    from dronesim_amd.obstacles import corridor_reach
    from tests.test_gpu_motion import fleet_about
    t, R = one_type("robobee")
    n, k, margin, clock = 300, 4, 0.5, 7
    tau = clock * mr.DT
    reach = corridor_reach([t], margin, 0.0, 0.5)
    for j, motion in enumerate(mr.small_motions()):
        rng = np.random.default_rng(271 + j)
        pos, sid = fleet_about(motion, tau, n, 281 + j)
        now = motion.snapshot(tau)
        draw = uniform_rows(0.0, 1.5)
        w = dict(pos=pos, rad=np.full(n, R), margin=margin, half=half_of([t], reach, margin, 0.0), kw=dict(scenes=now, scene_id=sid))
        base = dict(w, kw=dict(scenes=motion.scenes, scene_id=sid))
        rel, frac, ref = settle(rng, [w, base], first_rows(rng, k, n, draw), draw)
        assert frac <= 0.01, frac
        still = brute(base, rel)
        moved = int((np.abs(np.minimum(still["raw"], 9.0) - np.minimum(ref["raw"], 9.0)) > 0.01).sum())
        assert moved > 100 and (ref["raw"] < 0).sum() > 30                # (the base table would be found out)
        ctx = fleet.Context([t])
        dev = motion.scenes.to_device(ctx, reach)
        dev.set_motion(motion)
        st = load(fleet, ctx, pos)
        cor = Corridor(ctx, st, dev, k, margin, scene_id=sid)
        d_rel = rel_tensor(rel, st.n_pad, ctx.device)
        check(cor.query(d_rel), still, margin, f"motion {j}, before the move")
        dev.move(torch.tensor([clock], dtype=torch.int64, device=ctx.device), mr.DT)
        check(cor.query(d_rel), ref, margin, f"motion {j}, after one move at a clock of {clock} (re-drawn {frac:.4f}, {moved} slots differ from the base)")
        cor.close()
        dev.close()
        ctx.close()


# ---- 7. the ground -------------------------------------------------------------------------------------------------------------------------
def test_ground(gpu):
    nat, fleet = gpu
    from dronesim_amd.corridor import Corridor
    from dronesim_amd.obstacles import corridor_reach
    t, R = one_type("robobee")
    s = sr.gate()
    n, k, margin = 300, 4, 0.5
    reach = corridor_reach([t], margin, 0.0, 0.5)
    rng = np.random.default_rng(291)
    lift = 0.7                                                           # the gate stands 0.3 m above the ground
    tri = f32(s.triangles.astype(np.float64) + [0.0, 0.0, lift])
    from dronesim_amd.obstacles import ObstacleSet
    lifted = ObstacleSet(tri, s.body)
    # (the drones stand 0.25 m or more off the gate's plane x = 0 and the dipping segments lead away from it: a segment that dips
    # AND pierces a bar has two bodies at exactly -Rs, and such ties are capped at 1 % of a case's slots)
    pos = f32(rng.uniform([0.25, -1.2, 0.05], [1.0, 1.2, 1.6], (n, 3)) * np.where(rng.uniform(size=(n, 1)) < 0.5, [-1.0, 1.0, 1.0], 1.0))
    uni = uniform_rows(0.0, 1.5)

    def draw(rg, tt, ii):
        rows = uni(rg, tt, ii)
        dip = np.stack([np.sign(pos[ii, 0]) * rg.uniform(0.0, 0.5, len(ii)), rg.uniform(-0.5, 0.5, len(ii)),
                        -pos[ii, 2] - rg.uniform(0.05, 0.5, len(ii))], 1)
        return np.where((tt == 0)[:, None], f32(dip), rows)              # slot 0 dips below z = 0
    both = dict(pos=pos, rad=np.full(n, R), margin=margin, half=half_of([t], reach, margin, 0.0),
                kw=dict(tri32=lifted.triangles, body=lifted.body, ground=True))
    alone = dict(both, half=np.inf, kw=dict(ground=True))
    rel, frac, ref = settle(rng, [both, alone], first_rows(rng, k, n, draw), draw)
    assert frac <= 0.01, frac
    dips = (pos[:, 2].astype(np.float64) + rel[0, 2].astype(np.float64)) < 0
    wins_g, wins_t = int((ref["body"] == GROUND).sum()), int((ref["body"] >= 0).sum())
    print(f"ground and gate: re-drawn {frac:.4f}; the ground wins {wins_g} slots, the gate {wins_t}")
    assert dips.all() and wins_g > 300 and wins_t > 100
    ctx = fleet.Context([t])
    dev = lifted.to_device(ctx, reach)
    st = load(fleet, ctx, pos)
    d_rel = rel_tensor(rel, st.n_pad, ctx.device)
    cor = Corridor(ctx, st, dev, k, margin, ground=True)
    out = cor.query(d_rel)
    check(out, ref, margin, "ground and gate together")
    # a segment that dips below z = 0 with the gate out of reach: the ground, exactly -Rs
    only_g = ref["body"][0] == GROUND
    got0 = out.clearance[0].cpu().numpy()
    assert only_g.sum() > 100 and np.all(got0[only_g] == -R) and np.all(out.body[0].cpu().numpy()[only_g] == GROUND)
    cor.close()
    # the ground alone is a valid world, and every finite segment is one piece
    cor = Corridor(ctx, st, None, k, margin, ground=True)
    assert cor.max_length == float("inf")
    out = cor.query(d_rel)
    ref_g = brute(alone, rel)
    check(out, ref_g, margin, "ground alone")
    assert np.all(out.clearance[0].cpu().numpy() == -R) and set(np.unique(out.body.cpu().numpy())) <= {GROUND, -1}
    assert cor.unserved() == 0
    cor.close()
    dev.close()
    ctx.close()


# ---- 8. edges --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 32])
def test_slot_counts_index_nan_and_unserved(gpu, k):
    nat, fleet = gpu
    from dronesim_amd.corridor import Corridor
    from dronesim_amd.obstacles import corridor_reach
    t, R = one_type("robobee")
    s = sr.gate()
    n, margin = 300, 0.5
    reach = corridor_reach([t], margin, 0.0, 0.25)
    half = half_of([t], reach, margin, 0.0)
    rng = np.random.default_rng(301 + k)
    pos = f32(rng.uniform([-1.0, -1.4, -1.2], [1.0, 1.4, 1.2], (n, 3)))
    draw = uniform_rows(0.0, 1.5)
    w = dict(pos=pos, rad=np.full(n, R), margin=margin, half=half, kw=dict(tri32=s.triangles, body=s.body))
    rel, frac, _ = settle(rng, w, first_rows(rng, k, n, draw), draw)
    assert frac <= 0.01, frac
    ctx = fleet.Context([t])
    dev = s.to_device(ctx, reach)
    cor_len = 64.0 * half * (1.0 - 2.0 ** -10)
    # the statuses: every 7th slot has a negative index, every 11th a NaN in its rel row, every 13th is 1.01 x max_length long,
    # drone 3 has a NaN in its position
    flat = np.arange(k * n).reshape(k, n)
    index = np.where(flat % 7 == 0, -1 - (flat % 3), flat % 5).astype(np.int32)
    nan_row, long_row = (flat % 11 == 1), (flat % 13 == 2) & (flat % 11 != 1)
    rel = rel.copy()
    rel[:, 1, :][nan_row] = np.nan
    v = rng.normal(size=(k, n, 3))
    v = f32(1.01 * cor_len * v / np.linalg.norm(v, axis=2, keepdims=True)).transpose(0, 2, 1)
    rel = np.where(long_row[:, None, :], v, rel)
    pos = pos.copy()
    pos[3, 2] = np.nan
    w = dict(w, pos=pos)
    ref = brute(w, rel, index=index)
    want_unserved = int((ref["evaluated"] & ~ref["served"]).sum())
    assert want_unserved == int((long_row & (index >= 0) & (np.arange(n) != 3)[None, :]).sum()) and want_unserved >= (1 if k == 1 else 50)
    assert not ref["evaluated"][:, 3].any() and (~ref["evaluated"]).sum() > k * n // 6
    st = fleet.FleetState(ctx, n, "soa")
    from tests.util import random_fleet
    rigid, mem, _ = random_fleet(np.random.default_rng(5), n, n_act=ctx.n_act)
    rigid[:, 0:3] = pos
    st.load_aos(rigid, mem)
    cor = Corridor(ctx, st, dev, k, margin)
    assert abs(cor.max_length - cor_len) < 1e-9
    d_index = torch.full((k, st.n_pad), -1, dtype=torch.int32, device=ctx.device)
    d_index[:, :n] = torch.from_numpy(index).to(ctx.device)
    out = cor.query(rel_tensor(rel, st.n_pad, ctx.device), d_index)
    check(out, ref, margin, f"k = {k}: index, NaN and unserved slots")
    assert cor.unserved() == want_unserved                               # a negative index and a NaN are not counted
    out = cor.query(rel_tensor(rel, st.n_pad, ctx.device), d_index, body=False)
    assert out.body is None and cor.unserved() == 2 * want_unserved
    cor.close()
    dev.close()
    ctx.close()


def test_mixed_fleet_with_a_type_of_radius_zero_and_a_sag(gpu):
    nat, fleet = gpu
    from dronesim_amd.corridor import Corridor
    from dronesim_amd.obstacles import corridor_reach
    types = _mixed_types()
    s = sr.gate()
    n, k, margin, sag = 300, 3, 0.75, 0.01
    tid = (np.arange(n) % 4).astype(np.uint8)
    rad = np.array([np.float32(t.collision_sphere) for t in types])[tid]
    reach = corridor_reach(types, margin, sag, 0.5)
    rng = np.random.default_rng(311)
    pos, off = sr.with_offsets(rng, rng.uniform([-1.0, -1.4, -1.2], [1.0, 1.4, 1.2], (n, 3)))
    draw = uniform_rows(0.0, 1.5)
    w = dict(pos=pos, off=off, rad=rad, margin=margin, sag=sag, half=half_of(types, reach, margin, sag), kw=dict(tri32=s.triangles, body=s.body))
    rel, frac, ref = settle(rng, w, first_rows(rng, k, n, draw), draw)
    assert frac <= 0.01 and (rad == 0).sum() == n // 4
    ghosts = ref["raw"][:, rad == 0]
    assert (ghosts < 0).sum() > 5 and (ghosts < margin).sum() > 50       # a type with R = 0 still asks, with the radius sag
    ctx = fleet.Context(types)
    dev = s.to_device(ctx, reach)
    st = load(fleet, ctx, pos)
    t_id = torch.zeros((st.n_pad,), dtype=torch.uint8, device=ctx.device)
    t_id[:n] = torch.from_numpy(tid).to(ctx.device)
    cor = Corridor(ctx, st, dev, k, margin, sag=sag, offsets=off, type_id=t_id)
    check(cor.query(rel_tensor(rel, st.n_pad, ctx.device)), ref, margin, f"mixed fleet, R = 0 type, sag {sag} (re-drawn {frac:.4f})")
    with pytest.raises(ValueError, match="type_id is required"):
        Corridor(ctx, st, dev, k, margin, sag=sag)
    cor.close()
    dev.close()
    ctx.close()


def test_every_refusal_returns_e_arg_and_writes_nothing(gpu):
    nat, fleet = gpu
    from dronesim_amd.obstacles import ObstacleScenes, corridor_reach, watch_reach
    t, R = one_type("robobee")
    s = sr.gate()
    n, k, margin = 70, 4, 0.5
    ctx = fleet.Context([t])
    dev = s.to_device(ctx, corridor_reach([t], margin, 0.0, 0.5))
    tight = s.to_device(ctx, watch_reach([t], margin))                   # half = reach / 1025: the point watch's set
    p, rpy = sr.random_placements(np.random.default_rng(1), 1, 1)
    scenes = ObstacleScenes(s, p, rpy).to_device(ctx, prototype_dev=dev)
    st = load(fleet, ctx, f32(np.random.default_rng(2).uniform(-1, 1, (n, 3))))
    rel = torch.zeros((k, 3, st.n_pad), dtype=torch.float32, device=ctx.device)
    clr = torch.full((k, st.n_pad), -7.0, dtype=torch.float32, device=ctx.device)
    body = torch.full((k, st.n_pad), -7, dtype=torch.int32, device=ctx.device)
    uns = torch.zeros((1,), dtype=torch.int64, device=ctx.device)
    sid = torch.zeros((st.n_pad,), dtype=torch.int32, device=ctx.device)
    E_ARG = -1

    def call(set_=dev, n_=n, ctx_=ctx.handle, null_args=False, **kw):
        a = nat.CorridorArgs()
        a.rel, a.k, a.flags, a.margin, a.sag = rel.data_ptr(), k, 0, margin, 0.0
        a.clearance_out, a.body_out, a.unserved_out = clr.data_ptr(), body.data_ptr(), uns.data_ptr()
        for name, v in kw.items():
            setattr(a, name, v)
        return ctx.lib.dsim_corridor_clearance(ctx_, ctx.stream_ptr(), n_, st.view(), set_.handle if set_ is not None else None,
                                               None if null_args else ctypes.byref(a))
    refused = {
        "a null ctx": call(ctx_=None), "null args": call(null_args=True), "a null rel": call(rel=None),
        "a null clearance_out": call(clearance_out=None), "n = 0": call(n_=0), "n > n_pad": call(n_=st.n_pad + 1),
        "k = 0": call(k=0), "k = 33": call(k=33), "an unknown flag": call(flags=2), "margin = 0": call(margin=0.0),
        "margin < 0": call(margin=-0.5), "margin = inf": call(margin=float("inf")), "margin = NaN": call(margin=float("nan")),
        "sag < 0": call(sag=-0.01), "sag = inf": call(sag=float("inf")), "sag = NaN": call(sag=float("nan")),
        "scenes without scene_id": call(set_=None, scenes=scenes.handle), "scene_id without scenes": call(scene_id=sid.data_ptr()),
        "scenes together with a set": call(scenes=scenes.handle, scene_id=sid.data_ptr()), "no world at all": call(set_=None),
        "half < reach / 1024": call(set_=tight),
    }
    ctx2 = fleet.Context(_mixed_types())
    refused["several types and no type_id"] = call(ctx_=ctx2.handle)
    torch.cuda.synchronize()
    assert all(rc == E_ARG for rc in refused.values()), refused
    assert bool((clr == -7.0).all()) and bool((body == -7).all()) and int(uns.item()) == 0
    # and what is not refused: the ground alone, scenes, a set
    assert call(set_=None, flags=nat.CORRIDOR_GROUND) == 0 and call(set_=None, scenes=scenes.handle, scene_id=sid.data_ptr()) == 0 and call() == 0
    torch.cuda.synchronize()
    assert bool((clr[:, :n] != -7.0).all()) and bool((clr[:, n:] == -7.0).all())
    ctx2.close()
    scenes.close()
    tight.close()
    dev.close()
    ctx.close()


# ---- 9. the env ------------------------------------------------------------------------------------------------------------------------------
def test_env_corridor_behind_every_kind_of_launch_and_its_twin_without(gpu):
    nat, _ = gpu
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.fleet import Targets
    from dronesim_amd.obstacles import ObstacleScenes, corridor_reach, watch_reach
    from tests.test_gpu_motion import fleet_about, same_bits
    n, k, margin, dt = 300, 4, 0.5, 5 / 240
    tid = (np.arange(n) % 2).astype(np.uint8)
    types = [params.builtin_type("tello"), params.builtin_type("hexa_6DOF")]
    rad = np.array([np.float32(t.collision_sphere) for t in types])[tid]
    motion = mr.small_motions()[0]
    xyz, sid = fleet_about(motion, 3 * dt, n, 321)
    xyz = xyz.astype(np.float64)
    kw = dict(initial_xyzs=xyz, type_ids=tid, storage="auto", aggregate_phy_steps=5, obstacle_watch=motion.scenes, obstacle_margin=margin,
              obstacle_scene_id=sid, obstacle_motion=motion, dict_io=False, noise_seed=0)
    env, twin = CtrlAviary(types, n, corridor=dict(k=k, piece=0.5), **kw), CtrlAviary(types, n, **kw)
    assert env.order is not None and not np.array_equal(env.order.drone_np, np.arange(n))
    reach = corridor_reach(types, margin, 0.0, 0.5)
    assert env._obst.reach == float(np.float32(reach)) > twin._obst.reach == float(np.float32(watch_reach(types, margin)))
    with pytest.raises(ValueError, match="needs an env made with corridor"):
        twin.corridor_clearance(np.zeros((k, 3, n), dtype=np.float32))
    with pytest.raises(ValueError, match="needs an env made with corridor"):
        twin.corridor_unserved()
    with pytest.raises(ValueError, match="rel must be"):
        env.corridor_clearance(np.zeros((k, 3, n + 1), dtype=np.float32))
    tgs = [Targets(e.ctx, n) for e in (env, twin)]
    for tg in tgs:
        tg.set(pos=f32(xyz).T, yaw=0.0)
    rng = np.random.default_rng(331)
    draw = uniform_rows(0.0, 1.5)
    half = half_of(types, reach, margin, 0.0)

    def behind(what):
        pos = env.state.pos.T.cpu().numpy().astype(np.float32)           # the caller's numbering, as the device holds them
        now = ObstacleScenes.from_place(motion.scenes.prototype, env.scene_placements(), motion.scenes.count)
        w = dict(pos=pos, rad=rad, margin=margin, half=half, kw=dict(scenes=now, scene_id=sid))
        rel, frac, _ = settle(rng, w, first_rows(rng, k, n, draw), draw)
        assert frac <= 0.01, frac
        index = np.where(rng.uniform(size=(k, n)) < 0.1, -1, 0)
        ref = brute(w, rel, index=index)
        before = env.obstacle_contacts()
        out = env.corridor_clearance(rel, index)
        assert tuple(out.clearance.shape) == (k, n) == tuple(out.body.shape)
        check(out, ref, margin, f"env, {what} (re-drawn {frac:.4f})")
        assert (ref["raw"] < 0).sum() > 20 and env.obstacle_contacts() == before and env.corridor_unserved() == 0
        # the twin without the keyword: the same watch, bit for bit, on a set of a smaller reach
        a, b = env.last_obstacle_clearance, twin.last_obstacle_clearance
        assert same_bits(a[0], b[0]) and torch.equal(a[1], b[1]) and env.obstacle_contacts() == twin.obstacle_contacts(), what
        assert np.array_equal(env.scene_placements().view(np.uint32), twin.scene_placements().view(np.uint32))

    for e in (env, twin):
        e.step(torch.zeros((n, e.n_act), dtype=torch.float32, device=e.ctx.device))
    behind("step()")
    for e, tg in zip((env, twin), tgs):
        e.step_fused(tg, n_steps=3)
    behind("step_fused(n_steps=3)")
    assert env.scene_time() == 4 * dt
    env.close()
    twin.close()
