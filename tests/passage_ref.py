"""The reference of the gate passage tests (numpy only, so the CPU tests use it without a device).  tests/README_passage.md.

fp64 on the fp32 inputs the device holds, with no cull: both ends of every chord into every used placement's frame with the SAME
float32 R and t (scenes_ref.placement64), the signed distances from the aperture's plane, the half-open crossing rule, the
crossing point against the aperture and the outer rectangle, then the progress rule drone by drone.  A float32 restatement of
the kernel's arithmetic (gate_eval of dsim_passage.hip), from which the tolerance of the passage time is derived, and the inputs
the GPU cases and the CPU checks of their conditions share."""
import functools

import numpy as np

from tests import scenes_ref as sr
from tests.util import f32

GUARD = 1e-4
# the float32 restatement's worst |tau32 - tau64| |s1 - s0| [m along the normal] over the crossings of the GPU cases' own inputs:
# measured by tests/test_passage_cpu.py::test_restated_tau_error_is_what_is_recorded; the kernel is granted 4 x this
RESTATED_WORST = 7.80e-8
TAU_TOL = 4.0 * RESTATED_WORST
TRAVEL = 2.0


def gate_aperture(shape="rect"):
    """The opening of tests/golden/gate_50_curved: a rectangle on the plane x = 0, normal +x, half-extents 0.30 x 0.20 m — inside
    the mesh's opening (|y| <= 0.35, |z| <= 0.25 with cut corners) — and the frame's front as the outer rectangle."""
    from dronesim_amd.obstacles import Aperture
    return Aperture((0, 0, 0), (1, 0, 0), (0, 1, 0), (0.30, 0.20), shape, outer=(0.56, 0.40))


# ---- fp64 --------------------------------------------------------------------------------------------------------------------------
def _points(p32, off32):
    q = np.asarray(p32, dtype=np.float32).astype(np.float64)
    return q if off32 is None else q - np.asarray(off32, dtype=np.float32).astype(np.float64)


def _counts(scenes, sid):
    sid = np.asarray(sid, dtype=np.int64)
    look = (sid >= 0) & (sid < scenes.K)
    return look, np.where(look, scenes.count[np.clip(sid, 0, scenes.K - 1)], 0)


def _inside(ap, y, z):
    a, b = (float(x) for x in ap.half)
    if ap.shape == "ellipse":
        rho = np.sqrt((y / a) ** 2 + (z / b) ** 2)
        return rho <= 1.0, np.abs(rho - 1.0) * min(a, b)
    return (np.abs(y) <= a) & (np.abs(z) <= b), np.minimum(np.abs(np.abs(y) - a), np.abs(np.abs(z) - b))


def crossings(prev32, pos32, off32, scenes, sid, ap, travel=TRAVEL):
    """Per drone and slot [n, G]: kind (0 nothing, 1 forward inside, 2 backward inside, 3 forward miss), tau, span = |s1 - s0|,
    and per drone: look (a scene), swept, count, bad (within GUARD of a decision: a plane, a border, the travel)."""
    q0, q1 = _points(prev32, off32), _points(pos32, off32)
    sid = np.asarray(sid, dtype=np.int64)
    n, G = q0.shape[0], scenes.G
    look, cnt = _counts(scenes, sid)
    with np.errstate(invalid="ignore"):
        length = np.linalg.norm(q1 - q0, axis=1)
        swept = np.isfinite(q0).all(1) & np.isfinite(q1).all(1) & (length <= travel)
        bad = look & np.isfinite(length) & (np.abs(length - travel) < GUARD)
    kind, tau, span = np.zeros((n, G), dtype=np.int64), np.zeros((n, G)), np.zeros((n, G))
    c, nrm, u, v = ap.center.astype(np.float64), ap.normal.astype(np.float64), ap.u.astype(np.float64), ap.v
    outer = ap.outer.astype(np.float64) if ap.outer is not None else None
    for g in range(G):
        m = np.nonzero(look & swept & (cnt > g))[0]
        if not len(m):
            continue
        P = scenes.place[sid[m], g].astype(np.float64)
        R, t = P[:, :9].reshape(-1, 3, 3), P[:, 9:]
        d0 = np.einsum("nji,nj->ni", R, q0[m] - t) - c
        d1 = np.einsum("nji,nj->ni", R, q1[m] - t) - c
        s0, s1 = d0 @ nrm, d1 @ nrm
        fw, bw = (s0 < 0) & (s1 >= 0), (s0 >= 0) & (s1 < 0)
        cross = fw | bw
        with np.errstate(divide="ignore", invalid="ignore"):
            tt = np.where(cross, s0 / (s0 - s1), 0.0)
        e = d0 + tt[:, None] * (d1 - d0)
        y, z = e @ u, e @ v
        ins, border = _inside(ap, y, z)
        k = np.where(cross & ins, np.where(fw, 1, 2), 0)
        if outer is not None:
            in_o = (np.abs(y) <= outer[0]) & (np.abs(z) <= outer[1])
            k = np.where(fw & ~ins & in_o, 3, k)
            border = np.minimum(border, np.minimum(np.abs(np.abs(y) - outer[0]), np.abs(np.abs(z) - outer[1])))
        kind[m, g], tau[m, g], span[m, g] = k, tt, np.abs(s1 - s0)
        bad[m] |= (np.abs(s0) < GUARD) | (np.abs(s1) < GUARD) | (cross & (border < GUARD))
    return {"kind": kind, "tau": tau, "span": span, "look": look, "swept": swept, "count": cnt, "bad": bad}


def progress(x, due, laps, wrap, clock=0):
    """The progress rule on what crossings() found: masks, the course state after the query, the passage times written
    ({(slot, drone): time}) and the five fleet counters."""
    kind, tau, cnt = x["kind"], x["tau"], x["count"]
    n, G = kind.shape
    bit = (1 << np.arange(G, dtype=np.int64))[None, :]
    fwd, back, miss = (((kind == k) * bit).sum(1) for k in (1, 2, 3))
    due, laps = np.array(due, dtype=np.int64), np.array(laps, dtype=np.int64)
    times, passes, misses = {}, 0, 0
    for i in np.nonzero((fwd | miss) != 0)[0]:
        last, d = -1.0, int(due[i])
        for _ in range(int(cnt[i])):
            if d < 0 or d >= cnt[i] or kind[i, d] != 1 or not tau[i, d] > last:
                break
            last = tau[i, d]
            times[(d, int(i))] = clock + tau[i, d]
            passes += 1
            d += 1
            if d == cnt[i] and wrap:
                d = 0
                laps[i] += 1
        due[i] = d
        misses += int(0 <= d < cnt[i] and kind[i, d] == 3)
    return {"fwd": fwd, "back": back, "miss": miss, "due": due, "laps": laps, "times": times, "passes": passes,
            "wrong_way": int((kind == 2).sum()), "out_of_order": int((kind == 1).sum()) - passes, "misses": misses,
            "unswept": int((x["look"] & ~x["swept"]).sum()), "written": x["look"]}


def reference(prev32, pos32, off32, scenes, sid, ap, due, laps, wrap=False, clock=0, travel=TRAVEL):
    x = crossings(prev32, pos32, off32, scenes, sid, ap, travel)
    out = progress(x, due, laps, wrap, clock)
    out["x"] = x
    return out


def dense_events(q0, q1, R, t, ap, samples=2001):
    """One chord in one placement's frame, sampled: (sign changes of n.(l - c) from < 0 to >= 0, from >= 0 to < 0, and for the first
    of either the sample index before it): what the closed form must agree with."""
    w = np.linspace(0.0, 1.0, samples)
    pts = q0[None] + w[:, None] * (q1 - q0)[None]
    s = ((pts - t) @ R - ap.center.astype(np.float64)) @ ap.normal.astype(np.float64)
    neg = s < 0
    up, down = np.nonzero(neg[:-1] & ~neg[1:])[0], np.nonzero(~neg[:-1] & neg[1:])[0]
    return up, down, w


# ---- the kernel's arithmetic in float32 ------------------------------------------------------------------------------------------
def restated_tau(prev32, pos32, off32, scenes, sid, ap):
    """tau [n, G] as gate_eval computes it, in float32: q = p - offset, d = q - t, l = R^T d with every product and sum rounded,
    minus c, the two dot products with n, one division (numpy rounds every product and sum where the device contracts some into
    fused multiply-adds).  0 where the float32 signs show no crossing."""
    F = np.float32
    q0, q1 = np.asarray(prev32, dtype=F), np.asarray(pos32, dtype=F)
    if off32 is not None:
        q0, q1 = q0 - np.asarray(off32, dtype=F), q1 - np.asarray(off32, dtype=F)
    sid = np.asarray(sid, dtype=np.int64)
    look, cnt = _counts(scenes, sid)
    tau = np.zeros((q0.shape[0], scenes.G), dtype=F)
    for g in range(scenes.G):
        m = np.nonzero(look & (cnt > g))[0]
        if not len(m):
            continue
        P = scenes.place[sid[m], g]
        cols = [P[:, [k, 3 + k, 6 + k]] for k in range(3)]
        s = []
        for q in (q0, q1):
            d = q[m] - P[:, 9:]
            l = [cc[:, 0] * d[:, 0] + cc[:, 1] * d[:, 1] + cc[:, 2] * d[:, 2] - ap.center[k] for k, cc in enumerate(cols)]
            s.append(ap.normal[0] * l[0] + ap.normal[1] * l[1] + ap.normal[2] * l[2])
        s0, s1 = s
        assert s0.dtype == F
        cross = ((s0 < 0) & (s1 >= 0)) | ((s0 >= 0) & (s1 < 0))
        with np.errstate(divide="ignore", invalid="ignore"):
            tau[m, g] = np.where(cross, s0 / (s0 - s1), F(0))
    return tau


def tau_error(tau_got, x):
    """max over the reference's crossings (kind 1: the ones whose time is recorded) of |tau - tau_ref| |s1 - s0|, in metres."""
    m = x["kind"] == 1
    return float((np.abs(np.asarray(tau_got, dtype=np.float64)[m] - x["tau"][m]) * x["span"][m]).max()) if m.any() else 0.0


# ---- the inputs of the GPU cases -------------------------------------------------------------------------------------------------
def settle(rng, draw, n, scenes, sid, ap, exempt=()):
    """The input rule: draw(rng, idx) -> (prev, pos, off or None); a chord within GUARD of a decision is drawn again.
    -> (prev, pos, off, fraction re-drawn).  `exempt`: drones whose chords are planted by hand and stay."""
    prev, pos, off = draw(rng, np.arange(n))
    redrawn = np.zeros(n, dtype=bool)
    for _ in range(50):
        bad = crossings(prev, pos, off, scenes, sid, ap)["bad"]
        bad[list(exempt)] = False
        if not bad.any():
            return prev, pos, off, float(redrawn.mean())
        redrawn |= bad
        p0, p1, o = draw(rng, np.nonzero(bad)[0])
        prev[bad], pos[bad] = p0, p1
        if off is not None:
            off[bad] = o
    raise AssertionError("the input rule did not settle")


def _unit(rng, k, bias):
    d = rng.normal(size=(k, 3)) + np.array([bias, 0.0, 0.0]) * rng.choice([-1.0, 1.0], (k, 1))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def identity_scene():
    from dronesim_amd.obstacles import ObstacleScenes
    return ObstacleScenes(sr.gate(), np.zeros((1, 1, 3)), np.zeros((1, 1, 3)))


ONE_N, ONE_PARALLEL, ONE_ZERO, ONE_NAN, ONE_TELEPORT, ONE_PLANTED = 700, range(0, 20), range(20, 30), 333, 400, 500


@functools.lru_cache(maxsize=None)
def case_one(shape):
    """GPU case 1: one gate at the identity, 700 drones.  Random chords about the opening (forward, backward, missing), 20
    parallel to the plane, 10 of length zero, one NaN position, one teleport across the aperture, one state planted exactly on
    the plane — and the second query's positions: everybody stays but the planted drone, which moves on."""
    n, scenes, ap = ONE_N, identity_scene(), gate_aperture(shape)
    sid = np.zeros(n, dtype=np.int64)

    def draw(rng, idx):
        k = len(idx)
        mid = rng.uniform([-0.05, -0.6, -0.5], [0.05, 0.6, 0.5], (k, 3))
        d, L, r = _unit(rng, k, 2.0), rng.uniform(0.0, 1.0, (k, 1)), rng.uniform(0.0, 1.0, (k, 1))
        q0, q1 = mid - d * L * r, mid + d * L * (1.0 - r)
        par = np.isin(idx, ONE_PARALLEL)
        q0[par, 0] = q1[par, 0] = 0.125
        zero = np.isin(idx, ONE_ZERO)
        q0[zero] = q1[zero]
        return f32(q0), f32(q1), None
    exempt = (ONE_NAN, ONE_TELEPORT, ONE_PLANTED)
    prev, pos, _, frac = settle(np.random.default_rng(101), draw, n, scenes, sid, ap, exempt)
    pos[ONE_NAN, 1] = np.nan
    prev[ONE_TELEPORT], pos[ONE_TELEPORT] = (-3.0, 0.0, 0.0), (3.0, 0.0, 0.0)
    prev[ONE_PLANTED], pos[ONE_PLANTED] = (-0.25, 0.0, 0.0), (0.0, 0.0625, 0.0625)
    pos2 = pos.copy()
    pos2[ONE_PLANTED] = (0.25, 0.0625, 0.0625)
    return {"scenes": scenes, "scene_id": sid, "ap": ap, "prev": prev, "pos": pos, "pos2": pos2, "off": None, "redrawn": frac}


def _aimed(rng, scenes, sid, idx, offsets):
    """70 % of the chords through a random slot's aperture region +-0.5 m, lengths 0.05 .. 1.5 m; the others anywhere in the box."""
    k = len(idx)
    s = sid[idx]
    look, cnt = _counts(scenes, s)
    d, L, r = _unit(rng, k, 1.5), rng.uniform(0.05, 1.5, (k, 1)), rng.uniform(0.0, 1.0, (k, 1))
    mid = rng.uniform([-4.0, -4.0, 0.0], [4.0, 4.0, 5.0], (k, 3))
    aim = (rng.uniform(size=k) < 0.7) & (cnt > 0)
    g = np.minimum((rng.uniform(size=k) * np.maximum(cnt, 1)).astype(np.int64), scenes.G - 1)
    local = rng.uniform([-0.05, -0.8, -0.7], [0.05, 0.8, 0.7], (k, 3))
    P = np.nan_to_num(scenes.place[np.clip(s, 0, scenes.K - 1), g].astype(np.float64))
    R, t = P[:, :9].reshape(-1, 3, 3), P[:, 9:]
    dl = np.where(aim[:, None], np.einsum("nij,nj->ni", R, d), d)
    mid = np.where(aim[:, None], np.einsum("nij,nj->ni", R, local) + t, mid)
    q0, q1 = mid - dl * L * r, mid + dl * L * (1.0 - r)
    if not offsets:
        return f32(q0), f32(q1), None
    off = f32(rng.uniform(-128.0, 128.0, (k, 3)))
    return f32(q0 + off), f32(q1 + off), off


def _placed_case(scenes, sid, seed, offsets):
    ap = gate_aperture("rect")
    n = len(sid)
    rng = np.random.default_rng(seed)
    draw = lambda rg, idx: _aimed(rg, scenes, sid, idx, offsets)
    prev, pos, off, frac = settle(rng, draw, n, scenes, sid, ap)
    _, cnt = _counts(scenes, sid)
    due = rng.integers(0, cnt + 1)                                  # (count included: some have finished)
    laps = rng.integers(0, 4, n)
    return {"scenes": scenes, "scene_id": sid, "ap": ap, "prev": prev, "pos": pos, "off": off, "redrawn": frac, "due": due,
            "laps": laps}


@functools.lru_cache(maxsize=None)
def case_placed(offsets: bool):
    """GPU case 2: the placements of scenes_ref.case_gates (K = 64, G = 3, n = 2048), random due on entry."""
    d = sr.case_gates(False)
    return _placed_case(d["scenes"], np.asarray(d["scene_id"]), 112 if offsets else 111, offsets)


@functools.lru_cache(maxsize=None)
def case_ragged():
    """GPU case 3: the scenes of scenes_ref.case_ragged (counts 0, 1, 2, 3, 8 of G = 8; ids from -1 to K), with offsets."""
    d = sr.case_ragged()
    return _placed_case(d["scenes"], np.asarray(d["scene_id"]), 121, True)


ROW = (  # (scene, due on entry): scene 0 has its gates in order along the chord, scene 1 in the reverse order
    (0, 0), (1, 0), (0, 1), (0, 3), (1, 2), (0, 2), (1, 1), (0, -1))


@functools.lru_cache(maxsize=None)
def case_row():
    """GPU case 4: three gates 0.2 m apart along x at z = 1, and one chord through all of them from x = -0.1 to x = 0.5."""
    from dronesim_amd.obstacles import ObstacleScenes
    x = np.array([[0.0, 0.2, 0.4], [0.4, 0.2, 0.0]])
    pos = np.zeros((2, 3, 3))
    pos[:, :, 0], pos[:, :, 2] = x, 1.0
    scenes = ObstacleScenes(sr.gate(), pos, np.zeros((2, 3, 3)))
    n = len(ROW)
    sid, due = np.array([r[0] for r in ROW]), np.array([r[1] for r in ROW])
    prev = f32(np.tile([-0.1, 0.03, 1.02], (n, 1)))
    end = f32(np.tile([0.5, -0.02, 0.97], (n, 1)))
    return {"scenes": scenes, "scene_id": sid, "ap": gate_aperture("rect"), "prev": prev, "pos": end, "off": None, "due": due,
            "laps": np.zeros(n, dtype=np.int64)}


def gpu_cases():
    """(name, prev, pos, off, scenes, scene_id, aperture) of every query of the GPU cases on drawn inputs."""
    out = []
    for shape in ("rect", "ellipse"):
        d = case_one(shape)
        out.append((f"one gate {shape}", d["prev"], d["pos"], None, d["scenes"], d["scene_id"], d["ap"]))
    for name, d in (("placed", case_placed(False)), ("placed, offsets", case_placed(True)), ("ragged", case_ragged()),
                    ("row", case_row())):
        out.append((name, d["prev"], d["pos"], d["off"], d["scenes"], d["scene_id"], d["ap"]))
    return out
