"""The reference of line of sight (dsim_line_of_sight, LineOfSight, the env's neighbor_sight keyword), numpy only so that the CPU
tests use it without a device: the specification in fp64 on the float32 inputs (sight_brute: camera_ref.cast per drone over ALL
triangles, no grid, no walk), a float32 restatement of the kernel's own arithmetic from which the tests' tolerance is derived
(restated_sight, from scan_ref's pieces), and the inputs the GPU cases and the CPU checks of their conditions share.
tests/README_sight.md.

The segment (include/dronesim_amd.h): e + s d, s in [0, 1], e = p_i - offset_i, d = rel[t][:][i] as given."""
import functools

import numpy as np

from tests import camera_ref as cr
from tests import knn_ref as kr
from tests import scan_ref as sf
from tests import scenes_ref as sr

SEG_GROUND = -2
_NO_TRI = np.zeros((0, 3, 3), dtype=np.float32)


def cast_mask(pos, rel, index=None, offsets=None):
    """[k, n] bool: the slots that are cast — index not negative (or None), e finite (in float32, as the kernel forms it), d
    finite, not zero, |d|^2 finite in float32."""
    F = np.float32
    p = np.asarray(pos, F)
    d = np.asarray(rel, F)
    with np.errstate(all="ignore"):
        e = p if offsets is None else p - np.asarray(offsets, F)
        l2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    ok = np.isfinite(e).all(1)[None, :] & np.isfinite(d).all(1) & (d != 0).any(1) & np.isfinite(l2)
    if index is not None:
        ok &= np.asarray(index) >= 0
    return ok


# ---- fp64 brute force ----------------------------------------------------------------------------------------------------------------
def sight_brute(pos, rel, index=None, tri=None, body=None, scenes=None, scene_id=None, ground=False, offsets=None):
    """What dsim_line_of_sight is specified to give, in fp64 on the float32 inputs: pos [n, 3], rel [k, 3, n], index [k, n] or
    None, tri / body an unplaced set or scenes / scene_id a placed one (neither: no triangles), offsets [n, 3] or None.  Returns a
    dict of [k, n] arrays: visible (0 / 1), blocker (body — instance-major on scenes —, -1, -2 the plane), frac (inf: clear or
    not cast; also under the name t, for camera_ref.t_error), ambiguous (camera_ref.cast's mask), ndot, cast."""
    pos = np.asarray(pos, np.float32)
    rel = np.asarray(rel, np.float32)
    k, _, n = rel.shape
    cast = cast_mask(pos, rel, index, offsets)
    out = {"visible": np.zeros((k, n), dtype=np.int64), "blocker": np.full((k, n), -1, dtype=np.int64), "frac": np.full((k, n), np.inf),
           "ambiguous": np.zeros((k, n), bool), "ndot": np.ones((k, n)), "cast": cast}
    if tri is not None:
        tri = np.asarray(tri, np.float32)
    placed = {}
    for i in range(n):
        c = cast[:, i]
        if not c.any():
            continue
        e = pos[i].astype(np.float64) - (0.0 if offsets is None else np.asarray(offsets[i], np.float32).astype(np.float64))
        d = np.where(c[:, None], rel[:, :, i].astype(np.float64), np.array([1.0, 0.0, 0.0]))     # (a slot that is not cast: any ray, dropped below)
        t_i, b_i = _NO_TRI, 0
        if tri is not None:
            t_i, b_i = tri, body
        elif scenes is not None:
            s = int(scene_id[i])
            if 0 <= s < scenes.K and scenes.count[s] > 0:
                if s not in placed:
                    placed[s] = sr.placed_triangles(scenes, s)
                t_i, b_i = placed[s]
        r = cr.cast(t_i, b_i, e, d, 0.0, 1.0, ground)
        hit = np.isfinite(r["t"])
        out["visible"][:, i] = np.where(c & ~hit, 1, 0)
        out["blocker"][:, i] = np.where(c & hit, r["seg"], -1)
        out["frac"][:, i] = np.where(c, r["t"], np.inf)
        out["ambiguous"][:, i] = c & r["ambiguous"]
        out["ndot"][:, i] = np.where(c, r["ndot"], 1.0)
    out["t"] = out["frac"]
    return out


# ---- the kernel's arithmetic in float32 ----------------------------------------------------------------------------------------------
def restated_sight(pos, rel, index=None, tri=None, scenes=None, scene_id=None, ground=False, offsets=None, chunk=64):
    """frac [k, n] (inf: clear or not cast) as the kernel computes it, operation by operation in float32 (numpy rounds every product
    and sum where the device contracts some into fused multiply-adds and takes 1-ulp reciprocals), over all triangles without a
    grid: e = p - offset, d = rel as given, the plane, the triangle test of scan_ref._tri32 (on scenes by the placed route of
    scan_ref.restated_scan: subtract, rotate), near = 0 and far = 1."""
    F = np.float32
    w = np.asarray(pos, F)
    e = w if offsets is None else w - np.asarray(offsets, F)
    d = np.ascontiguousarray(np.transpose(np.asarray(rel, F), (2, 0, 1)))          # [n, k, 3]
    n, k = d.shape[:2]
    with np.errstate(all="ignore"):
        ray = (np.abs(e) <= F(3.0e38)).all(1)[:, None] & (np.abs(d) <= F(3.0e38)).all(-1) & (d != 0).any(-1) & \
              (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2] <= F(3.0e38))
        if index is not None:
            ray &= (np.asarray(index) >= 0).T
        dd = np.where(ray[..., None], d, F(0.0)).astype(F)                          # (what is not cast tests nothing)
        ee = np.where(np.isfinite(e), e, F(0.0)).astype(F)
        near, far = F(0.0), F(1.0)
        best = np.full((n, k), np.inf, dtype=F)
        if ground:
            tg = -ee[:, 2][:, None] / dd[..., 2]
            best = np.where((tg >= near) & (tg <= far), tg, best)
        if tri is not None:
            rec = sf._records(tri)
            for k0 in range(0, n, chunk):
                best[k0:k0 + chunk] = np.minimum(best[k0:k0 + chunk], sf._tri32(rec, ee[k0:k0 + chunk], dd[k0:k0 + chunk], near, far))
        if scenes is not None:
            rec = sf._records(scenes.prototype.triangles)
            sid = np.asarray(scene_id, np.int64)
            for s in range(scenes.K):
                m = np.nonzero(sid == s)[0]
                for g in range(int(scenes.count[s])):
                    P = scenes.place[s, g]
                    c = [P[[j, 3 + j, 6 + j]] for j in range(3)]                # column j of R
                    for k0 in range(0, len(m), chunk):
                        mm = m[k0:k0 + chunk]
                        tx, ty, tz = ee[mm, 0] - P[9], ee[mm, 1] - P[10], ee[mm, 2] - P[11]
                        le = np.stack([cj[0] * tx + cj[1] * ty + cj[2] * tz for cj in c], -1)
                        ld = np.stack([cj[0] * dd[mm, :, 0] + cj[1] * dd[mm, :, 1] + cj[2] * dd[mm, :, 2] for cj in c], -1)
                        assert le.dtype == np.float32 and ld.dtype == np.float32
                        best[mm] = np.minimum(best[mm], sf._tri32(rec, le, ld, near, far))
    return np.where(ray, best, F(np.inf)).T.astype(np.float64)


# the float32 restatement's worst camera_ref.t_error against sight_brute over the inputs of every GPU case (restated_inputs):
# measured by tests/test_sight_cpu.py::test_restated_error_is_what_is_recorded; the kernel is granted 4 x this, the project's
# standing margin for FMA contraction and 1-ulp reciprocals
SIGHT_RESTATED_WORST = 3.87e-6
SIGHT_TOL = 4.0 * SIGHT_RESTATED_WORST
MASK_CAP = 0.01


# ---- the inputs of the GPU cases -----------------------------------------------------------------------------------------------------
BOX_LO, BOX_HI = (1.0, -1.5, 0.2), (4.5, 1.8, 2.2)
MAIN = ((0, 8, 3.0, 141, 200), (0, 16, 4.0, 142, 300), (2, 8, 3.0, 143, 100))       # (subdiv, k, within [m], seed, floor of blocked)


def draw_targets(seed, pos, k, within):
    """(rel [k, 3, n] float32, index [k, n] int32): for every drone k others drawn (seeded) among those within `within` metres,
    without repetition where there are k of them; rel the float32 differences p_j - p_i."""
    rng = np.random.default_rng(seed)
    p = np.asarray(pos, np.float32)
    n = p.shape[0]
    d = np.linalg.norm(p[:, None, :].astype(np.float64) - p[None, :, :], axis=-1)
    np.fill_diagonal(d, np.inf)
    index = np.zeros((k, n), dtype=np.int32)
    for i in range(n):
        cand = np.nonzero(d[i] < within)[0]
        assert cand.size > 0
        index[:, i] = rng.choice(cand, k, replace=cand.size < k)
    rel = np.ascontiguousarray(np.transpose(p[index] - p[None, :, :], (0, 2, 1)))
    assert rel.dtype == np.float32 and rel.shape == (k, 3, n)
    return rel, index


def _world_kw(c):
    return {key: c[key] for key in ("tri", "body", "scenes", "scene_id", "ground", "offsets") if key in c}


def _finish(c):
    c["ref"] = sight_brute(c["pos"], c["rel"], c.get("index"), **_world_kw(c))
    return c


@functools.lru_cache(maxsize=None)
def case_main(which):
    """Case 1, MAIN[which]: scan_ref.draw_fleet in the box about scene(subdiv), n = 300 (two tiles, the second with 44 live lanes;
    192 on scene(2)), k targets each among the drones within 3 m (4 m)."""
    subdiv, k, within, seed, _ = MAIN[which]
    n = 300 if subdiv == 0 else 192
    pos = sf.draw_fleet(seed, n, lo=BOX_LO, hi=BOX_HI)[:, :3].copy()
    sc = cr.scene(subdiv)
    rel, index = draw_targets(seed + 1000, pos, k, within)
    return _finish({"pos": pos, "rel": rel, "index": index, "sc": sc, "tri": sc.triangles, "body": sc.body, "subdiv": subdiv})


KNN = ((1.0, 16), (1.0, 1))                     # (radius, k) of the knn-record case


@functools.lru_cache(maxsize=None)
def case_knn(which):
    """Case 2: the knn record of case_main(0)'s fleet as knn_ref.brute states it (the device's own record is what the GPU test
    feeds; on this fleet's 2^-10 m grid its rel_pos are these numbers exactly): sparse drones leave slots unused."""
    radius, k = KNN[which]
    c = case_main(0)
    ref = kr.brute(c["pos"], radius, k)
    rel = np.ascontiguousarray(np.transpose(ref.rel_pos, (1, 2, 0)).astype(np.float32))
    index = np.ascontiguousarray(ref.index.T.astype(np.int32))
    return _finish({"pos": c["pos"], "rel": rel, "index": index, "sc": c["sc"], "tri": c["tri"], "body": c["body"], "radius": radius, "k": k})


EDGE_K = 8


@functools.lru_cache(maxsize=None)
def case_edges(subdiv=0):
    """Case 3, one table of (name, position, EDGE_K slots) about scene(subdiv).  The eyes of scan_ref.case_edges (on cell planes,
    on the box's faces, outside a slab, and the three aimed at the rotated box so that axis segments along cell planes also HIT)
    with the six axis directions 6 m long (two components exactly 0; from a face they cross the whole box, from off_corner four of
    them lie wholly outside it), a zero rel and a valid rel under index -1.  Then: a segment that ends short of the wall it points
    at and one that goes on through it (0.9 and 1.5 of the reference's own distance from aim_back along -x); a drone far outside
    with segments wholly outside; nan, inf, a component of 2e19 (its square overflows), a component of 1e-25 (its square
    underflows: cast all the same); two drones whose position is not finite, with valid rels."""
    F = np.float32
    sc = cr.scene(subdiv)
    edge = sf.case_edges(subdiv)
    eyes = {}
    for (e, _), row in zip(edge["names"], edge["st"]):
        eyes.setdefault(e, row[:3].copy())
    axis6 = sf.AXIS_BEAMS * F(6.0)
    rows = []
    for name, eye in eyes.items():
        rel = np.concatenate([axis6, np.zeros((1, 3), F), np.array([[1.0, 0.5, 0.25]], F)])
        rows.append((name, eye, rel, np.array([1, 1, 1, 1, 1, 1, 1, -1])))
    back = eyes["aim_back"]
    far_hit = cr.cast(sc.triangles, sc.body, back.astype(np.float64), np.array([[-1.0, 0.0, 0.0]]), 0.0, 100.0)["t"][0]
    assert np.isfinite(far_hit) and far_hit > 0.25
    wall = np.zeros((EDGE_K, 3), F)
    wall[:, 0] = -F(far_hit) * np.array([0.9, 1.5, 0.5, 1.01, 0.99, 2.0, 0.1, 4.0], F)
    rows.append(("wall", back, wall, np.ones(EDGE_K, dtype=int)))
    out = np.array([[1, 1, 0.5], [-1, 0, 0], [0, 3, 0], [0, 0, -0.5], [2, -2, 0.25], [0.5, 0, 0], [0, -0.5, 0], [1, 1, 1]], F)
    rows.append(("outside", np.array([10.0, 10.0, 1.0], F), out, np.ones(EDGE_K, dtype=int)))
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [2e19, 0, 0], [1e-25, 0, 0], [0, 0, -np.inf], [1, np.nan, 1], [0, 2e19, 1], [1, 0, 0]], F)
    rows.append(("bad rel", eyes["corner"], bad, np.ones(EDGE_K, dtype=int)))
    good = np.tile(np.array([[1.0, 0.25, 0.125]], F), (EDGE_K, 1))
    rows.append(("nan position", np.array([np.nan, 0.0, 1.0], F), good, np.ones(EDGE_K, dtype=int)))
    rows.append(("inf position", np.array([2.0, np.inf, 1.0], F), good, np.ones(EDGE_K, dtype=int)))
    names = [r[0] for r in rows]
    pos = np.stack([r[1] for r in rows]).astype(F)
    rel = np.ascontiguousarray(np.stack([r[2] for r in rows], -1).astype(F))          # [k, 3, n]
    index = np.ascontiguousarray(np.stack([r[3] for r in rows], -1).astype(np.int32))
    return _finish({"names": names, "pos": pos, "rel": rel, "index": index, "sc": sc, "tri": sc.triangles, "body": sc.body})


@functools.lru_cache(maxsize=None)
def case_scenes():
    """Case 5: scan_ref.case_scenes — the gate prototype, K = 6 with counts (0, 1, 2, 3, 3, 3), n = 256, scene ids from -1 to K —
    with 8 targets each among the drones within 3 m."""
    c = sf.case_scenes()
    pos = c["st"][:, :3].copy()
    rel, index = draw_targets(151, pos, 8, 3.0)
    return _finish({"pos": pos, "rel": rel, "index": index, "scenes": c["scenes"], "scene_id": c["sid"]})


@functools.lru_cache(maxsize=None)
def case_lattice_scenes(subdiv):
    """... and scan_ref.lattice_scenes(subdiv), two scenes of one placement of scene(subdiv) each, under scan_ref's lattice of 256
    drones with the scene ids -1, 0, 1, 2 (= K) in turn: 8 targets each among the drones within 3 m."""
    pos = sf.lattice()[0][:, :3].copy()
    rel, index = draw_targets(152 + subdiv, pos, 8, 3.0)
    return _finish({"pos": pos, "rel": rel, "index": index, "scenes": sf.lattice_scenes(subdiv), "scene_id": sf.LATTICE_SCENE_ID})


def identity_scenes(subdiv):
    """scene(subdiv) as one scene of one placement at the origin, unrotated."""
    from dronesim_amd.obstacles import ObstacleScenes
    return ObstacleScenes(cr.scene(subdiv), np.zeros((1, 1, 3)), np.zeros((1, 1, 3)))


@functools.lru_cache(maxsize=None)
def case_ground(with_set):
    """Case 6: case_main(0)'s fleet, every drone with 8 targets of which four lie below the plane (z = -0.25 .. -1) and four
    above it, beside and beyond the scene; with the set, or the plane alone."""
    c = case_main(0)
    pos = c["pos"]
    n = pos.shape[0]
    rng = np.random.default_rng(161)
    tgt = np.round(rng.uniform([0.0, -2.5, 0.25], [5.5, 2.5, 2.5], (8, n, 3)) * 1024.0) / 1024.0
    tgt[:4, :, 2] = -np.round(rng.uniform(0.25, 1.0, (4, n)) * 1024.0) / 1024.0
    rel = np.ascontiguousarray(np.transpose(tgt.astype(np.float32) - pos[None, :, :], (0, 2, 1)))
    d = {"pos": pos, "rel": rel, "index": None, "ground": True, "below": np.arange(8) < 4}
    if with_set:
        d.update(sc=c["sc"], tri=c["tri"], body=c["body"])
    return _finish(d)


def gpu_cases():
    """(name, case) of every GPU case that is held against sight_brute: what SIGHT_RESTATED_WORST is measured over and what the
    1 % cap is asserted on.  (The offsets, identity-placement and chunk cases compare the device with itself on these inputs; the
    env case flies its own fleet and is measured in the GPU test.)"""
    for w in range(len(MAIN)):
        yield f"main {MAIN[w][:2]}", case_main(w)
    for w in range(len(KNN)):
        yield f"knn record {KNN[w]}", case_knn(w)
    yield "edges", case_edges(0)
    yield "edges, subdiv 2", case_edges(2)
    yield "scenes", case_scenes()
    yield "lattice scenes", case_lattice_scenes(0)
    yield "lattice scenes, subdiv 2", case_lattice_scenes(2)
    yield "ground, set", case_ground(True)
    yield "ground alone", case_ground(False)


def restated(c):
    kw = _world_kw(c)
    kw.pop("body", None)
    return restated_sight(c["pos"], c["rel"], c.get("index"), **kw)


def mask_share(ref):
    """The share of the cast segments under the ambiguity mask."""
    return float(ref["ambiguous"].sum()) / max(int(ref["cast"].sum()), 1)
