"""The reference of line of sight among the drones (dsim_line_of_sight_drones, LineOfSight(drones=True), the env's
neighbor_sight_drones keyword), numpy only so that the CPU tests use it without a device: the specification in fp64 on the float32
inputs (sight_drones_brute: sight_ref.sight_brute for the world, a brute-force ball-against-segment test over ALL other drones for
the fleet, the minimum frac winning), the ambiguity mask, a float32 restatement of the kernel's arithmetic without a grid
(restated) and one through the walker the camera's and the scanner's references share (walked), and the inputs the GPU cases and
the CPU checks of their conditions share.  tests/README_sight_drones.md.

The rule (include/dronesim_amd.h): the spheres stand at the STORED positions and are met from the stored p_i with d = rel[t][:][i];
the triangles and the plane keep e = p_i - offset_i.  Drone m blocks when its closed ball meets the closed segment: rho^2 <= R^2,
t0 <= min(1, range), t1 >= 0; frac = max(t0, 0).  Drone i never blocks, nor does the slot's own target index[t][i]."""
import functools

import numpy as np

from tests import camera_drones_ref as dr
from tests import camera_ref as cr
from tests import knn_ref as kr
from tests import scan_ref as sf
from tests import sight_ref as sg

AMBIG_REL = dr.AMBIG_REL         # the camera's sphere mask constant: relative closeness of rho to R
AMBIG_S = 1e-3                   # ... and, in units of s, of a ball's end to s = 0 / s = min(1, range), and of two hits to each other
SEG_GROUND = -2


def seg_drone(k):
    return -3 - k


# ---- fp64 brute force ----------------------------------------------------------------------------------------------------------------
def cast_balls(pos, rel, index, radius, cast, rng=1.0):
    """Every cast segment against the ball of every other drone, fp64 on the float32 inputs.  -> dict of [k, n] arrays: frac (inf:
    no ball meets the segment), idx (the world index of the nearest ball, -1), ndot (|n^ . d^| where the segment enters it; 1 for a
    start inside, and where none), second (the frac of the nearest ball of ANOTHER drone, inf), edge (a ball that could win — its
    t0 not beyond (1 + 1e-3) x the nearest's — grazes the segment, or has a root within 1e-3 of s = 0 or its first within 1e-3 of
    s = min(1, range))."""
    p = np.asarray(pos, np.float32).astype(np.float64)
    d_all = np.asarray(rel, np.float32).astype(np.float64)
    R = np.asarray(radius, np.float32).astype(np.float64)
    k, _, n = d_all.shape
    tmax = min(1.0, float(np.float32(rng)))
    target = (R > 0.0) & np.isfinite(p).all(1)
    out = {"frac": np.full((k, n), np.inf), "idx": np.full((k, n), -1, dtype=np.int64), "ndot": np.ones((k, n)),
           "second": np.full((k, n), np.inf), "edge": np.zeros((k, n), bool)}
    who = np.arange(n)
    with np.errstate(all="ignore"):
        for i in range(n):
            c = cast[:, i]
            if not c.any():
                continue
            d = np.where(c[:, None], d_all[:, :, i], np.array([1.0, 0.0, 0.0]))          # [k, 3]
            a = (d * d).sum(1)[:, None]                                                 # [k, 1]
            m = np.where(target[:, None], p - p[i][None, :], 1.0e9)                     # [n, 3] (no target: far away)
            tc = (d @ m.T) / a                                                          # [k, n]
            q = m[None, :, :] - tc[:, :, None] * d[:, None, :]
            rho = np.sqrt((q * q).sum(-1))
            disc = R[None, :] ** 2 - rho * rho
            h = np.sqrt(np.maximum(disc, 0.0) / a)
            t0, t1 = tc - h, tc + h
            may = target[None, :] & (who[None, :] != i) & c[:, None]
            if index is not None:
                may &= who[None, :] != np.asarray(index)[:, i][:, None]
            hit = may & (disc >= 0.0) & (t0 <= tmax) & (t1 >= 0.0)
            f = np.where(hit, np.maximum(t0, 0.0), np.inf)
            j = f.argmin(1)
            best = f[np.arange(k), j]
            got = np.isfinite(best)
            out["frac"][:, i] = best
            out["idx"][:, i] = np.where(got, j, -1)
            f2 = f.copy()
            f2[np.arange(k), j] = np.inf
            out["second"][:, i] = f2.min(1)
            # |n^ . d^| where the segment enters the winner: n = (w + t0 d - c) / R; a start inside the ball has no surface point
            tw = t0[np.arange(k), j]
            nrm = (tw[:, None] * d - m[j]) / R[j][:, None]
            nd = np.abs((nrm * d).sum(1)) / np.sqrt(a[:, 0])
            out["ndot"][:, i] = np.where(got & (tw > 0.0), nd, 1.0)
            w = np.where(got, best, tmax)[:, None] * (1.0 + AMBIG_REL) + 1e-12
            graze = (np.abs(rho - R[None, :]) <= AMBIG_REL * R[None, :]) & (tc > 0.0) & (tc <= w)
            # (a start ON a ball, |t0| <= 1e-3: frac is about 0 either way, and the relative error has no meaning there)
            ends = (disc >= 0.0) & (t0 <= w) & ((np.abs(t1) <= AMBIG_S) | (np.abs(t0 - tmax) <= AMBIG_S) | (np.abs(t0) <= AMBIG_S))
            out["edge"][:, i] = (may & (graze | ends)).any(1)
    return out


def sight_drones_brute(pos, rel, index=None, radius=None, label=None, rng=1.0, **world):
    """What dsim_line_of_sight_drones is specified to give: sight_ref.sight_brute(pos, rel, index, **world) (world: tri / body,
    scenes / scene_id, ground, offsets, or nothing at all) merged with cast_balls — the minimum frac wins.  The same dict as
    sight_brute (blocker -3 - label[m] for a drone), with is_drone (a ball wins), both (a ball AND the world cut the segment), and `ambiguous` the union of sight_brute's mask and the sphere
    mask: cast_balls' edge, and two hits of different blockers within 1e-3 of each other in s (two balls, or a ball and a
    triangle or the plane)."""
    base = sg.sight_brute(pos, rel, index, **world)
    sph = cast_balls(pos, rel, index, radius, base["cast"], rng)
    wins = sph["frac"] < base["frac"]
    frac = np.where(wins, sph["frac"], base["frac"])
    lab = np.arange(np.asarray(pos).shape[0]) if label is None else np.asarray(label)
    blocker = np.where(wins, seg_drone(lab[np.maximum(sph["idx"], 0)]), base["blocker"])
    # the nearest hit of ANOTHER blocker: behind a ball the next ball or the world's hit, behind the world's hit the nearest ball
    other = np.where(wins, np.minimum(sph["second"], base["frac"]), sph["frac"])
    with np.errstate(invalid="ignore"):                        # (inf - inf where neither hits)
        tie = np.isfinite(frac) & np.isfinite(other) & (np.abs(other - frac) <= AMBIG_S)
    out = dict(base)
    out.update(visible=np.where(base["cast"] & ~np.isfinite(frac), 1, 0), blocker=blocker, frac=frac, t=frac,
               ambiguous=base["ambiguous"] | (base["cast"] & (sph["edge"] | tie)), ndot=np.where(wins, sph["ndot"], base["ndot"]),
               is_drone=wins, both=np.isfinite(sph["frac"]) & np.isfinite(base["frac"]))
    return out


# ---- the kernel's arithmetic in float32, without a grid --------------------------------------------------------------------------------
def restated_balls(pos, rel, index, radius, rng=1.0, offsets=None):
    """frac [k, n] (inf: none) of the nearest ball as sight_sphere computes it, operation by operation in float32 (numpy rounds
    every product and sum where the device contracts some into fused multiply-adds and takes 1-ulp reciprocals and square roots),
    over all drones without the grid."""
    F = np.float32
    w = np.asarray(pos, F)
    d_all = np.asarray(rel, F)
    R = np.asarray(radius, F)
    k, _, n = d_all.shape
    tmax = min(F(1.0), F(rng))
    cast = sg.cast_mask(pos, rel, index, offsets)
    who = np.arange(n)
    best = np.full((k, n), np.inf, dtype=F)
    with np.errstate(all="ignore"):
        for i in range(n):
            if not cast[:, i].any():
                continue
            dx, dy, dz = (d_all[:, c, i][:, None] for c in range(3))                      # [k, 1]
            inv_a = F(1.0) / (dx * dx + dy * dy + dz * dz)
            mx, my, mz = (w[None, :, c] - w[i, c] for c in range(3))                      # [1, n]
            tc = (mx * dx + my * dy + mz * dz) * inv_a
            qx, qy, qz = mx - tc * dx, my - tc * dy, mz - tc * dz
            disc = (R * R)[None, :] - (qx * qx + qy * qy + qz * qz)
            h = np.sqrt(np.maximum(disc, F(0.0)) * inv_a)
            t0, t1 = tc - h, tc + h
            t = np.maximum(t0, F(0.0))
            assert t.dtype == np.float32
            hit = (R > 0)[None, :] & (disc >= 0) & (t0 <= tmax) & (t1 >= 0) & (who[None, :] != i)
            if index is not None:
                hit &= who[None, :] != np.asarray(index)[:, i][:, None]
            best[:, i] = np.where(hit, t, F(np.inf)).min(1)
    return np.where(cast, best, F(np.inf)).astype(np.float64)


def restated(c):
    """frac [k, n] of a case as the kernel computes it: sight_ref.restated_sight for the world, restated_balls for the fleet."""
    kw = world_kw(c)
    kw.pop("body", None)
    tri = sg.restated_sight(c["pos"], c["rel"], c.get("index"), **kw)
    return np.minimum(tri, restated_balls(c["pos"], c["rel"], c.get("index"), c["rad"], c.get("rng", 1.0), c.get("offsets")))


def starts_clear(pos, radius, slack=1e-3):
    """[n] bool: drones whose centre lies in no other drone's ball (nor within `slack` R of one): from there the solid-ball rule
    and the camera's surface rule with near = 0 are one rule."""
    p = np.asarray(pos, np.float32).astype(np.float64)
    R = np.asarray(radius, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        dist = np.linalg.norm(p[:, None, :] - p[None, :, :], axis=-1)
    inside = dist <= (1.0 + slack) * R[None, :]
    np.fill_diagonal(inside, False)
    return ~inside.any(1)


def walked(pos, rel, index, radius, grid, who, rng=1.0):
    """frac [k, len(who)] of the drones `who` by the kernels' own route in float32, ray by ray: camera_drones_ref.walk_rays with
    near = 0 and tmax = min(1, range) on grid = (cell, xmin, ymin, nx, ny) — the binning, the 2-D walk, the early stop, the
    outside list.  The slot's target is left out by giving it radius 0 for that ray (binning does not look at radii).  walk_rays
    tests a SURFACE: only for drones of starts_clear() is this the solid-ball rule.  Slow (a Python loop per ray)."""
    F = np.float32
    w = np.asarray(pos, F)
    R = np.asarray(radius, F)
    k = np.asarray(rel).shape[0]
    cast = sg.cast_mask(pos, rel, index)
    out = np.full((k, len(who)), np.inf)
    for col, i in enumerate(who):
        for t in range(k):
            if not cast[t, i]:
                continue
            rad = R.copy()
            if index is not None:
                rad[int(index[t, i])] = F(0.0)
            out[t, col] = dr.walk_rays(w, rad, grid, w[i], np.asarray(rel, F)[t, :, i][None, :], int(i), F(0.0), min(F(1.0), F(rng)))[0][0]
    return out


# the float32 restatement's worst camera_ref.t_error against sight_drones_brute over the inputs of every GPU case (gpu_cases):
# measured by tests/test_sight_drones_cpu.py::test_restated_error_is_what_is_recorded; the kernel is granted 4 x this, the
# project's standing margin for FMA contraction and 1-ulp reciprocals
SIGHT_DRONES_RESTATED_WORST = 1.47e-6
SIGHT_DRONES_TOL = 4.0 * SIGHT_DRONES_RESTATED_WORST
MASK_CAP = 0.01


# ---- the inputs of the GPU cases -----------------------------------------------------------------------------------------------------
MODELS = sf.STACK_MODELS                       # ("tello", "hexa_6DOF_simple"): drone i is MODELS[i % 2]


def radii(n, models=MODELS):
    return dr.type_radii([models[i % len(models)] for i in range(n)])


def main_types():
    """[300] type ids of the main fleet: every eighth drone a hexa (R = 0.202 m), the others tellos (R = 0.052 m).  In this crowd
    (13 drones per cubic metre) a fleet of half hexas has one drone in five standing inside TWO balls, whose blocker at frac = 0
    is anybody's: that alone put 1.6 % of the segments under the mask."""
    return (np.arange(300) % 8 == 0).astype(np.uint8)


def main_radii():
    return dr.type_radii([MODELS[t] for t in main_types()])


def world_kw(c):
    return {key: c[key] for key in ("tri", "body", "scenes", "scene_id", "ground", "offsets") if key in c}


def finish(c):
    c["ref"] = sight_drones_brute(c["pos"], c["rel"], c.get("index"), c["rad"], rng=c.get("rng", 1.0), **world_kw(c))
    return c


def mask_share(ref):
    return sg.mask_share(ref)


def t_error(t, ref):
    """camera_ref.t_error, which is relative to the reference's t, with the hits at frac = 0 taken out first: outside the mask
    the reference reads 0 only for a segment that starts more than 1e-3 (in s) inside a ball, where max(t0, 0) is 0 in any
    arithmetic — so there t must BE 0 (inf otherwise), and the relative error is measured over the rest."""
    t = np.asarray(t, np.float64)
    zero = (ref["t"] == 0.0) & ~ref["ambiguous"]
    if not np.all(t[zero] == 0.0):
        return float("inf")
    return cr.t_error(t, dict(ref, ambiguous=ref["ambiguous"] | zero))


@functools.lru_cache(maxsize=None)
def case_column(ground=False):
    """Collinear A (0), B (1), C (2) on a line along x at z = 1, 1 m and 2.5 m from A, hexas all three; D (3), a tello whose
    centre lies inside B's ball, off the line, and whose slots name A, C and E; E (4), a hexa high above, alone.  A knn-shaped
    record of k = 3 (index -1: unused).  ground: one slot of E aims below the plane through nobody."""
    F = np.float32
    pos = np.array([[0, 0, 1], [1, 0, 1], [2.5, 0, 1], [1.0, 0.15625, 1.09375], [0, 6, 4]], F)
    models = ["hexa_6DOF_simple"] * 3 + ["tello", "hexa_6DOF_simple"]
    rad = dr.type_radii(models)
    index = np.array([[1, 0, 1, 0, 0], [2, 2, 0, 2, -1], [3, 3, 3, 4, -1]], np.int32)
    rel = np.zeros((3, 3, 5), F)
    for t in range(3):
        for i in range(5):
            if index[t, i] >= 0:
                rel[t, :, i] = pos[index[t, i]] - pos[i]
    c = {"pos": pos, "rad": rad, "rel": rel, "index": index, "models": models}
    if ground:
        rel[1, :, 4] = (0.0, 0.0, -8.0)
        index[1, 4] = 0                                        # (any drone off that segment: used, and not in its way)
        c["ground"] = True
    return finish(c)


@functools.lru_cache(maxsize=None)
def main_pos():
    """sight_ref.case_main(0)'s fleet: 300 drones in the box about scene(0), on multiples of 2^-10 m."""
    return sg.case_main(0)["pos"]


MAIN = (("knn16", 0, False), ("knn16", 0, True), ("knn1", 2, False), ("goal32", 0, False), ("goal32", 2, True))   # (record, subdiv, offsets)


@functools.lru_cache(maxsize=None)
def main_record(kind):
    """(rel [k, 3, 300], index or None) of the main case: "knn16" / "knn1": the knn record of radius 1 m as knn_ref.brute states it
    (the device's own record is what the GPU test feeds; on this fleet's 2^-10 m grid its rel_pos are these numbers exactly);
    "goal32": 32 goal segments per drone, sight_ref.draw_targets' vectors to drones within 3 m with the index withheld (so
    every segment ends at the centre of a drone that blocks it unless something else does first)."""
    pos = main_pos()
    if kind == "goal32":
        return sg.draw_targets(1181, pos, 32, 3.0)[0], None
    k = 16 if kind == "knn16" else 1
    ref = kr.brute(pos, 1.0, k)
    rel = np.ascontiguousarray(np.transpose(ref.rel_pos, (1, 2, 0)).astype(np.float32))
    return rel, np.ascontiguousarray(ref.index.T.astype(np.int32))


# per record: the floors on the segments drones block, triangles block, a triangle blocks in front of a drone, and the reverse
FLOORS = {"knn16": (500, 100, 8, 20), "knn1": (5, 2, 0, 0), "goal32": (3000, 1000, 500, 500)}


def main_offsets():
    """[300, 3]: per-drone offsets of multiples of 1/4 m in +-0.5 in x and y (scan_ref's stack offsets): the neighbours' balls stay
    near where the record says the neighbours are, a quarter or a half metre off."""
    ab = np.random.default_rng(7).integers(-2, 3, (300, 2)).astype(np.float64) * 0.25
    return np.concatenate([ab, np.zeros((300, 1))], 1)


@functools.lru_cache(maxsize=None)
def case_main(which):
    """Case 1, MAIN[which]: the mixed fleet (tello, hexa, tello, ...) about scene(subdiv) with one of the records.  With offsets
    the fleet is STORED at p + offset (exact): the triangles see p, the spheres stand — and are met — where the drones are stored,
    so the neighbours' balls move with their own offsets and the record's vectors no longer point at them."""
    kind, subdiv, offsets = MAIN[which]
    rel, index = main_record(kind)
    sc = cr.scene(subdiv)
    c = {"pos": main_pos(), "rad": main_radii(), "rel": rel, "index": index, "sc": sc, "tri": sc.triangles, "body": sc.body, "kind": kind}
    if offsets:
        off = main_offsets()
        c["pos"] = (main_pos().astype(np.float64) + off).astype(np.float32)
        assert np.array_equal(c["pos"] - off.astype(np.float32), main_pos())
        c["offsets"] = off
    return finish(c)


def common_offset_case(which, shift=(64.0, -32.0, 0.0)):
    """case_main(which) (no offsets) stored `shift` away with that one offset for every drone: the same world and the same balls,
    so every output must be the unshifted query's bit for bit (p + shift is exact)."""
    c = dict(case_main(which))
    off = np.tile(np.asarray(shift, np.float64), (300, 1))
    c["pos"] = (c["pos"].astype(np.float64) + off).astype(np.float32)
    assert np.array_equal(c["pos"] - off.astype(np.float32), main_pos())
    c["offsets"] = off
    return c


EDGE_K = 10
EDGE_LOST = 155                   # a drone whose position is not finite
EDGE_LEN = 2.5


@functools.lru_cache(maxsize=None)
def case_edges(zero_type=False):
    """Case 3: scan_ref.case_stack's fleet — 300 level drones on three layers of 10 x 10 at 1 m pitch, every fifth 0.125 m beside
    its line — with goal segments (no index): the six axis directions (dx = 0, dy = 0, both) and four diagonals, 2.5 m long, so
    that a segment passes two drones of its line.  Drone EDGE_LOST has x = NaN.  zero_type: the tellos (even drones) have radius 0:
    no targets, and they still look."""
    F = np.float32
    st = sf.case_stack()["st"]
    pos = st[:, :3].copy()
    pos[EDGE_LOST, 0] = np.nan
    beams = sf.stack_beams() * F(EDGE_LEN)
    rel = np.ascontiguousarray(np.tile(beams[:, :, None], (1, 1, 300)).astype(F))
    rad = radii(300)
    if zero_type:
        rad = rad.copy()
        rad[0::2] = 0.0
    return finish({"pos": pos, "rad": rad, "rel": rel, "index": None, "zero_type": zero_type})


@functools.lru_cache(maxsize=None)
def case_scenes(subdiv):
    """Case 4, scenes + drones: subdiv None: scan_ref.case_scenes' ragged scenes (the gate prototype, counts 0 .. 3, ids from -1
    to K; records in LDS) with its 256 drones; 0 / 2: scan_ref.lattice_scenes(subdiv) under the lattice (2: records through L2).
    16 segments per drone to drones within 3 m, with their index."""
    if subdiv is None:
        c = sf.case_scenes()
        pos, scenes, sid = c["st"][:, :3].copy(), c["scenes"], c["sid"]
    else:
        pos, scenes, sid = sf.lattice()[0][:, :3].copy(), sf.lattice_scenes(subdiv), sf.LATTICE_SCENE_ID
    rel, index = sg.draw_targets(1191, pos, 16, 3.0)
    return finish({"pos": pos, "rad": radii(pos.shape[0]), "rel": rel, "index": index, "scenes": scenes, "scene_id": sid})


@functools.lru_cache(maxsize=None)
def case_plane():
    """Drones + plane, no triangles: the main fleet's knn16 record with every fourth slot aimed 3 m down instead (through the
    plane, unless a drone below hides it first)."""
    rel, index = main_record("knn16")
    rel, index = rel.copy(), index.copy()
    rel[::4] = np.array([0.0, 0.0, -3.0], np.float32)[None, :, None]
    index[::4] = np.where(index[::4] >= 0, index[::4], 0)
    return finish({"pos": main_pos(), "rad": main_radii(), "rel": rel, "index": index, "ground": True})


CHUNK_K = 8
CHUNK_PITCH = 64.0


@functools.lru_cache(maxsize=None)
def chunk_record():
    ref = kr.brute(main_pos(), 1.0, CHUNK_K)
    return (np.ascontiguousarray(np.transpose(ref.rel_pos, (1, 2, 0)).astype(np.float32)), np.ascontiguousarray(ref.index.T.astype(np.int32)))


def chunk_layout(n):
    """The main fleet laid out over n drones: copy c = i // 300 stands (c % 32, c // 32) x 64 m away, stored there with that shift
    as its offset (exact: multiples of 64 m on a 2^-10 m grid below 2 048 m), so that the triangles see the one scene and every
    copy's balls stand 64 m from the next copy's.  The record is the small fleet's with the indices moved into the copy.
    -> (pos [n, 3], offsets [n, 3], rel [k, 3, n], index [k, n], i mod 300)."""
    rel, index = chunk_record()
    i = np.arange(n)
    c, j = i // 300, i % 300
    off = np.stack([(c % 32) * CHUNK_PITCH, (c // 32) * CHUNK_PITCH, np.zeros(n)], 1)
    pos = (main_pos()[j].astype(np.float64) + off).astype(np.float32)
    assert np.array_equal(pos - off.astype(np.float32), main_pos()[j])
    idx = index[:, j]
    idx = np.where(idx >= 0, idx + (c * 300)[None, :], idx).astype(np.int32)
    idx = np.where(idx >= n, -1, idx).astype(np.int32)          # (the last, partial copy: a neighbour that is not there)
    return pos, off, np.ascontiguousarray(rel[:, :, j]), np.ascontiguousarray(idx), j


def gpu_cases():
    """(name, case) of every GPU case that is held against sight_drones_brute: what SIGHT_DRONES_RESTATED_WORST is measured over
    and what the 1 % cap is asserted on.  (The chunk and common-offset cases compare the device with itself on these inputs; the
    env case flies its own fleet and is measured in the GPU test.)"""
    yield "column", case_column(False)
    yield "column, plane", case_column(True)
    for w in range(len(MAIN)):
        yield f"main {MAIN[w]}", case_main(w)
    yield "edges", case_edges(False)
    yield "edges, a type of radius 0", case_edges(True)
    for s in (None, 0, 2):
        yield f"scenes {s}", case_scenes(s)
    yield "drones and the plane", case_plane()
