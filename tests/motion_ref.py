"""What the moving-scenes tests share (numpy only: the CPU tests use it without a device; tests/README_motion.md).

The reference of a moved table is SceneMotion.place(tau) itself: the fp64 restatement of the law in include/dronesim_amd.h on the
float32 records and base poses the device is given, rounded to float32 once.  Its closed forms are checked by
tests/test_motion_cpu.py; here are the worlds, the motions of every kind, and the tolerance, which is derived, not measured."""
import functools

import numpy as np

from tests import scenes_ref as sr

DT = 1.0 / 48.0
CLOCKS = (0, 1, 7, 2 ** 33)
KINDS = ("translation", "oscillation", "spin", "swing", "all", "static")


def motion_of_kinds(scenes, kinds, seed, vel_zero=False):
    """A SceneMotion whose USED slots take ``kinds`` in turn, in (k, g) order; its ``kinds`` [K, G] names them.  Sizes at which
    clock 7 of DT (0.146 s) moves a gate by decimetres and tenths of a radian; swing <= 1 rad, as the tolerance's middle term
    assumes.  The entries of unused slots are NaN: they are never looked at.  vel_zero: every velocity 0 (the clock of 2^33,
    where vel tau would leave the positions a float32 resolves)."""
    from dronesim_amd.obstacles import SceneMotion
    rng = np.random.default_rng(seed)
    K, G = scenes.K, scenes.G
    used = np.arange(G)[None, :] < scenes.count[:, None]
    rank = np.cumsum(used.ravel()).reshape(K, G) - 1
    names = np.array(list(kinds) + [""])[np.where(used, rank % len(kinds), len(kinds))]
    has = lambda *which: np.isin(names, which)
    axis = rng.normal(size=(K, G, 3))
    axis = (axis / np.linalg.norm(axis, axis=-1, keepdims=True)).astype(np.float32)
    arr = {"velocity": np.where(has("translation", "all")[..., None] & (not vel_zero), rng.uniform(-1.5, 1.5, (K, G, 3)), 0.0),
           "amplitude": np.where(has("oscillation", "all")[..., None], rng.uniform(-0.4, 0.4, (K, G, 3)), 0.0),
           "omega": np.where(has("oscillation", "swing", "all"), rng.uniform(3.0, 6.0, (K, G)), 0.0),
           "phase": np.where(has("oscillation", "swing", "all"), rng.uniform(-1.0, 1.0, (K, G)), 0.0),
           "axis": np.where(has("spin", "swing", "all")[..., None], axis, np.float32(0.0)),
           "rate": np.where(has("spin", "all"), rng.uniform(2.0, 4.0, (K, G)), 0.0),
           "swing": np.where(has("swing", "all"), rng.uniform(0.3, 0.9, (K, G)), 0.0)}
    for v in arr.values():
        v[~used] = np.nan
    m = SceneMotion(scenes, **arr)
    m.kinds = names
    return m


@functools.lru_cache(maxsize=None)
def small_world():
    """K = 3, G = 3, counts (3, 1, 0) of the committed gate: a full scene, a ragged one and an empty one; unused slots NaN."""
    from dronesim_amd.obstacles import ObstacleScenes
    pos, rpy = sr.random_placements(np.random.default_rng(61), 3, 3)
    count = np.array([3, 1, 0])
    unused = np.arange(3)[None, :] >= count[:, None]
    pos[unused], rpy[unused] = np.nan, np.nan
    return ObstacleScenes(sr.gate(), pos, rpy, count)


# the small world has four used slots and there are six kinds: every case runs BOTH assignments, which together hold them all
SMALL_KINDS = (("translation", "oscillation", "spin", "static"), ("swing", "all", "static", "translation"))


def small_motions(vel_zero=False):
    return [motion_of_kinds(small_world(), kinds, 62 + i, vel_zero) for i, kinds in enumerate(SMALL_KINDS)]


@functools.lru_cache(maxsize=None)
def big_world():
    """K = 700, G = 2: 1 400 slots, six blocks of 256 lanes (the last partial); counts 2, 1, 0 in turn."""
    from dronesim_amd.obstacles import ObstacleScenes
    K, G = 700, 2
    pos, rpy = sr.random_placements(np.random.default_rng(63), K, G)
    count = np.array([2, 1, 0] * 234)[:K]
    unused = np.arange(G)[None, :] >= count[:, None]
    pos[unused], rpy[unused] = np.nan, np.nan
    return ObstacleScenes(sr.gate(), pos, rpy, count)


def big_motion(vel_zero=False):
    return motion_of_kinds(big_world(), KINDS, 64, vel_zero)


STRIDE_SLOTS = 2048 * 256          # what one sweep of the move kernel's grid covers (SCM_MAX_BLOCKS x SCM_BLOCK, dsim_scene_motion.hip)


@functools.lru_cache(maxsize=None)
def stride_world():
    """K = 262 400, G = 2: 524 800 slots, 512 more than one sweep of the grid — the only size at which the kernel's grid stride
    takes a second turn.  Every slot used."""
    from dronesim_amd.obstacles import ObstacleScenes
    K, G = 262400, 2
    pos, rpy = sr.random_placements(np.random.default_rng(65), K, G)
    return ObstacleScenes(sr.gate(), pos, rpy)


def box_centre(prototype):
    """The centre of the prototype's box in its own frame, as dsim_scenes_create takes it."""
    t = prototype.triangles.astype(np.float64).reshape(-1, 3)
    return 0.5 * (t.min(0) + t.max(0))


def tolerance(motion, tau, ref):
    """[K, G, 12], NaN in unused slots.  Both sides round one fp64 value to float32, so they differ by an ulp of float32 where the
    fp64 values straddle a rounding border: 2^-23 |ref|.  The fp64 values differ by the phase's rounding — a fused multiply-add on
    one side and not on the other: 2^-51 (|omega tau| + |rate tau|) radians, times the size S of what the angle multiplies — and by
    the last bits of sin, cos and the sums: 1e-12 S.  S = |t0| + |vel| tau + |amp| + |box_c| + 1 for t (and c_task), 1 for R."""
    d = lambda x: np.abs(x.astype(np.float64))
    nrm = lambda x: np.sqrt((x.astype(np.float64) ** 2).sum(-1))
    t0 = motion.scenes.place[..., 9:]
    S_t = nrm(t0) + nrm(motion.velocity) * abs(tau) + nrm(motion.amplitude) + np.linalg.norm(box_centre(motion.scenes.prototype)) + 1.0
    S = np.concatenate([np.ones(ref.shape[:2] + (9,)), np.repeat(S_t[..., None], 3, -1)], -1)
    angle = (d(motion.omega) + d(motion.rate)) * abs(tau)
    return 2.0 ** -23 * np.abs(ref.astype(np.float64)) + 2.0 ** -51 * angle[..., None] * S + 1e-12 * S


def check_table(got, motion, tau, what=""):
    """``got`` [K, G, 12] (DeviceScenes.read()) against SceneMotion.place(tau), entry by entry within :func:`tolerance`; NaN
    exactly in the unused slots; static slots the base table's, bit for bit.  Prints the worst figure before it asserts."""
    ref = motion.place(tau)
    tol = tolerance(motion, tau, ref)
    used = motion.used
    assert got.shape == ref.shape and got.dtype == np.float32
    assert np.isnan(got[~used]).all() and np.isfinite(got[used]).all()
    err = np.abs(got[used].astype(np.float64) - ref[used].astype(np.float64))
    worst = float((err / tol[used]).max()) if used.any() else 0.0
    print(f"moved table {what} tau = {tau:.6g}: max |got - ref| = {err.max():.3e}, worst |got - ref| / tol = {worst:.3f} over "
          f"{int(motion.moving.sum())} moving of {int(used.sum())} used slots")
    assert (err <= tol[used]).all(), worst
    static = used & ~motion.moving
    assert np.array_equal(got[static].view(np.uint32), motion.scenes.place[static].view(np.uint32))
    return worst
