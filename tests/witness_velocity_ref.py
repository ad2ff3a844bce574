"""The reference of the witness-velocity tests (numpy only, so the CPU tests use it without a device; tests/README_witness_velocity.md).

The twist table against SceneMotion.twist(tau), the fp64 derivative of the law, within a DERIVED bar (twist_tolerance).  The
velocity of a witness against fp64 on the float32 tables the device holds:  v_ref = t' + w x (w* - t), with w* from
witness_ref.brute_witness_scenes on the world as it stands at that scene time and (t', w) the twist table's floats.  A float32
restatement of the kernel's tail (r = R (l + v_l), v = t' + w x r, every product and sum rounded), whose recorded worst error
gives the kernel's tolerance, the masks of witness_ref, and the inputs the GPU cases and the CPU checks share."""
import functools

import numpy as np

from tests import motion_ref as mr
from tests import scenes_ref as sr
from tests import witness_ref as wr

CLOCK = 7                                  # the GPU cases stand at clock 7 of motion_ref.DT: 0.146 s of scene time
TAU = CLOCK * mr.DT
# the float32 restatement's worst |v32 - v_ref| outside the strict mask over the inputs of the GPU cases (the gates with and
# without offsets, the soup): tests/test_witness_velocity_cpu.py::test_restated_velocity_error_is_what_is_recorded — not above the
# record, the record not padded by more than 2 %.  The kernel is granted 4 x it.
RESTATED_VEL = 5.04e-6
TOL_VEL = 4.0 * RESTATED_VEL
CASES = (("gates", False), ("gates", True), ("soup", False))
SEED = {"gates": 71, "soup": 72}


# ---- the twist table -----------------------------------------------------------------------------------------------------------------
def twist_ref(motion, tau):
    """fp64 [K, G, 8] as dsim_scenes_move_twist lays it out: (t'.xyz, 0, w.xyz, 0); zeros in static slots, NaN in unused ones."""
    v, w = motion.twist(tau)
    z = np.where(np.isnan(v[..., :1]), np.nan, 0.0)
    return np.concatenate([v, z, w, z], -1)


def twist_tolerance(motion, tau, ref):
    """[K, G, 8], in the manner of motion_ref.tolerance.  Both sides round one fp64 value to float32: 2^-23 |ref| where the two
    straddle a rounding border.  The fp64 values differ by the phase's rounding, a fused multiply-add on one side and not on the
    other: 2^-51 (|omega| + |rate|) |tau| radians, times the size S of what the cosine multiplies; and by the last bits of the
    cosine, the products and the sums: 1e-12 S.  S = |vel| + |amp| |omega| + 1 for t', |rate| + |swing| |omega| + 1 for w."""
    d = lambda x: np.abs(x.astype(np.float64))
    nrm = lambda x: np.sqrt((x.astype(np.float64) ** 2).sum(-1))
    S_t = nrm(motion.velocity) + nrm(motion.amplitude) * d(motion.omega) + 1.0
    S_w = d(motion.rate) + d(motion.swing) * d(motion.omega) + 1.0
    S = np.concatenate([np.repeat(S_t[..., None], 4, -1), np.repeat(S_w[..., None], 4, -1)], -1)
    angle = (d(motion.omega) + d(motion.rate)) * abs(tau)
    return 2.0 ** -23 * np.abs(ref) + 2.0 ** -51 * angle[..., None] * S + 1e-12 * S


def check_twist(got, motion, tau, sentinel, what=""):
    """``got`` float32 [K, G, 8], a table that held ``sentinel`` everywhere before the move: the moving slots within
    :func:`twist_tolerance` of :func:`twist_ref` (their two pads exact zeros), every other slot still the sentinel."""
    ref = twist_ref(motion, tau)
    tol = twist_tolerance(motion, tau, ref)
    mv = motion.moving
    assert got.shape == ref.shape and got.dtype == np.float32
    err = np.abs(got[mv].astype(np.float64) - ref[mv])
    worst = float((err / tol[mv]).max()) if mv.any() else 0.0
    print(f"twist table {what} tau = {tau:.6g}: max |got - ref| = {err.max(initial=0.0):.3e}, worst |got - ref| / tol = {worst:.3f} "
          f"over {int(mv.sum())} moving slots; largest |t'| {np.abs(ref[mv][:, :3]).max(initial=0.0):.3f} m/s, "
          f"|w| {np.abs(ref[mv][:, 4:7]).max(initial=0.0):.3f} rad/s")
    assert (err <= tol[mv]).all(), worst
    assert np.all(got[mv][:, [3, 7]] == 0.0)
    assert np.array_equal(got[~mv].view(np.uint32), np.full_like(got[~mv], sentinel).view(np.uint32))
    return worst


# ---- fp64: the velocity of the reference's witness -----------------------------------------------------------------------------------
def velocity_ref(ref, scenes_now, scene_id, twist32):
    """(v_ref [n, 3], |w| [n], slot [n]) of a witness reference dict on ``scenes_now`` (the world as the device holds it, float32
    widened): t' + w x (w* - t) of the slot that holds w*, from the float32 twist table [K, G, 8]; zeros without a witness."""
    T = scenes_now.prototype.n_tri
    sid = np.clip(np.asarray(scene_id, dtype=np.int64), 0, scenes_now.K - 1)
    slot = np.where(ref["in"], ref["tri"] // T, 0)
    tw = np.nan_to_num(np.asarray(twist32, dtype=np.float32)[sid, slot].astype(np.float64))
    t = np.nan_to_num(scenes_now.place[sid, slot, 9:].astype(np.float64))
    v = tw[:, 0:3] + np.cross(tw[:, 4:7], ref["w"] - t)
    inr = ref["in"][:, None]
    return np.where(inr, v, 0.0), np.where(ref["in"], np.linalg.norm(tw[:, 4:7], axis=1), 0.0), slot


def bars(ref, wnorm):
    """(bar [n], checked [n]): TOL_VEL outside the strict mask; inside it but outside the tie mask the witness may sit up to the
    position bound 2 (2 sqrt(2 d E) + E) from the reference's, which the angular speed turns into velocity; inside the tie mask
    nothing is asked."""
    d = np.where(ref["in"], ref["d"], 0.0)
    pos = 2.0 * (2.0 * np.sqrt(2.0 * d * wr.E) + wr.E)
    return np.where(ref["strict"], TOL_VEL + wnorm * pos, TOL_VEL), ref["in"] & ~ref["tie"]


def check_velocity(vel, has, ref, scenes_now, scene_id, twist32, what, sure=None):
    """``vel`` [n, 3] and ``has`` [n] (nearest >= 0) of the device against the reference: zeros exactly without a witness, within
    the bars elsewhere.  Prints the worst figures before it asserts.  -> the worst error outside the strict mask."""
    vref, wnorm, _ = velocity_ref(ref, scenes_now, scene_id, twist32)
    bar, checked = bars(ref, wnorm)
    sure = np.ones(len(has), bool) if sure is None else sure
    np.testing.assert_array_equal(has[sure], ref["in"][sure])
    vel = np.asarray(vel, dtype=np.float64)
    assert np.all(vel[~has] == 0.0)
    m = checked & has
    err = np.linalg.norm(vel - vref, axis=1)
    plain = m & ~ref["strict"]
    worst, ratio = float(err[plain].max(initial=0.0)), float((err[m] / bar[m]).max(initial=0.0))
    tie, strict = wr.mask_shares(ref)
    print(f"witness velocity {what}: |v - v_ref| outside the strict mask {worst:.3e} (TOL_VEL {TOL_VEL:.3e}), worst |v - v_ref| / bar "
          f"{ratio:.3f} over {int(m.sum())} drones; largest |v_ref| {np.linalg.norm(vref, axis=1).max(initial=0.0):.2f} m/s; tie mask "
          f"{tie:.4f}, strict mask {strict:.4f}")
    assert tie <= wr.TIE_CAP and strict <= wr.STRICT_CAP
    assert (err[m] <= bar[m]).all(), ratio
    return worst


# ---- the kernel's tail in float32 ----------------------------------------------------------------------------------------------------
def restated_velocity_scenes(p32, scenes, scene_id, rad, margin, twist32, off32=None, chunk=256):
    """(vel [n, 3] float32, tri [n], in [n]) as the placed kernel computes them: witness_ref.restated_witness_scenes' search (the
    local point l of every placement, the walk, a strict < across placements in slot order, tri_closest at the winner's l), then
    the new tail with every product and sum rounded: u = l + v_l, r = sum_k col_k u_k, v = t' + (w x r)."""
    q = np.asarray(p32, dtype=np.float32)
    if off32 is not None:
        q = q - np.asarray(off32, dtype=np.float32)
    r = np.asarray(rad, dtype=np.float32)
    sid = np.asarray(scene_id, dtype=np.int64)
    rec = sr.records32(scenes.prototype.triangles)
    n, T = q.shape[0], scenes.prototype.n_tri
    valid = (sid >= 0) & (sid < scenes.K)
    cnt = np.where(valid, scenes.count[np.clip(sid, 0, scenes.K - 1)], 0)
    best, tri, slot = np.full(n, np.inf, dtype=np.float32), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    loc = np.zeros((n, 3), dtype=np.float32)
    for g in range(scenes.G):
        m = np.nonzero(cnt > g)[0]
        for k0 in range(0, len(m), chunk):
            mm = m[k0:k0 + chunk]
            P = scenes.place[sid[mm], g]
            d = q[mm] - P[:, 9:]
            l = np.stack([P[:, k] * d[:, 0] + P[:, 3 + k] * d[:, 1] + P[:, 6 + k] * d[:, 2] for k in range(3)], 1)
            d2 = sr.tri_dist2_32(rec, l)
            b, t = d2.min(1), d2.argmin(1)
            better = b < best[mm]
            best[mm], tri[mm], slot[mm] = np.where(better, b, best[mm]), np.where(better, t, tri[mm]), np.where(better, g, slot[mm])
            loc[mm] = np.where(better[:, None], l, loc[mm])
    inr = (r > 0) & np.isfinite(best) & ((np.sqrt(best) - r) < np.float32(margin))
    vel = np.zeros((n, 3), dtype=np.float32)
    ix = np.nonzero(inr)[0]
    if len(ix):
        v = wr.tri_closest_32(rec, tri[ix], loc[ix])
        u = loc[ix] + v
        P = scenes.place[sid[ix], slot[ix]]
        rr = [P[:, 3 * k] * u[:, 0] + P[:, 3 * k + 1] * u[:, 1] + P[:, 3 * k + 2] * u[:, 2] for k in range(3)]
        tw = np.asarray(twist32, dtype=np.float32)[sid[ix], slot[ix]]
        td, om = tw[:, 0:3], tw[:, 4:7]
        vel[ix] = np.stack([td[:, 0] + (om[:, 1] * rr[2] - om[:, 2] * rr[1]), td[:, 1] + (om[:, 2] * rr[0] - om[:, 0] * rr[2]),
                            td[:, 2] + (om[:, 0] * rr[1] - om[:, 1] * rr[0])], 1)
    assert vel.dtype == np.float32
    return vel, np.where(inr, slot * T + tri, -1), inr


# ---- the inputs of the GPU cases -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def moving_case(name, offsets=False):
    """(case dict of scenes_ref, SceneMotion of every kind of motion_ref.KINDS on its scenes): the gates (K = 64, G = 3, 2 048
    robobees: the LDS instance) with and without offsets of +-128 m, the soup (K = 4, G = 2, 512 hexa_6DOF: the L2 instance)."""
    d = sr.case_gates(offsets) if name == "gates" else sr.case_soup()
    return d, mr.motion_of_kinds(d["scenes"], mr.KINDS, SEED[name])


@functools.lru_cache(maxsize=None)
def host_world(name, offsets=False):
    """What the CPU checks stand on: (case, motion, the world at TAU as SceneMotion.snapshot gives it, the float32 twist table of
    SceneMotion.twist, the witness reference on them).  The GPU cases take both tables from the device instead."""
    d, m = moving_case(name, offsets)
    now = m.snapshot(TAU)
    twist32 = np.nan_to_num(twist_ref(m, TAU)).astype(np.float32)
    ref = wr.brute_witness_scenes(d["pos"], now, d["scene_id"], d["rad"], d["margin"], d["off"])
    return d, m, now, twist32, ref


def witnesses_per_kind(motion, ref, scene_id, n_tri):
    """How many of the reference's witnesses lie on a placement of each kind of motion."""
    sid = np.asarray(scene_id, dtype=np.int64)[ref["in"]]
    slot = ref["tri"][ref["in"]] // n_tri
    names = motion.kinds[sid, slot]
    return {k: int((names == k).sum()) for k in mr.KINDS}
