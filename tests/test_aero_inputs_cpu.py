"""The inputs of tests/test_gpu_aero_edges.py, checked without a device: what the drag (P6) and ground-effect (P7) tests on
the GPU take for granted about the cases tests/util.py builds (aero_gate_cases, aero_height_cases, aero_drag_cases), and the
POWER of the comparisons they make — every check here uses the fp64 oracle alone.

  - the gate cases lie where the kernel's fp32 predicate and the oracle's fp64 one must agree, at the start and at every
    later sub-step of every launch the device tests make from them: no case is excluded from any device comparison;
  - the height cases hold what they claim (z at the clip to the ulp, rotors on both sides of it);
  - a kernel that drops a term, takes the wrong previous action or flips the gate differs from the oracle by more than ten
    times the bar the device tests apply to that drone, on at least 90 % of the drones of the class concerned.
"""
import math

import numpy as np
import pytest

from dronesim_amd import params
from oracle import oracle as orc
from tests.util import (AERO_CLASSES, AERO_DELTA, AERO_GATE_RATE, AERO_PITCH_GATE, EULER_CLAMP, OPT_DRAG, OPT_GROUND, aero_fleet, aero_fused_starts,
                        aero_gate_margins, aero_power, aero_rotor_rel_heights, aero_sets, aero_substep_starts, f32)

DT = float(np.float32(1.0 / 240.0))
TYPES = ("robobee", "tello")
POWER, SHARE = 10.0, 0.90
SUBSTEPS = (1, 3)                                   # of the dsim_physics launches of the device tests


def _type(name):
    return params.builtin_type(name)


def _a6(a):
    out = np.zeros((len(a), 6)); out[:, :4] = a
    return out


@pytest.mark.parametrize("name", TYPES)
def test_cases_are_fp32_representable_and_in_range(name):
    t = _type(name)
    for cl, c in aero_sets(t).items():
        for key in ("rigid", "mem", "tgt", "act", "prev"):
            assert np.array_equal(c[key], f32(c[key])), (cl, key)
        assert np.allclose(np.linalg.norm(c["rigid"][:, 3:7], axis=1), 1.0, atol=1e-6)
    g = aero_sets(t)["gate"]
    assert g["rigid"][:, 2].min() >= 0.05 and g["rigid"][:, 2].max() <= f32(0.3)
    for key in ("act", "prev"):
        assert g[key].min() >= f32(0.3) and g[key].max() <= f32(0.9)           # no rotor at idle
    assert g["mem"][:, 7:11].min() >= f32(0.3)
    assert AERO_DELTA == 1e-3 and abs(math.sin(AERO_PITCH_GATE) - EULER_CLAMP) < 1e-15
    # every threshold from both sides, at the pitches and rolls asked for, at more than one yaw
    r, p, y = g["rpy"].T
    for s in (1, -1):
        for d in (-AERO_DELTA, AERO_DELTA):
            for pitch in (0.0, 0.7, -0.7):
                assert ((r == s * (math.pi / 2 + d)) & (p == pitch)).sum() == 2
            for roll in (0.0, 0.5, -0.5):
                assert ((p == s * (AERO_PITCH_GATE + d)) & (r == roll)).sum() == 2
    assert (r == math.pi).sum() == 2 and (r == -math.pi).sum() == 2 and ((r == 0) & (p == 0.1)).sum() == 2
    assert len(np.unique(y)) >= 26
    # a pair differs in the side only
    pr = g["partner"]
    assert (g["open"] != g["open"][pr]).all()
    for key in ("mem", "act", "prev", "tgt"):
        assert np.array_equal(g[key], g[key][pr])
    assert np.array_equal(g["rigid"][:, [0, 1, 2, 7, 8, 9]], g["rigid"][pr][:, [0, 1, 2, 7, 8, 9]])
    # ... and in which way it turns: away from the threshold, each at AERO_GATE_RATE (the plain members do not turn)
    plain = (np.abs(g["rpy"][:, 1]) == 0.1)
    w = np.linalg.norm(g["rigid"][:, 10:13], axis=1)
    assert plain.sum() == 6 and (w[plain] == 0).all() and np.allclose(w[~plain], AERO_GATE_RATE, rtol=1e-6)
    # (away: after one oracle sub-step without any force the angle in question has moved 0.02 rad to the case's own side)
    r1 = g["rigid"].copy()
    orc.Oracle([t]).physics(r1, g["mem"], 1, DT, action=np.zeros((len(r1), 6)))
    e0 = np.stack([orc.euler_from_quat(q) for q in g["rigid"][:, 3:7]])
    x, y_, z, w_ = r1[:, 3:7].T
    sarg1, rb1 = -2 * (x * z - w_ * y_), w_ * w_ - x * x - y_ * y_ + z * z
    rolls = ~plain & (np.abs(g["rpy"][:, 1]) < 1.0)
    pitches = ~plain & ~rolls
    assert rolls.sum() == 24 and pitches.sum() == 24
    assert ((rb1[rolls] > 0.01) == g["open"][rolls]).all() and (np.abs(rb1[rolls]) > 0.01).all()
    inside = pitches & g["open"]
    assert (np.abs(sarg1[inside]) < EULER_CLAMP - 5e-5).all() and (rb1[inside] > 0).all()
    outside = pitches & ~g["open"]            # over the top: the roll angle flips, the gate stays shut
    assert ((rb1[outside] < -1e-3) | (np.abs(sarg1[outside]) > EULER_CLAMP + 1e-6)).all()
    # (rounding the quaternion to fp32 moves the angles themselves: by up to 1e-5 rad beside the gimbal point, 1 % of delta)
    assert np.abs(e0[:, 0:2] - g["rpy"][:, 0:2])[g["open"]].max() < AERO_DELTA / 50


@pytest.mark.parametrize("name", TYPES)
def test_gate_cases_both_predicates_agree_with_margin(name):
    """(i) the oracle's predicate (Euler angles in fp64, gimbal branch included) == the kernel's (fp32, from the quaternion as
    load_aos stores it) == the side the case was built on; (ii) 16 fp32 ulps of the operands between every case and either
    threshold.  All three classes: the height and drag cases fly through the same gate."""
    for cl, c in aero_sets(_type(name)).items():
        open32, open64, clear, strict = aero_gate_margins(c["rigid"][:, 3:7])
        assert np.array_equal(open32, open64), (cl, np.flatnonzero(open32 != open64))
        assert strict.all(), (cl, np.flatnonzero(~strict))
        if cl == "gate":
            assert np.array_equal(open64, c["open"])
            assert 0.4 < c["open"].mean() < 0.6
        else:
            assert open64.all()


def _assert_clear(label, starts):
    for k, r in enumerate(starts):
        open32, open64, clear, _ = aero_gate_margins(f32(r[:, 3:7]))
        assert clear.all(), (label, "sub-step", k, np.flatnonzero(~clear))
        assert np.array_equal(open32, open64), (label, "sub-step", k)


@pytest.mark.parametrize("opts", [2, 3])             # (without DSIM_OPT_GROUND nobody evaluates the gate)
@pytest.mark.parametrize("names", [("robobee",), ("tello",), ("robobee", "tello")])
def test_no_drone_reaches_a_threshold_during_the_launches_of_the_device_tests(names, opts):
    """The gate is evaluated at the start of EVERY sub-step.  Along the oracle's own run of each launch the device tests make
    — dsim_physics at 1 and 3 sub-steps with the explicit and with the stored command, dsim_step at 1 and 2 sub-steps: one
    Env.step, another, then three more (in one launch, and one by one on the twin block) — no drone comes within the margin of a threshold with the gate's value at
    stake.  (The device tests ask the same of the device's own states in front of each launch.)"""
    types = [_type(m) for m in names]
    O = orc.Oracle(types)
    for n in (200, 333):
        f = aero_fleet(types, n)
        for sub in SUBSTEPS:
            for action in (_a6(f["act"]), None):
                starts, _ = aero_substep_starts(O, f["tid"], f["rigid"], f["mem"], sub, DT, action=action, options=opts,
                                                last_action=_a6(f["prev"]))
                _assert_clear((names, n, "physics", sub), starts)
        for sub in (1, 2):
            dtc = float(np.float32(sub / 240))
            r, m = f["rigid"], f["mem"]
            for n_steps in (1, 1, 3):
                starts, _, _, r, m = aero_fused_starts(O, f["tid"], r, m, f["tgt"], sub, DT, dtc, opts, n_steps)
                _assert_clear((names, n, "fused", sub, n_steps), starts)
                r, m = f32(r), f32(m)


@pytest.mark.parametrize("name", TYPES)
def test_height_cases_sit_where_they_claim(name):
    t = _type(name)
    c = aero_sets(t)["height"]
    clip32 = np.float32(t.gnd_eff_h_clip)
    z32 = c["rigid"][:, 2].astype(np.float32)
    g = c["group"]
    assert (z32[g == 0] == clip32).all() and (g == 0).sum() >= 2
    assert (z32[g == 1] == np.nextafter(clip32, np.float32(np.inf))).all() and (g == 1).sum() >= 2
    assert (z32[g == 2] == np.nextafter(clip32, np.float32(-np.inf))).all() and (g == 2).sum() >= 2
    assert (z32[g == 3] == np.float32(-0.2)).all() and (z32[g == 4] == np.float32(100.0)).all()
    rel = aero_rotor_rel_heights(t, c["rigid"][:, 3:7])
    level = g <= 4
    assert np.array_equal(rel[level], np.tile(np.asarray(t.rotor_pos)[:4, 2], (level.sum(), 1)))     # R's third row is (0, 0, 1)
    h = c["rigid"][:, 2:3] + rel
    tilted = g == 5
    tilt = np.arccos(np.clip([orc.matrix_from_quat(q)[2, 2] for q in c["rigid"][tilted, 3:7]], -1, 1))
    assert tilt.min() > 0.45 and tilt.max() < 1.25
    below, above = t.gnd_eff_h_clip - h[tilted].min(1), h[tilted].max(1) - t.gnd_eff_h_clip
    assert tilted.sum() >= 32 and (below > 1e-4).all() and (above > 1e-4).all(), (below.min(), above.min())
    assert (h[g == 3] < t.gnd_eff_h_clip).all() and (h[g == 4] > 99).all()


@pytest.mark.parametrize("name", TYPES)
def test_drag_cases_hold_every_speed_and_both_kinds_of_previous_action(name):
    c = aero_sets(_type(name))["drag"]
    v = np.linalg.norm(c["rigid"][:, 7:10], axis=1)
    rest = c["speed"] == 0
    assert rest.sum() >= 2 and (c["rigid"][rest, 7:10] == 0).all()
    for s in (0.5, 5.0, 30.0):
        assert (c["speed"] == s).sum() >= 4 and np.allclose(v[c["speed"] == s], s, rtol=1e-6)
    tilt = np.arccos([orc.matrix_from_quat(q)[2, 2] for q in c["rigid"][:, 3:7]])
    assert tilt.max() > 0.6
    assert (np.abs(c["act"] - c["prev"])[c["far"]].min(1) > 0.5).all()
    assert (~c["far"]).sum() >= 8 and np.array_equal(c["act"][~c["far"]], c["prev"][~c["far"]])
    for s in (0.0, 0.5, 5.0, 30.0):                     # every speed with a far and with an equal previous action
        assert (c["far"] & (c["speed"] == s)).any()
    assert (~c["far"] & (c["speed"] >= 5)).sum() >= 8
    assert (c["act_high"] & c["far"]).sum() >= 8 and (~c["act_high"] & c["far"]).sum() >= 12


def _share(label, ratio, among=None):
    sel = np.ones(len(ratio), dtype=bool) if among is None else among
    share = float((ratio[sel] > POWER).mean())
    msg = f"{label}: {share:.3f} of {int(sel.sum())} drones beyond {POWER:g} x the bar (median {np.median(ratio[sel]):.3g} x)"
    print(msg)
    assert share >= SHARE, msg
    return share


@pytest.mark.parametrize("sub", SUBSTEPS)
@pytest.mark.parametrize("name", TYPES)
def test_power_of_the_device_comparisons(name, sub):
    """For every class and every option set that acts on it: the oracle's step against the oracle's step WITHOUT the term, with
    the wrong previous action, or with the gate on the other side — in units of the bar the device test applies to that drone
    (tests/util.py:aero_power), beyond 10 on at least 90 % of the class.  The shares are printed (pytest -s) and stand in the
    assertion messages."""
    t = _type(name)
    O = orc.Oracle([t])
    sets = aero_sets(t)

    def run(c, options, last, rigid=None):
        r = (c["rigid"] if rigid is None else rigid).copy()
        O.physics(r, c["mem"], sub, DT, action=_a6(c["act"]), options=options, last_action=None if last is None else _a6(last))
        return r

    def power(c, options, ref, alt, rigid=None):
        return aero_power([t], None, c["rigid"] if rigid is None else rigid, c["mem"], c["tgt"], ref, alt, DT, sub, options,
                          c["act"], np.maximum(c["act"], c["prev"]))

    for opts in (1, 2, 3):
        # ---- a dropped term
        for cl, bit in (("gate", OPT_GROUND), ("height", OPT_GROUND), ("drag", OPT_DRAG)):
            if not opts & bit:
                continue
            c = sets[cl]
            ref, alt = run(c, opts, c["prev"]), run(c, opts & ~bit, c["prev"])
            ratio = power(c, opts, ref, alt)
            if cl == "gate":
                # a shut gate drops the term by right: there the fault is an OPEN gate, which adds what its partner across the
                # threshold gets (the same drone 2 delta away: the term differs by a few parts in a thousand)
                assert (ratio[~c["open"]] == 0).all()
                ratio = np.where(c["open"], ratio, ratio[c["partner"]])
            if cl == "drag":
                assert (ratio[c["speed"] == 0] == 0).all() or sub > 1          # at rest the term is exactly nothing
            _share(f"{name} sub={sub} opts={opts} {cl}: term dropped", ratio)
        # ---- the previous action
        if opts & OPT_DRAG:
            c = sets["drag"]
            ref, alt = run(c, opts, c["prev"]), run(c, opts, c["act"])
            ratio = power(c, opts, ref, alt)
            assert (ratio[~c["far"]] == 0).all()                               # the control group: prev == act, no difference
            # (the class of this check: the drones whose previous action differs — for the others the "fault" is none)
            _share(f"{name} sub={sub} opts={opts} drag: previous action := current", ratio, c["far"])
            # (... := 0, what an env that forgot its echo would hand over: told by the drones whose previous action was high)
            zero = run(c, opts, np.zeros_like(c["prev"]))
            _share(f"{name} sub={sub} opts={opts} drag: previous action := 0", power(c, opts, ref, zero),
                   c["far"] & ~c["act_high"] & (c["speed"] >= 5))


@pytest.mark.parametrize("name", TYPES)
def test_drag_at_rest_is_exactly_nothing_and_height_100_is_almost_nothing(name):
    t = _type(name)
    O = orc.Oracle([t])
    c = aero_sets(t)["drag"]
    rest = c["speed"] == 0
    a, b = c["rigid"].copy(), c["rigid"].copy()
    O.physics(a, c["mem"], 1, DT, action=_a6(c["act"]), options=OPT_DRAG, last_action=_a6(c["prev"]))
    O.physics(b, c["mem"], 1, DT, action=_a6(c["act"]))
    assert np.array_equal(a[rest], b[rest]) and not np.array_equal(a[~rest], b[~rest])
    h = aero_sets(t)["height"]
    far = h["group"] == 4
    a, b = h["rigid"].copy(), h["rigid"].copy()
    O.physics(a, h["mem"], 1, DT, action=_a6(h["act"]), options=OPT_GROUND)
    O.physics(b, h["mem"], 1, DT, action=_a6(h["act"]))
    assert 0 < np.abs(a[far] - b[far]).max() < 1e-6


def test_every_class_flies_in_every_fleet():
    """The fleets of the device tests (tests/util.py:aero_fleet) hold all three case sets, every group, side and speed of them,
    for every type, down to the smallest fleet; the interleaved one has at least three drones at rest."""
    for table, names in {"robobee": ("robobee",), "tello": ("tello",), "mixed": ("robobee", "tello")}.items():
        types = [params.builtin_type(m) for m in names]
        for n in (200, 333):
            f = aero_fleet(types, n)
            for k, t in enumerate(types):
                sel = np.ones(n, dtype=bool) if f["tid"] is None else f["tid"] == k
                s = aero_sets(t)
                for ci, cl in enumerate(AERO_CLASSES):
                    mine = sel & (f["cls"] == ci)
                    assert mine.sum() >= 15, (table, n, t.name, cl)
                    key = "open" if cl == "gate" else "group" if cl == "height" else "speed"
                    assert set(np.unique(s[cl][key][f["case"][mine]])) == set(np.unique(s[cl][key])), (table, n, t.name, cl)
            rest = (f["cls"] == AERO_CLASSES.index("drag")) & (np.linalg.norm(f["rigid"][:, 7:10], axis=1) == 0)
            assert rest.sum() >= 3, (table, n)
