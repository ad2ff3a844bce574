"""CPU tests of moving obstacle scenes: SceneMotion's closed forms and validation, the env's refusals (checked before any device
work) and the ABI of the new struct and symbols (tests/README_motion.md).  The GPU tests compare the device's table with
SceneMotion.place, so what is checked here is that reference itself."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from dronesim_amd import _native as nat
from dronesim_amd.obstacles import ObstacleScenes, SceneMotion
from tests import motion_ref as mr
from tests import scenes_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one(rpy=(0.3, -0.2, 1.1), pos=(1.0, -2.0, 1.5)):
    """K = 1, G = 1: one placement of the gate."""
    return ObstacleScenes(sr.gate(), np.array(pos, dtype=np.float64).reshape(1, 1, 3), np.array(rpy, dtype=np.float64).reshape(1, 1, 3))


def base(scenes):
    p = scenes.place.astype(np.float64)
    return p[..., :9].reshape(p.shape[:2] + (3, 3)), p[..., 9:]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- closed forms ----------------------------------------------------------------------------------------------------------------------
def test_velocity_alone_is_a_straight_line():
    s = one()
    R0, t0 = base(s)
    R, t = SceneMotion(s, velocity=(1, 0, 0)).pose(2.0)
    assert np.array_equal(t, t0 + np.array([2.0, 0, 0])) and np.array_equal(R, R0)


def test_rate_about_z_for_a_quarter_turn():
    s = one()
    R0, t0 = base(s)
    rate = np.float32(np.pi / 2)
    R, t = SceneMotion(s, axis=(0, 0, 1), rate=rate).pose(1.0)
    th = float(rate)                                             # (the float32 the library is given, not pi / 2 itself)
    Rz = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
    np.testing.assert_allclose(R[0, 0], Rz @ R0[0, 0], rtol=0, atol=1e-15)
    quarter = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    np.testing.assert_allclose(R[0, 0], quarter @ R0[0, 0], rtol=0, atol=1e-7)       # pi / 2 to float32
    assert np.array_equal(t, t0)


def test_oscillation_at_a_quarter_period_stands_at_the_amplitude():
    s = one()
    R0, t0 = base(s)
    amp = np.array([0.25, -0.5, 0.125], dtype=np.float32)
    # omega tau + phase = pi / 2 with omega = 2, phase = 0.5 (both exact in float32)
    tau = (np.pi / 2 - 0.5) / 2.0
    R, t = SceneMotion(s, amplitude=amp, omega=2.0, phase=0.5).pose(tau)
    np.testing.assert_allclose(t[0, 0], t0[0, 0] + amp, rtol=0, atol=1e-15)
    assert np.array_equal(R, R0)


def test_swing_alone_at_a_half_period_is_back_at_the_base():
    s = one()
    R0, _ = base(s)
    m = SceneMotion(s, axis=(0, 1, 0), omega=4.0, swing=0.7)
    R, _ = m.pose(np.pi / 4.0)                                  # omega tau = pi: s = sin(pi) = 1.2e-16, theta = 0.7 s
    np.testing.assert_allclose(R, R0, rtol=0, atol=1e-15)
    Rq, _ = m.pose(np.pi / 8.0)                                 # ... and at a quarter period theta = swing
    th = float(np.float32(0.7))
    Ry = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    np.testing.assert_allclose(Rq[0, 0], Ry @ R0[0, 0], rtol=0, atol=1e-15)


@pytest.mark.parametrize("tau", [0.0, 7 * mr.DT, 123.456, 2 ** 33 * mr.DT])
def test_rotation_stays_a_rotation(tau):
    """R^T R = I and det R = 1 to 1e-14 with an EXACT base rotation and an axis normalised in fp64: the float32 base matrix is
    orthonormal to 6e-8 only, and Rodrigues' formula keeps what it is given."""
    from dronesim_amd.obstacles import _rot
    s = mr.small_world()
    for m in mr.small_motions(vel_zero=tau > 1e6):
        k = m.axis.astype(np.float64)
        n = np.linalg.norm(k, axis=-1, keepdims=True)
        k = np.where(n > 0, k / np.where(n > 0, n, 1.0), 0.0)
        sn = np.sin(m.omega.astype(np.float64) * tau + m.phase.astype(np.float64))
        th = m.rate.astype(np.float64) * tau + m.swing.astype(np.float64) * sn
        Rm, _ = m.pose(tau)
        for (a, g) in zip(*np.nonzero(m.used)):
            R0 = _rot(s.rpy[a, g])
            v, c, sg = R0, np.cos(th[a, g]), np.sin(th[a, g])
            kk = k[a, g][:, None]
            R = v * c + np.cross(np.broadcast_to(kk, (3, 3)), v, axis=0) * sg + kk * ((kk * v).sum(0, keepdims=True) * (1 - c))
            assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(R) - 1.0) <= 1e-14
            # ... and pose(), on the float32 base matrix and axis, is that rotation to their rounding (a few 6e-8)
            assert np.abs(Rm[a, g] - R).max() <= 1e-6


def test_place_at_zero_is_the_base_table_bit_for_bit():
    """With phase = 0: sin(0) = 0 exactly, so t(0) = t0 and theta(0) = 0.  (A non-zero phase starts the oscillation away from
    the base pose: t(0) = t0 + amp sin(phase), by the law.)"""
    s = mr.small_world()
    rng = np.random.default_rng(5)
    ax = rng.normal(size=(3, 3, 3))
    ax /= np.linalg.norm(ax, axis=-1, keepdims=True)
    m = SceneMotion(s, velocity=rng.uniform(-1, 1, (3, 3, 3)), amplitude=rng.uniform(-1, 1, (3, 3, 3)), omega=rng.uniform(1, 5, (3, 3)),
                    axis=ax, rate=rng.uniform(-3, 3, (3, 3)), swing=0.5)
    assert m.moving.sum() == 4
    got = m.place(0.0)
    assert got.dtype == np.float32 and got.shape == (3, 3, 12)
    assert np.array_equal(bits(got), bits(s.place))


def test_static_slots_are_the_base_table_at_every_time_and_unused_slots_nan():
    s = mr.small_world()
    for m in mr.small_motions():
        assert (m.kinds[m.used & ~m.moving] == "static").all() and (m.kinds[m.moving] != "static").all()
        got = m.place(123.456)
        static = m.used & ~m.moving
        assert static.sum() == 1 and np.array_equal(bits(got[static]), bits(s.place[static]))
        assert np.isnan(got[~m.used]).all() and np.isfinite(got[m.used]).all()
        assert not np.array_equal(bits(got[m.moving]), bits(s.place[m.moving]))
        R, t = m.pose(123.456)
        assert R.dtype == np.float64 and R.shape == (3, 3, 3, 3) and t.shape == (3, 3, 3) and np.isnan(R[~m.used]).all()
        snap = m.snapshot(123.456)
        assert isinstance(snap, ObstacleScenes) and np.array_equal(bits(snap.place), bits(got)) and snap.prototype is s.prototype
        assert np.array_equal(snap.count, s.count) and snap.K == 3 and snap.G == 3


def test_the_worlds_of_the_gpu_tests_hold_every_kind():
    kinds = set()
    for m in mr.small_motions():
        kinds |= set(m.kinds[m.used])
    assert kinds == set(mr.KINDS)
    big = mr.big_motion()
    assert set(big.kinds[big.used]) == set(mr.KINDS) and big.used.sum() == 701 and big.scenes.K * big.scenes.G == 1400
    zero = mr.big_motion(vel_zero=True)
    assert not zero.velocity[zero.used].any() and zero.moving.sum() < big.moving.sum()


# ---- validation and broadcasting ---------------------------------------------------------------------------------------------------------
def test_broadcasting():
    s = mr.small_world()
    m = SceneMotion(s, velocity=(1, 2, 3), omega=np.array([1.0, 2.0, 3.0])[:, None], axis=(0, 0, 1), rate=np.arange(3.0))
    assert m.velocity.shape == (3, 3, 3) and m.velocity.dtype == np.float32 and (m.velocity == [1, 2, 3]).all()
    assert m.omega.shape == (3, 3) and (m.omega[:, 0] == [1, 2, 3]).all() and (m.rate[0] == [0, 1, 2]).all()
    rec = m.records()
    assert rec.shape == (3, 3, 16) and rec.dtype == np.float32 and rec.flags.c_contiguous and not rec[..., 13:].any()
    assert (rec[..., 8:11] == [0, 0, 1]).all() and (rec[..., 6] == m.omega).all() and (rec[..., 11] == m.rate).all()


def test_validation_errors():
    s = mr.small_world()
    with pytest.raises(TypeError):
        SceneMotion(sr.gate())
    with pytest.raises(ValueError, match="broadcast"):
        SceneMotion(s, velocity=np.zeros((2, 3)))
    with pytest.raises(ValueError, match="broadcast"):
        SceneMotion(s, omega=np.zeros((4, 3)))
    for key in ("velocity", "amplitude", "omega", "phase", "rate", "swing"):
        for bad in (np.nan, np.inf):
            with pytest.raises(ValueError, match="non-finite"):
                SceneMotion(s, axis=(1, 0, 0), **{key: bad})
    with pytest.raises(ValueError, match="non-finite"):
        SceneMotion(s, axis=(np.nan, 0, 0))
    with pytest.raises(ValueError, match="unit"):
        SceneMotion(s, axis=(1, 1, 0), rate=1.0)
    with pytest.raises(ValueError, match="unit"):
        SceneMotion(s, axis=(1.0 + 1e-4, 0, 0))
    with pytest.raises(ValueError, match="unit"):
        SceneMotion(s, rate=1.0)                                 # a zero axis turns nothing
    with pytest.raises(ValueError, match="unit"):
        SceneMotion(s, swing=0.5)
    SceneMotion(s, axis=(1.0 + 5e-6, 0, 0), rate=1.0)            # unit to 1e-5
    # an unused slot is not looked at
    bad = np.zeros((3, 3))
    bad[2, :] = np.nan
    bad[1, 1:] = np.inf
    assert not SceneMotion(s, omega=bad).moving.any()
    bad[1, 0] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        SceneMotion(s, omega=bad)


# ---- the env's refusals, before any device work ---------------------------------------------------------------------------------------
def test_env_refusals_without_a_device():
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.obstacles import Aperture
    s, other = mr.small_world(), one()
    m = SceneMotion(s, velocity=(1, 0, 0))
    ids = np.arange(4) % 3
    xyz = np.zeros((4, 3)) + [0, 0, 1.0]
    kw = dict(initial_xyzs=xyz, obstacle_scene_id=ids)
    ap = Aperture((0, 0, 0), (1, 0, 0), (0, 1, 0), (0.3, 0.2))
    with pytest.raises(ValueError, match="SceneMotion"):
        CtrlAviary(["tello"], 4, obstacle_watch=s, obstacle_motion=s, **kw)
    with pytest.raises(ValueError, match="made for"):                              # a motion made for another scenes object
        CtrlAviary(["tello"], 4, obstacle_watch=s, obstacle_motion=SceneMotion(other), **kw)
    twin = ObstacleScenes(s.prototype, s.position, s.rpy, s.count)                  # (equal, but not the object)
    with pytest.raises(ValueError, match="made for"):
        CtrlAviary(["tello"], 4, obstacle_watch=twin, obstacle_motion=m, **kw)
    with pytest.raises(ValueError, match="made for"):                              # a motion without obstacle_watch
        CtrlAviary(["tello"], 4, obstacle_motion=m, initial_xyzs=xyz)
    with pytest.raises(ValueError, match="made for"):                              # ... or with a plain set
        CtrlAviary(["tello"], 4, obstacle_watch=sr.gate(), obstacle_motion=m, initial_xyzs=xyz)
    for gs in (None, s):                                                            # a gate watch that would read the moved table
        with pytest.raises(NotImplementedError, match="k_gate_passage"):
            CtrlAviary(["tello"], 4, obstacle_watch=s, obstacle_motion=m, gate_watch=ap, gate_scenes=gs, **kw)
    with pytest.raises(NotImplementedError, match="swept watch on scenes"):        # refused as it is without a motion
        CtrlAviary(["tello"], 4, obstacle_watch=s, obstacle_motion=m, obstacle_sweep=True, **kw)
    with pytest.raises(NotImplementedError, match="swept watch on scenes"):
        CtrlAviary(["tello"], 4, obstacle_watch=s, obstacle_sweep=True, **kw)


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------
def test_header_declares_what_the_binding_exports_and_the_abi_stands():
    hdr = open(os.path.join(ROOT, "include", "dronesim_amd.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(dsim_\w+)\s*\(", hdr, flags=re.M))
    new = {"dsim_scenes_motion_set", "dsim_scenes_move", "dsim_scenes_read"}
    assert new <= declared and declared == set(nat.EXPORTS), declared ^ set(nat.EXPORTS)
    lib = nat.load()
    for sym in new:
        assert getattr(lib, sym) is not None
    assert (nat.ABI_VERSION, nat.ABI_MINOR) == (11, 1) and (lib.dsim_abi_version(), lib.dsim_abi_minor()) == (11, 1)
    assert re.search(r"#define DSIM_ABI_VERSION 11\b", hdr) and re.search(r"#define DSIM_ABI_MINOR 1\b", hdr)
    note = hdr[hdr.index("#define DSIM_ABI_MINOR"):hdr.index("#define DSIM_MAX_ACT")]
    for name in sorted(new) + ["dsim_scene_motion"]:
        assert name in note, name


def test_scene_motion_struct_matches_c(tmp_path):
    """dsim_scene_motion: 64 bytes, and the ctypes mirror has the C compiler's size and field offsets (the protocol of
    tests/test_abi_cpu.py::test_struct_sizes_match_c)."""
    cls, cname = nat.SceneMotionC, "dsim_scene_motion"
    lines = [f'printf("{cname} %zu\\n", sizeof({cname}));']
    for fname, _ in cls._fields_:
        lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dronesim_amd.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got[cname]) == ctypes.sizeof(cls) == 64
    for fname, _ in cls._fields_:
        assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, fname
    want = {"vel": 0, "amp": 12, "omega": 24, "phase": 28, "axis": 32, "rate": 44, "swing": 48, "pad_": 52}
    assert {f: getattr(cls, f).offset for f, _ in cls._fields_} == want
    # ... and SceneMotion.records() lays a slot out as that struct
    m = SceneMotion(one(), velocity=(1, 2, 3), amplitude=(4, 5, 6), omega=7.0, phase=8.0, axis=(0, 0, 1), rate=9.0, swing=10.0)
    c = cls.from_buffer_copy(m.records().tobytes())
    assert (list(c.vel), list(c.amp), c.omega, c.phase, list(c.axis), c.rate, c.swing) == ([1, 2, 3], [4, 5, 6], 7, 8, [0, 0, 1], 9, 10)
