"""CPU-side checks of the swept drone-drone contact watch (dsim_clearance_sweep): the ABI surface, the refusals that need no device,
the tests' own fp64 reference (tests/clearance_sweep_ref.py) against dense sampling and hand cases, the cell rule, the recorded
float32 error the GPU tolerance comes from, the input conditions of the GPU cases, and the env's keyword validation.
tests/README_clearance_sweep.md."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as graft
from dronesim_amd import params
from tests import clearance_sweep_ref as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nat():
    graft.build()
    from dronesim_amd import _native
    return _native


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_struct_layout(nat, tmp_path):
    hdr = open(os.path.join(ROOT, "include", "dronesim_amd.h")).read()
    lib = nat.load()
    assert re.search(r"^int\s+dsim_clearance_sweep\s*\(", hdr, flags=re.M)
    assert re.search(r"^int64_t\s+dsim_clearance_sweep_workspace\s*\(", hdr, flags=re.M)
    for f in ("dsim_clearance_sweep", "dsim_clearance_sweep_workspace"):
        assert f in nat.EXPORTS and getattr(lib, f) is not None
    assert lib.dsim_abi_version() == 11 and lib.dsim_abi_minor() == 1
    assert os.path.join(ROOT, "dronesim_amd", "csrc", "dsim_clearance_sweep.hip") in graft.HIP_DEPS and len(graft.HIP_SRCS) == 6
    fields = [f for f, _ in nat.ClearanceSweepArgs._fields_]
    lines = ['printf("size %zu\\n", sizeof(dsim_clearance_sweep_args));']
    lines += [f'printf("{f} %zu\\n", offsetof(dsim_clearance_sweep_args, {f}));' for f in fields]
    src = tmp_path / "clr_sweep.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dronesim_amd.h"\nint main(void) {\n' + "\n".join(lines)
                   + "\nreturn 0; }\n")
    exe = tmp_path / "clr_sweep"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(nat.ClearanceSweepArgs)
    for f in fields:
        assert int(got[f]) == getattr(nat.ClearanceSweepArgs, f).offset, f
    # the workspace: the clearance layout and one 16-byte aligned float4 [m] (its 4 words of slack counted), from one walk
    # (never below what the grid's own forms take: dsim_downwash_workspace)
    for m, nx, ny in ((1, 1, 1), (257, 9, 7), (1000, 30, 23), (4096, 2, 2), (65536, 300, 200)):
        cells = nx * ny
        walk = 2 * (cells + 1) + cells + (4 + 4 * m) + m + (4 + 4 * m)
        assert lib.dsim_clearance_sweep_workspace(m, nx, ny) == max(walk, lib.dsim_downwash_workspace(m, nx, ny))
    assert lib.dsim_clearance_sweep_workspace(4096, 2, 2) == lib.dsim_clearance_workspace(4096, 2, 2) + 4 + 4 * 4096
    assert lib.dsim_clearance_sweep_workspace(-1, 4, 4) == -1 and lib.dsim_clearance_sweep_workspace(4, 0, 4) == -1


def test_library_refuses_before_it_touches_a_device(nat):
    """The library looks at args, prev and the flags first, then at the grid's form, then at the context: with no context on this
    machine a call that is in order as far as that goes is DSIM_E_UNSUPPORTED for a halo plan (-5) — and DSIM_E_ARG (-1) as soon as
    args, prev or the flags are not, which shows that those are refused before anything else is looked at."""
    lib = nat.load()
    prev = np.zeros((3, 64), dtype=np.float32)
    out = np.zeros(64, dtype=np.float32)
    hp = nat.HaloPlan()
    g = nat.DownwashArgs()
    g.halo = ctypes.addressof(hp)
    world = nat.DownwashArgs()
    world.pos_all = prev.ctypes.data

    def call(grid=g, p=prev.ctypes.data, flags=0, null_args=False):
        a = nat.ClearanceSweepArgs(p, 0.5, 0.0, 0.2, flags, out.ctypes.data, None, None, None)
        return lib.dsim_clearance_sweep(None, None, 1, nat.View(), ctypes.byref(grid) if grid is not None else None,
                                        None if null_args else ctypes.byref(a))
    assert call() == -5 and call(grid=world) == -5 and call(flags=nat.SWEEP_KEEP_PREV) == -5 and call(flags=nat.SWEEP_PRIME) == -5
    assert call(null_args=True) == -1
    assert call(p=None) == -1
    assert call(flags=nat.SWEEP_KEEP_PREV | nat.SWEEP_PRIME) == -1
    assert call(flags=4) == -1 and call(flags=-1) == -1 and call(flags=nat.SWEEP_PRIME | 8) == -1
    # no context: refused, with or without a grid
    assert call(grid=nat.DownwashArgs()) == -1 and call(grid=None) == -1 and call(grid=None, flags=nat.SWEEP_PRIME) == -1
    assert not prev.any() and not out.any()


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def _random_pairs(rng, k, reach=1.0, length=0.8):
    p0i = rng.uniform(-1, 1, (k, 3))
    p0j = p0i + rng.uniform(-reach, reach, (k, 3))
    p1i = p0i + rng.uniform(0, length, (k, 1)) * cs.directions(rng, k)
    p1j = p0j + rng.uniform(0, length, (k, 1)) * cs.directions(rng, k)
    return p0i, p1i, p0j, p1j


def test_reference_against_dense_sampling():
    rng = np.random.default_rng(73)
    p0i, p1i, p0j, p1j = _random_pairs(rng, 2000)
    ref = cs.pair_dist(p0i, p1i, p0j, p1j)
    s = np.linspace(0.0, 1.0, 401)[None, :, None]
    d = (p0j - p0i)[:, None, :] * (1 - s) + (p1j - p1i)[:, None, :] * s
    sampled = np.sqrt((d * d).sum(-1)).min(1)
    delta = np.linalg.norm((p1j - p1i) - (p0j - p0i), axis=1)
    inside = ((ref < np.linalg.norm(p0j - p0i, axis=1) - 1e-9) & (ref < np.linalg.norm(p1j - p1i, axis=1) - 1e-9)).sum()
    print(f"reference vs 401 samples per pair: {int(inside)} of 2000 minima inside the step, worst sampled - reference "
          f"{(sampled - ref).max():.3e} m, worst reference - sampled {(ref - sampled).max():.3e} m")
    assert inside > 300
    assert np.all(ref <= sampled + 1e-12)                          # never above the sampled minimum
    assert np.all(sampled - ref <= delta / 400 + 1e-12)            # and within one sample spacing times |Delta| of it


def test_hand_cases():
    R = float(np.float32(params.builtin_type("robobee").collision_sphere))
    rad = np.full(2, np.float32(R))
    # a head-on swap: 0.05 m apart in y where they pass, 1 m apart at both ends
    ref = cs.sweep_pairs_brute(cs.f32(cs.SWAP_PREV), cs.f32(cs.SWAP_POS), rad, cs.SWAP_MARGIN, 0.0, cs.SWAP_TRAVEL)
    want = float(np.float32(0.025)) * 2 - 2 * R
    assert abs(ref[0][0] - want) < 1e-12 and abs(ref[0][1] - want) < 1e-12 and ref[1].tolist() == [1, 0] and ref[3] == 1 and ref[4] == 0
    ends = cs.sweep_pairs_brute(cs.f32(cs.SWAP_POS), cs.f32(cs.SWAP_POS), rad, cs.SWAP_MARGIN, 0.0, cs.SWAP_TRAVEL)
    assert ends[3] == 0 and ends[1].tolist() == [-1, -1] and ends[0].tolist() == [0.5, 0.5]
    # with a sag the pair is two sags closer
    sag = 0.01
    assert abs(cs.sweep_pairs_brute(cs.f32(cs.SWAP_PREV), cs.f32(cs.SWAP_POS), rad, cs.SWAP_MARGIN, sag, cs.SWAP_TRAVEL)[0][0]
               - (want - 2 * float(np.float32(sag)))) < 1e-12
    # a chord longer than travel is a point sample: both are, and nothing is seen
    short = cs.sweep_pairs_brute(cs.f32(cs.SWAP_PREV), cs.f32(cs.SWAP_POS), rad, cs.SWAP_MARGIN, 0.0, 0.9)
    assert short[3] == 0 and short[4] == 2 and short[1].tolist() == [-1, -1]
    # the same velocity on both: Delta = 0, the distance never changes, the point query's answer
    prev, pos, travel = (cs.f32(a) if i < 2 else a for i, a in enumerate(cs.small_cases()["same velocity"]))
    d = float(np.linalg.norm(pos[1].astype(np.float64) - pos[0].astype(np.float64)))
    ref = cs.sweep_pairs_brute(prev, pos, rad, cs.SWAP_MARGIN, 0.0, travel)
    assert abs(ref[0][0] - (d - 2 * R)) < 1e-7 and d - 2 * R < 0 and ref[3] == 1
    assert abs(cs.pair_dist(prev[0].astype(float), pos[0].astype(float), prev[1].astype(float), pos[1].astype(float)) - d) < 1e-7
    # one drone static: the distance between a point and the other's chord
    prev, pos, travel = (cs.f32(a) if i < 2 else a for i, a in enumerate(cs.small_cases()["one static"]))
    a, b, p = prev[1].astype(np.float64), pos[1].astype(np.float64), pos[0].astype(np.float64)
    t = np.clip(((p - a) @ (b - a)) / ((b - a) @ (b - a)), 0, 1)
    want = float(np.linalg.norm(a + t * (b - a) - p)) - 2 * R
    ref = cs.sweep_pairs_brute(prev, pos, rad, cs.SWAP_MARGIN, 0.0, travel)
    assert 0 < t < 1 and abs(ref[0][0] - want) < 1e-12 and ref[1].tolist() == [1, 0]
    # and where the minima of the other pairs of GPU case 1 lie
    for name, where in (("apart", 0), ("closing", 1), ("inside", 0.5)):
        prev, pos, _ = cs.small_cases()[name]
        d0, d1 = prev[1] - prev[0], pos[1] - pos[0]
        g = d1 - d0
        s = float(np.clip(-(d0 @ g) / (g @ g), 0, 1))
        assert (s == where) if where in (0, 1) else (0.2 < s < 0.8), (name, s)


def test_cell_rule():
    """Over random pairs with chords <= travel and c_ij < margin, the two current positions are less than one cell apart per axis at
    cell = 2 (R_max + sag) + margin + 2 travel; with + travel only, a counter-example exists."""
    rng = np.random.default_rng(79)
    R, sag, margin, travel = 0.158, 0.01, 0.5, 0.3
    cell = 2 * (R + sag) + margin + 2 * travel
    k = 200000
    p0i, p1i, p0j, p1j = _random_pairs(rng, k, reach=0.6, length=travel)
    # (half of the chords at full length, pointing away from the partner: the extreme the rule is made for)
    u = (p0j - p0i) / np.linalg.norm(p0j - p0i, axis=1, keepdims=True)
    far = rng.uniform(size=k) < 0.5
    p1i[far], p1j[far] = (p0i - travel * u)[far], (p0j + travel * u)[far]
    c = cs.pair_dist(p0i, p1i, p0j, p1j) - 2 * (R + sag)
    near = np.flatnonzero(c < margin)[:10000]
    assert near.size == 10000
    apart = np.abs(p1j - p1i)[near][:, :2].max(1)
    print(f"cell rule: worst axis distance of the current positions {apart.max():.4f} m over {near.size} pairs in reach, cell {cell:.4f} m, "
          f"cell with one travel {cell - travel:.4f} m")
    assert apart.max() < cell
    assert apart.max() > cell - travel


def test_restated_error_is_what_is_recorded():
    """The float32 restatement of the kernel's pair arithmetic against the fp64 reference on the GPU cases' own inputs, over the
    drones whose clearance the device reports (c < margin): its worst |c32 - c64| is the recorded RESTATED_WORST (not above it, and
    the record is not padded); the kernel is granted 4 x it, which stays below GUARD / 4."""
    worst = 0.0
    for name, prev, pos, rad, margin, sag, travel in cs.designed_inputs():
        raw = cs.sweep_pairs_brute(prev, pos, rad, margin, sag, travel)[5]
        c32 = cs.restated_pairs(prev, pos, rad, sag, travel)
        m = raw < float(np.float32(margin))
        assert m.any(), name
        assert np.all(c32[m] < float(np.float32(margin))) and np.array_equal(c32[m] < 0, raw[m] < 0), name   # (the guard band)
        err = float(np.abs(c32[m] - raw[m]).max())
        print(f"restated, {name}: worst |c32 - c64| = {err:.3e} m over {int(m.sum())} drones")
        worst = max(worst, err)
    print(f"restated worst {worst:.3e} m")
    assert worst <= cs.RESTATED_WORST <= 1.02 * worst, worst
    assert cs.ATOL == 4.0 * cs.RESTATED_WORST and cs.ATOL <= cs.GUARD / 4 and cs.GUARD == 1e-4


# ---- the GPU cases' inputs ----------------------------------------------------------------------------------------------------------
def _conditions(d, pairs_min, reach_min):
    clr, near, second, pairs, unswept, raw = d["ref"]
    assert d["redrawn"] <= 0.01, d["redrawn"]
    tie = (near >= 0) & (second - np.minimum(clr, second) < cs.ATOL)
    assert tie.mean() <= 0.01, tie.mean()
    assert pairs >= pairs_min and (near >= 0).sum() >= reach_min
    fin = np.isfinite(raw)
    assert not (np.abs(raw[fin]) < cs.GUARD).any() and not (np.abs(raw[fin] - d["margin"]) < cs.GUARD).any()
    length = np.linalg.norm(d["pos"].astype(np.float64) - d["prev"].astype(np.float64), axis=1)
    ok = np.isfinite(length)
    assert not (np.abs(length[ok] - d["travel"]) <= cs.TRAVEL_BAND * d["travel"]).any()
    assert np.abs(d["pos"][np.isfinite(d["pos"]).all(1)][:, :2]).max() <= 128.0
    return length


def test_conditions_of_the_crowded_case():
    d = cs.case_crowded()
    length = _conditions(d, 500, 400)
    assert d["ref"][4] == 0 and length.max() <= d["travel"]
    R = float(np.float32(d["type"].collision_sphere))
    i = np.arange(cs.PLANT_FIRST, cs.PLANT_FIRST + 2 * cs.PLANT_PAIRS)
    a, b = i[0::2], i[1::2]
    clr, near, _, _, _, raw = d["ref"]
    # planted pairs: each the other's nearest, overlapping along the step by the gap they start with, apart at its end
    assert np.array_equal(near[a], b) and np.array_equal(near[b], a)
    assert np.all(np.abs(raw[a] - (cs.PLANT_GAP - 2 * R)) < 1e-5) and np.all(raw[a] < -cs.GUARD)
    end = np.linalg.norm(d["pos"][a].astype(np.float64) - d["pos"][b].astype(np.float64), axis=1)
    assert np.all(end - 2 * R > d["margin"] + cs.GUARD)          # (the point query does not even have them in reach)
    assert np.all(np.abs(length[i] - 0.95 * d["travel"]) < 1e-6)
    # their ends: two cells apart along the flight's axis in the point watch's grid, adjacent (and not the same) in the sweep's
    axis = np.repeat([0, 1, 0], 3)
    for grid, want in ((d["point_grid"], 2), (d["sweep_grid"], 1)):
        ca, cb = cs.cell_of(grid, d["pos"][a, :2].astype(np.float64)), cs.cell_of(grid, d["pos"][b, :2].astype(np.float64))
        diff = np.stack([cb[0] - ca[0], cb[1] - ca[1]], 1)
        assert np.array_equal(diff[np.arange(cs.PLANT_PAIRS), axis], np.full(cs.PLANT_PAIRS, want)), (grid[0], diff)
        assert np.abs(diff).max() <= want
    from dronesim_amd.downwash import clearance_grid
    assert d["sweep_grid"] == clearance_grid((-20.0, -15.0), (20.0, 15.0), d["type"].collision_sphere, d["margin"] + 2 * d["travel"], 1000)
    assert d["sweep_grid"][0] >= 2 * R + d["margin"] + 2 * d["travel"] > d["point_grid"][0]


def test_conditions_of_the_mixed_case():
    d = cs.case_mixed()
    _conditions(d, 10, 300)
    assert [t.collision_sphere > 0 for t in d["types"]] == [True, True, False] and (d["rad"] == 0).sum() == cs.MIXED_N // 3
    clr, near = d["ref"][0], d["ref"][1]
    ghost = d["rad"] == 0
    assert np.all(clr[ghost] == np.float32(d["margin"])) and np.all(near[ghost] == -1) and not np.isin(near[near >= 0], np.flatnonzero(ghost)).any()


def test_conditions_of_the_unswept_case():
    d = cs.case_unswept()
    _conditions(d, 5, 100)
    length = np.linalg.norm(d["pos"].astype(np.float64) - d["prev"].astype(np.float64), axis=1)
    assert np.all(length[:40] > 1.5 * d["travel"] - 1e-6) and np.all(length[:40] < 3 * d["travel"] + 1e-6)
    assert not np.isfinite(d["prev"][40:45]).all(1).any() and np.isnan(d["pos"][45, 1]) and np.isfinite(np.delete(d["pos"], 45, 0)).all()
    assert np.isfinite(length[46:]).all() and length[46:].max() < d["travel"]
    # 46 drones are point samples; those without a sphere (every third) are not counted
    assert d["ref"][4] == int((d["rad"][:46] > 0).sum()) == 30
    # the lost drone sees nobody and nobody sees it
    assert d["ref"][1][45] == -1 and not (d["ref"][1] == 45).any()


def test_the_dropped_column_on_paper():
    """GPU case 6's drop speed, chosen on the reference: with the row standing and the column falling at anything between no
    acceleration and g, the swept query counts every passing pair and more pair-steps than the samples do."""
    t = params.builtin_type("tello")
    from dronesim_amd.obstacles import sweep_sag
    for accel in (0.0, 5.0, 9.8):
        swept, point = cs.drop_model(t.collision_sphere, sweep_sag(9.8, cs.DROP_DT), accel)
        print(f"dropped column on paper, a = {accel}: swept {swept}, samples {point}")
        assert swept >= cs.DROP_N and swept >= point + 10
    # the chords of the flight: within DROP_TRAVEL per Env.step, beyond the default 10 m/s x one Env.step at four steps per launch
    v_end = cs.DROP_SPEED + 9.8 * cs.DROP_STEPS * cs.DROP_DT
    assert v_end * cs.DROP_DT < cs.DROP_TRAVEL and 4 * cs.DROP_SPEED * cs.DROP_DT > 10.0 * cs.DROP_DT


# ---- the env's keywords -----------------------------------------------------------------------------------------------------------
def test_env_keyword_validation():
    """All before a context is made."""
    from dronesim_amd.envs import CtrlAviary
    kw = dict(initial_xyzs=np.zeros((4, 3)), dict_io=False, noise_seed=0)
    for bad in (dict(drone_sweep=True), dict(drone_sweep_sag=0.01), dict(drone_sweep_travel=0.5)):
        with pytest.raises(ValueError, match="without drone_watch=True"):
            CtrlAviary(["tello"], 4, **bad, **kw)
    for bad in (dict(drone_sweep_sag=0.01), dict(drone_sweep_travel=0.5)):
        with pytest.raises(ValueError, match="without drone_sweep=True"):
            CtrlAviary(["tello"], 4, drone_watch=True, **bad, **kw)
    for sag in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="drone_sweep_sag must be >= 0"):
            CtrlAviary(["tello"], 4, drone_watch=True, drone_sweep=True, drone_sweep_sag=sag, **kw)
    for travel in (0.0, 5e-4, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="at least a millimetre"):
            CtrlAviary(["tello"], 4, drone_watch=True, drone_sweep=True, drone_sweep_travel=travel, **kw)


def test_drone_unswept_needs_the_sweep():
    from dronesim_amd.envs import CtrlAviary
    e = CtrlAviary.__new__(CtrlAviary)                            # (an env made without the sweep: the class's "nothing on")
    e._drone_watch = True
    with pytest.raises(ValueError, match="drone_sweep=True"):
        e.drone_unswept()
    e._drone_sweep, e._drone_unswept = True, None
    assert e.drone_unswept() == 0


def test_sharded_forms_are_refused():
    import types as pytypes
    from dronesim_amd.downwash import Downwash

    class TwoRanks:
        is_initialized = staticmethod(lambda: True)
        get_world_size = staticmethod(lambda: 2)
    dw = Downwash.__new__(Downwash)
    dw.halo, dw.dist = None, TwoRanks()
    with pytest.raises(NotImplementedError):
        dw.clearance_sweep(0.5, 0.0, 0.2, None)
    with pytest.raises(NotImplementedError):
        dw.clearance_prime(None)
    dw.halo, dw.dist = pytypes.SimpleNamespace(), None
    with pytest.raises(NotImplementedError):
        dw.clearance_sweep(0.5, 0.0, 0.2, None)
