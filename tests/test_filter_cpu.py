"""CPU-side checks of the velocity safety filter (dsim_velocity_filter, avoid.VelocityFilter, CtrlAviary(velocity_filter=...)): the
ABI names and the struct mirror, the library's and the Python calls' device-free refusals, the env's keyword checks, the fp64
reference of tests/filter_ref.py on cases with known answers, reciprocity on the reference, and — on the reference alone — the caps
of the two masks and the float32 figure of every random GPU case (tests/README_filter.md)."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

import __graft_entry__ as graft
from tests import filter_ref as fr
from tests import scenes_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nat():
    graft.build()
    from dronesim_amd import _native
    return _native


# ---- ABI -----------------------------------------------------------------------------------------------------------------------------
FIELDS = ["u", "offset", "type_id", "alpha", "share", "buffer_drone", "buffer_obstacle", "floor", "has_floor", "k", "m", "nb_index",
          "nb_dist", "nb_rel_pos", "nb_rel_vel", "wit_clearance", "wit_body", "wit_rel", "wit_vel", "v_out", "dropped_out", "counters"]


def test_header_declares_library_exports_and_mirror_matches(nat, tmp_path):
    hdr = open(os.path.join(ROOT, "include", "dronesim_amd.h")).read()
    lib = nat.load()
    minor = hdr[hdr.index("#define DSIM_ABI_MINOR"):hdr.index("#define DSIM_MAX_ACT")]
    m = re.search(r"^int\s+dsim_velocity_filter\s*\(([^;]*)\);", hdr, flags=re.M | re.S)
    assert m and m.group(1).count(",") + 1 == 5 == len(lib.dsim_velocity_filter.argtypes)
    assert "dsim_velocity_filter" in nat.EXPORTS and "dsim_velocity_filter" in minor and "dsim_filter_args" in minor
    # functions only: the ABI number stands
    assert re.search(r"#define DSIM_ABI_VERSION 11\b", hdr) and re.search(r"#define DSIM_ABI_MINOR 1\b", hdr)
    assert lib.dsim_abi_version() == 11 and lib.dsim_abi_minor() == 1 and (nat.ABI_VERSION, nat.ABI_MINOR) == (11, 1)
    assert os.path.join(ROOT, "dronesim_amd", "csrc", "dsim_avoid.hip") in graft.HIP_DEPS and len(graft.HIP_SRCS) == 6
    assert '#include "dsim_avoid.hip"' in open(os.path.join(ROOT, "dronesim_amd", "csrc", "dsim_downwash.hip")).read()
    assert [f for f, _ in nat.FilterArgs._fields_] == FIELDS
    lines = ['printf("size %zu\\n", sizeof(dsim_filter_args));',
             'printf("bits %d %d %d %d\\n", (int)DSIM_FILTER_FLOOR_BIT, (int)DSIM_FILTER_OBSTACLE_BIT, (int)DSIM_FILTER_NEIGHBOR_BIT, '
             '(int)DSIM_FILTER_ROWS);']
    lines += [f'printf("{f} %zu\\n", offsetof(dsim_filter_args, {f}));' for f in FIELDS]
    src = tmp_path / "filter.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dronesim_amd.h"\nint main(void) {\n' + "\n".join(lines)
                   + "\nreturn 0; }\n")
    exe = tmp_path / "filter"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(ln.split(None, 1) for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(nat.FilterArgs) == 144
    assert got["bits"].split() == ["0", "1", "9", "25"]
    assert (nat.FILTER_FLOOR_BIT, nat.FILTER_OBSTACLE_BIT, nat.FILTER_NEIGHBOR_BIT, nat.FILTER_ROWS) == (0, 1, 9, 25)
    assert (fr.FLOOR_BIT, fr.OBST_BIT, fr.NB_BIT, fr.ROWS) == (0, 1, 9, 25)
    for f in FIELDS:
        assert int(got[f]) == getattr(nat.FilterArgs, f).offset, f


def _args(nat, **kw):
    a = nat.FilterArgs()
    one = ctypes.c_void_p(16).value          # (never dereferenced: every refusal comes before the device is touched)
    base = dict(u=one, v_out=one, dropped_out=one, alpha=2.0, share=0.5, buffer_drone=0.0, buffer_obstacle=0.0, k=2, m=0,
                nb_index=one, nb_dist=one, nb_rel_pos=one, nb_rel_vel=one)
    base.update(kw)
    for f, v in base.items():
        setattr(a, f, v)
    return a


def test_library_refuses_before_it_touches_a_device(nat):
    lib = nat.load()
    v = nat.View()
    v.n_pad = 256
    ctx = ctypes.c_void_p(0)
    assert lib.dsim_velocity_filter(None, None, 1, v, None) == -1
    assert lib.dsim_velocity_filter(None, None, 1, v, ctypes.byref(_args(nat))) == -1            # a null ctx
    # a ctx that is never dereferenced before the checks below fail: the refusals are about the arguments alone
    fake = ctypes.create_string_buffer(1 << 16)
    ctx = ctypes.cast(fake, ctypes.c_void_p)
    bad = [dict(u=None), dict(v_out=None), dict(dropped_out=None), dict(k=17), dict(k=-1), dict(m=9), dict(m=-1), dict(k=0, m=0),
           dict(alpha=0.0), dict(alpha=-1.0), dict(alpha=float("inf")), dict(alpha=float("nan")), dict(share=0.0), dict(share=1.5),
           dict(share=float("nan")), dict(buffer_drone=-0.1), dict(buffer_obstacle=float("inf")), dict(buffer_obstacle=-1.0),
           dict(nb_dist=None), dict(nb_rel_vel=None), dict(m=2), dict(has_floor=1, floor=float("nan"))]
    for kw in bad:
        assert lib.dsim_velocity_filter(ctx, None, 1, v, ctypes.byref(_args(nat, **kw))) == -1, kw
    assert lib.dsim_velocity_filter(ctx, None, 0, v, ctypes.byref(_args(nat))) == -1
    assert lib.dsim_velocity_filter(ctx, None, 257, v, ctypes.byref(_args(nat))) == -1


# ---- the Python class, device-free ---------------------------------------------------------------------------------------------------
def _stand_in(n=5, n_pad=8, n_types=1):
    ctx = types.SimpleNamespace(types=[object()] * n_types, device="cpu", lib=None, handle=0, stream_ptr=lambda: 0)
    state = types.SimpleNamespace(n=n, n_pad=n_pad, view=lambda: None)
    return ctx, state


def test_python_refusals_come_before_any_device_call():
    import torch
    from dronesim_amd import avoid
    from dronesim_amd.downwash import Neighbors
    from dronesim_amd.obstacles import ObstacleWitnesses
    ctx, state = _stand_in()
    for kw, what in ((dict(alpha=0.0), "alpha"), (dict(alpha=float("nan")), "alpha"), (dict(alpha="2"), "alpha"),
                     (dict(alpha=1.0, share=0.0), "share"), (dict(alpha=1.0, share=1.01), "share"),
                     (dict(alpha=1.0, buffer_drone=-1e-3), "buffer_drone"), (dict(alpha=1.0, buffer_obstacle=float("inf")), "buffer_obstacle"),
                     (dict(alpha=1.0, floor=float("nan")), "floor")):
        with pytest.raises(ValueError, match=what):
            avoid.VelocityFilter(ctx, state, **kw)
    with pytest.raises(ValueError, match="type_id"):
        avoid.VelocityFilter(_stand_in(n_types=2)[0], state, 1.0)
    f = avoid.VelocityFilter(ctx, state, 2.0)                      # (ctx.lib is None: any call into the library would raise)
    assert (f.alpha, f.share, f.buffer_drone, f.buffer_obstacle, f.floor) == (2.0, 0.5, 0.0, 0.0, None) and f.counters() == (0, 0)
    u = torch.zeros((3, 8))
    k, m = 2, 3
    nb = Neighbors(torch.zeros((k, 8), dtype=torch.int32), torch.zeros((k, 8)), torch.zeros((k, 3, 8)), torch.zeros((k, 3, 8)), None)
    w = ObstacleWitnesses(torch.zeros((m, 8)), torch.zeros((m, 8), dtype=torch.int32), torch.zeros((m, 3, 8)), None, None)
    with pytest.raises(ValueError, match="nothing to filter against"):
        f.apply(u)
    with pytest.raises(ValueError, match="u must be"):
        f.apply(torch.zeros((3, 7)), nb)
    with pytest.raises(ValueError, match="u must be"):
        f.apply(u.double(), nb)
    with pytest.raises(ValueError, match="rel_vel"):
        f.apply(u, nb._replace(rel_vel=None))
    with pytest.raises(ValueError, match="neighbors.dist"):
        f.apply(u, nb._replace(dist=torch.zeros((k, 9))))
    with pytest.raises(ValueError, match="1 .. 16"):
        f.apply(u, Neighbors(torch.zeros((17, 8), dtype=torch.int32), torch.zeros((17, 8)), torch.zeros((17, 3, 8)),
                             torch.zeros((17, 3, 8)), None))
    with pytest.raises(ValueError, match="witnesses.body"):
        f.apply(u, None, w._replace(body=torch.zeros((m, 8))))
    with pytest.raises(ValueError, match="witnesses.rel"):
        f.apply(u, None, w._replace(rel=torch.zeros((m, 8, 3)).transpose(1, 2)))
    with pytest.raises(ValueError, match="out"):
        f.apply(u, nb, w, out=avoid.Filtered(torch.zeros((3, 5)), torch.zeros((8,), dtype=torch.int32)))
    assert avoid.Filtered._fields == ("vel", "dropped") and (avoid.FLOOR_BIT, avoid.OBSTACLE_BIT, avoid.NEIGHBOR_BIT) == (0, 1, 9)


# ---- the env's keyword -----------------------------------------------------------------------------------------------------------------
def _options(**kw):
    from dronesim_amd.envs.watches import StepWatches
    base = dict(num_drones=4, freq=240, aggregate_phy_steps=1, dist=None, drone_watch=False, drone_watch_margin=1.0,
                obstacle_watch=None, obstacle_margin=1.0, obstacle_sweep=False, obstacle_sweep_sag=0.0, obstacle_sweep_travel=None,
                vision_attributes=False, vision_scene=None, vision_drones=None, vision_res=(64, 48), vision_ground=True,
                vision_see_drones=False, vision_drone_range=None)
    base.update(kw)
    w = StepWatches()
    w._watch_options(**base)
    return w


def test_keyword_is_off_by_default_and_checked():
    from dronesim_amd.envs.watches import StepWatches
    w = StepWatches()
    assert StepWatches._filter is None and StepWatches._filter_opts is None and w.last_filter_dropped is None
    assert _options()._filter_opts is None and _options(neighbor_obs=4, neighbor_radius=2.0)._filter_opts is None
    for call in (lambda: w.filter_velocity(np.zeros((3, 4))), w.filter_counts):
        with pytest.raises(ValueError, match="velocity_filter"):
            call()
    # off by default allocates nothing: the set-up returns before it looks at the context
    w._filter_setup(None)
    assert w._filter is None and not hasattr(w, "_filter_u")
    f = dict(alpha=2.0)
    got = _options(neighbor_obs=4, neighbor_radius=2.0, velocity_filter=dict(alpha=3, share=1, floor=0.5))._filter_opts
    assert got == dict(alpha=3.0, buffer_drone=0.0, buffer_obstacle=0.0, share=1.0, floor=0.5)
    assert _options(obstacle_watch=sr.gate(), obstacle_witness="world", obstacle_witnesses=3, velocity_filter=f)._filter_opts["alpha"] == 2.0
    with pytest.raises(ValueError, match="source of rows"):
        _options(velocity_filter=f)
    with pytest.raises(ValueError, match="source of rows"):                  # the one witness is not the witnesses record
        _options(obstacle_watch=sr.gate(), obstacle_witness="world", velocity_filter=f)
    with pytest.raises(ValueError, match="world axes"):
        _options(obstacle_watch=sr.gate(), obstacle_witness="body", obstacle_witnesses=3, velocity_filter=f)
    with pytest.raises(ValueError, match="neighbor_vel=False"):
        _options(neighbor_obs=4, neighbor_radius=2.0, neighbor_vel=False, velocity_filter=f)
    for bad, what in ((dict(), "takes a dict"), (3.0, "takes a dict"), (dict(alpha=2.0, gain=1.0), "unknown keys"),
                      (dict(alpha=-1.0), "alpha"), (dict(alpha=1.0, share=2.0), "share"), (dict(alpha=1.0, buffer_drone=-1.0), "buffer_drone"),
                      (dict(alpha=1.0, floor=float("inf")), "floor")):
        with pytest.raises(ValueError, match=what):
            _options(neighbor_obs=4, neighbor_radius=2.0, velocity_filter=bad)

    class _Sharded:
        is_initialized = staticmethod(lambda: True)
        get_world_size = staticmethod(lambda: 2)

    with pytest.raises(NotImplementedError, match="neighbor_obs on a sharded fleet"):      # the existing refusal fires first
        _options(dist=_Sharded, neighbor_obs=4, neighbor_radius=2.0, velocity_filter=f)
    assert _options(dist=_Sharded, obstacle_watch=sr.gate(), obstacle_witness="world", obstacle_witnesses=2,
                    velocity_filter=f)._filter_opts is not None


def test_env_refusals_before_a_context_is_made():
    from dronesim_amd.envs import CtrlAviary, VelocityAviary
    kw = dict(initial_xyzs=np.zeros((4, 3)), dict_io=False)
    for cls in (CtrlAviary, VelocityAviary):
        with pytest.raises(ValueError, match="source of rows"):
            cls(["tello"], 4, velocity_filter=dict(alpha=2.0), **kw)
        with pytest.raises(ValueError, match="world axes"):
            cls(["tello"], 4, obstacle_watch=sr.gate(), obstacle_witness="body", obstacle_witnesses=2, velocity_filter=dict(alpha=2.0), **kw)
        with pytest.raises(ValueError, match="neighbor_vel=False"):
            cls(["tello"], 4, neighbor_obs=3, neighbor_radius=2.0, neighbor_vel=False, velocity_filter=dict(alpha=2.0), **kw)
        with pytest.raises(ValueError, match="alpha"):
            cls(["tello"], 4, neighbor_obs=3, neighbor_radius=2.0, velocity_filter=dict(alpha=0.0), **kw)
    assert hasattr(VelocityAviary, "step_velocity") and not hasattr(CtrlAviary, "step_velocity")


# ---- the reference on cases with known answers -----------------------------------------------------------------------------------------
def _solve(rows, u):
    """rows: [(a, b)] -> (v, dropped) of one drone, the rows in slots 0, 1, ..."""
    A, b, valid = np.zeros((1, fr.ROWS, 3)), np.zeros((1, fr.ROWS)), np.zeros((1, fr.ROWS), dtype=bool)
    for j, (a, bj) in enumerate(rows):
        A[0, j], b[0, j], valid[0, j] = a, bj, True
    v, d = fr.solve(A, b, valid, np.asarray(u, dtype=np.float64)[None, :])
    return v[0], int(d[0])


def test_reference_on_known_answers():
    a = np.array([0.6, 0.0, 0.8])
    u = np.array([0.5, -0.25, 0.125])
    v, d = _solve([(a, 2.0)], u)                                   # one violated row: the orthogonal projection
    np.testing.assert_allclose(v, u + (2.0 - a @ u) * a, atol=1e-14)
    assert d == 0 and abs(a @ v - 2.0) < 1e-14
    ex, ey, ez = np.eye(3)
    v, d = _solve([(ex, 1.0), (ey, 2.0), (ez, 3.0)], [0.0, 0.0, 0.0])          # three orthogonal planes: their corner
    np.testing.assert_allclose(v, [1.0, 2.0, 3.0], atol=1e-14)
    assert d == 0
    v, d = _solve([(ex, 1.0), (-ex, 0.5), (ey, 0.25)], [0.0, 0.0, 0.0])        # two opposed rows: the second dropped, the third kept
    np.testing.assert_allclose(v, [1.0, 0.25, 0.0], atol=1e-14)
    assert d == 0b010
    u = np.array([2.0, 3.0, 4.0])
    v, d = _solve([(ex, 1.0), (ey, 2.0), (ez, 3.0), (a, -1.0)], u)             # a u that meets everything: its own values
    assert d == 0 and np.array_equal(v, u)
    v, d = _solve([], u)                                                       # no rows
    assert d == 0 and np.array_equal(v, u)
    v, d = _solve([(np.zeros(3), 1.0), (np.zeros(3), -1.0), (ex, 3.0)], u)     # rows without direction: 0 >= b or dropped
    assert d == 0b001 and np.allclose(v, [3.0, 3.0, 4.0])
    # a thin wedge: the vertex runs away, and the value mask says so
    t = 1e-2
    rows = [(np.array([np.sin(t), np.cos(t), 0.0]), 0.5), (np.array([np.sin(t), -np.cos(t), 0.0]), 0.5)]
    A, b, valid = np.zeros((1, fr.ROWS, 3)), np.zeros((1, fr.ROWS)), np.zeros((1, fr.ROWS), dtype=bool)
    for j, (aj, bj) in enumerate(rows):
        A[0, j], b[0, j], valid[0, j] = aj, bj, True
    ref = fr.Ref(A, b, valid, np.zeros((1, 3)))
    np.testing.assert_allclose(ref.v[0], [0.5 / np.sin(t), 0.0, 0.0], atol=1e-9)
    assert ref.value[0] and not ref.decision[0]


def test_rows_from_records_by_hand():
    """One drone, one slot of each kind, the numbers worked out by hand."""
    alpha, share, bd, bo, R = 2.0, 0.5, 0.05, 0.1, 0.25
    pos, vel, u = np.array([[1.0, 2.0, 1.5]]), np.array([[0.5, 0.0, -1.0]]), np.zeros((1, 3))
    wit = (np.array([[0.75]]), np.array([[3]]), np.array([[[-1.0], [0.0], [0.0]]]), np.array([[[0.25], [9.0], [9.0]]]))      # |rel| = c + R = 1
    nb = (np.array([[0]]), np.array([[2.0]]), np.array([[[0.0], [2.0], [0.0]]]), np.array([[[7.0], [-1.0], [7.0]]]))
    A, b, valid = fr.build_rows(pos, vel, u, [R], [R], alpha, share, bd, bo, floor=0.5, offz=[0.25], nb=nb, wit=wit)
    assert valid[0].tolist() == [True, True] + [False] * 7 + [True] + [False] * 15
    np.testing.assert_allclose(A[0, 0], [0, 0, 1]); np.testing.assert_allclose(b[0, 0], -alpha * (1.5 - 0.25 - 0.5 - R))
    np.testing.assert_allclose(A[0, 1], [1, 0, 0]); np.testing.assert_allclose(b[0, 1], 0.25 - alpha * (0.75 - bo))
    np.testing.assert_allclose(A[0, 9], [0, -1, 0])
    h = 2.0 - 2 * R - bd
    np.testing.assert_allclose(b[0, 9], 0.0 + share * (1.0 - alpha * h))
    # what is no row: an unused index or body, a non-finite entry, a vanishing distance; a drone that is not finite has none
    for change in (dict(nb=(np.array([[-1]]),) + nb[1:]), dict(nb=(nb[0], np.array([[0.0]])) + nb[2:]),
                   dict(nb=nb[:3] + (np.array([[[np.nan], [0.0], [0.0]]]),))):
        assert not fr.build_rows(pos, vel, u, [R], [R], alpha, share, bd, bo, nb=change["nb"])[2].any()
    assert not fr.build_rows(pos, vel, u, [R], [R], alpha, wit=(wit[0], np.array([[-1]])) + wit[2:])[2].any()
    assert not fr.build_rows(pos, vel, u, [R], [R], alpha, wit=(np.array([[-R]]),) + wit[1:])[2].any()
    assert fr.build_rows(pos, vel, u, [R], [R], alpha, wit=wit[:3] + (None,))[1][0, 1] == -alpha * 0.75
    for lost in (dict(pos=pos * np.nan), dict(vel=vel + np.inf), dict(u=u * np.nan)):
        kw = dict(pos=pos, vel=vel, u=u)
        kw.update(lost)
        assert not fr.build_rows(kw["pos"], kw["vel"], kw["u"], [R], [R], alpha, floor=0.0, nb=nb, wit=wit)[2].any()


def test_reciprocity_on_the_reference():
    """Two drones head-on, both filtered with share = 1/2: n . (v_i - v_j) = -alpha h between them, to rounding."""
    alpha, R, bd = 1.5, 0.2, 0.1
    pos = np.array([[0.0, 0.0, 1.0], [1.0, 0.1, 1.0]])
    vel = np.array([[2.0, 0.0, 0.0], [-2.5, 0.0, 0.0]])
    u = vel.copy()                                              # both wish to go on as they are
    d = np.linalg.norm(pos[1] - pos[0])
    rel_pos = np.stack([pos[1] - pos[0], pos[0] - pos[1]], 1)[None]           # [1, 3, 2]
    rel_vel = np.stack([vel[1] - vel[0], vel[0] - vel[1]], 1)[None]
    nb = (np.array([[1, 0]]), np.array([[d, d]]), rel_pos, rel_vel)
    A, b, valid = fr.build_rows(pos, vel, u, [R, R], [R, R], alpha, 0.5, bd, 0.0, nb=nb)
    v, dropped = fr.solve(A, b, valid, u)
    assert not dropped.any() and np.abs(v - u).max() > 0.1
    n_hat = (pos[0] - pos[1]) / d                               # from j to i, drone 0's normal
    h = d - 2 * R - bd
    assert abs(n_hat @ (v[0] - v[1]) + alpha * h) < 1e-12
    # with share = 1 a drone alone takes the whole change
    A, b, valid = fr.build_rows(pos, vel, u, [R, R], [R, R], alpha, 1.0, bd, 0.0, nb=nb)
    v1, _ = fr.solve(A, b, valid, u)
    assert abs(n_hat @ (v1[0] - vel[1]) + alpha * h) < 1e-12


# ---- the masks and the float32 figure on every random GPU case, on the reference alone -------------------------------------------------
@pytest.mark.parametrize("spec", fr.RANDOM_CASES, ids=lambda s: f"{s[0]}-{s[4]}")
def test_caps_and_float32_figure_on_a_random_case(spec):
    case, ref = fr.random_ref(spec)
    decision, value = ref.shares()
    figure, mismatches, _ = ref.f32_figure()
    print(f"{case['name']}: decision mask {decision:.4f}, value mask {value:.4f}, float32 figure {figure:.3e} (record {fr.F32_FIGURE:.3e}, "
          f"bar {fr.BAR:.3e}), float32 kept sets that differ outside the decision mask {mismatches}, drones changed "
          f"{float((np.abs(ref.v - ref.u).max(1) > 0).mean()):.3f}, with a dropped row {float((ref.dropped != 0).mean()):.3f}")
    assert (fr.DECISION_CAP, fr.VALUE_CAP, fr.TAU, fr.LIP) == (0.005, 0.06, 1e-3, 8.0)
    assert decision <= fr.DECISION_CAP and value <= fr.VALUE_CAP
    assert figure <= fr.F32_FIGURE and mismatches == 0 and fr.BAR == 4.0 * fr.F32_FIGURE
    assert (np.abs(ref.v - ref.u).max(1) > 0).mean() > 0.5 and (np.abs(ref.v - ref.u).max(1) == 0).any()
    # the reference passes its own four assertions, and a v pushed off a kept row by 4 bars does not
    ref.check(ref.v, ref.dropped, what=case["name"])
    i = int(np.nonzero(ref.kept.any(1) & (np.abs(ref.v - ref.u).max(1) > 0))[0][0])
    worse = ref.v.copy()
    worse[i] += 4.0 * fr.BAR * (ref.u[i] - ref.v[i]) / np.linalg.norm(ref.u[i] - ref.v[i])
    with pytest.raises(AssertionError):
        ref.check(worse, ref.dropped, what="pushed")


def test_the_record_is_the_worst_case_and_the_squeezed_case_is_squeezed():
    worst = max(fr.random_ref(s)[1].f32_figure()[0] for s in fr.RANDOM_CASES)
    assert 0.8 * fr.F32_FIGURE <= worst <= fr.F32_FIGURE
    assert any(fr.random_ref(s)[1].dropped.any() for s in fr.RANDOM_CASES if s[0] == "full")
    case = fr.squeezed_case()
    ref = fr.case_ref(case)
    d = ref.dropped
    four = np.arange(case["n"]) % 4 == 0
    assert np.all(d & 0b0001 == 0)                               # the floor is never dropped
    assert np.all((d & 0b0100) != 0)                             # slot 1 (opposed to slot 0, which was there first) always is
    assert np.all((d & 0b0010) == 0)                             # ... and slot 0 never: obstacle rows in their order
    assert np.all(((d & 0b1000) != 0) == four)                   # slot 2 pushes down against the floor on every fourth drone: it loses
    tilted = np.arange(case["n"]) % 2 == 1
    assert np.all(((d >> fr.NB_BIT) & 1 == 1) == tilted)         # the neighbour row against slot 0 loses, the one across is kept
    decision, value = ref.shares()
    print(f"squeezed: decision mask {decision:.4f}, value mask {value:.4f}")
    assert decision <= fr.GEO_DECISION_CAP and value <= fr.GEO_VALUE_CAP
