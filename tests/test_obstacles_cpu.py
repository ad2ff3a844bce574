"""CPU-side checks of the static-obstacle watch: the ABI surface, the .obj / .urdf readers on the reference's gate, what the host
grid builder refuses, and the completeness of its cell lists against a brute-force fp64 point-triangle distance."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as graft
from tests.obstacle_ref import tri_dist


@pytest.fixture(scope="module")
def nat():
    graft.build()
    from dronesim_amd import _native
    return _native


FUNCS = ("dsim_obstacle_grid_plan", "dsim_obstacle_grid_build", "dsim_obstacles_create", "dsim_obstacles_destroy",
         "dsim_obstacle_clearance")


def test_header_declares_and_library_exports_the_five_functions(nat):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "dronesim_amd.h")).read()
    lib = nat.load()
    for f in FUNCS:
        assert re.search(rf"^int\s+{f}\s*\(", hdr, flags=re.M), f
        assert f in nat.EXPORTS and getattr(lib, f) is not None
    assert re.search(r"DSIM_Q_OBSTACLE_CONTACTS\s*=\s*7", hdr) and nat.QUERY_OBSTACLE_CONTACTS == 7
    assert re.search(r"#define DSIM_ABI_VERSION 11\b", hdr) and re.search(r"#define DSIM_ABI_MINOR 1\b", hdr)
    assert lib.dsim_abi_version() == 11 and lib.dsim_abi_minor() == 1
    assert os.path.join(root, "dronesim_amd", "csrc", "dsim_obstacles.hip") in graft.HIP_SRCS and len(graft.HIP_SRCS) == 6


def test_grid_struct_matches_c(nat, tmp_path):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['printf("size %zu\\n", sizeof(dsim_obstacle_grid));']
    lines += [f'printf("{f} %zu\\n", offsetof(dsim_obstacle_grid, {f}));' for f, _ in nat.ObstacleGrid._fields_]
    src = tmp_path / "grid.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dronesim_amd.h"\nint main(void) {\n' + "\n".join(lines)
                   + "\nreturn 0; }\n")
    exe = tmp_path / "grid"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(root, "include"), "-o", str(exe), str(src)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(nat.ObstacleGrid)
    for f, _ in nat.ObstacleGrid._fields_:
        assert int(got[f]) == getattr(nat.ObstacleGrid, f).offset, f


# ---- readers ---------------------------------------------------------------------------------------------------------------------
def test_gate_fixture_through_the_readers(nat, golden_dir):
    from dronesim_amd.obstacles import ObstacleSet, read_obj
    v, f = read_obj(os.path.join(golden_dir, "Gate_50_curved.obj"))
    assert v.shape == (48, 3) and f.shape == (96, 3)
    s = ObstacleSet.from_urdf(os.path.join(golden_dir, "gate_50_curved.urdf"), (0, 0, 0), (0, 0, 0))
    assert s.n_tri == 96 and s.n_bodies == 1
    lo, hi = s.aabb
    np.testing.assert_allclose(hi, [0.07, 0.56, 0.4], rtol=0, atol=1e-7)         # the URDF's scale 1.4 x 1.4 x 1.0
    np.testing.assert_allclose(lo, [-0.07, -0.56, -0.4], rtol=0, atol=1e-7)
    # the gate centre is 0.25 m from the nearest triangle (fp64, on the scaled fp64 vertices)
    tri64 = (v * np.array([1.4, 1.4, 1.0]))[f]
    assert abs(tri_dist(np.zeros((1, 3)), tri64).min() - 0.25) <= 1e-9
    # the same set from the .obj directly, and placed: position and yaw move the box
    o = ObstacleSet.from_obj(os.path.join(golden_dir, "Gate_50_curved.obj"), scale=(1.4, 1.4, 1.0))
    np.testing.assert_array_equal(o.triangles, s.triangles)
    p = ObstacleSet.from_urdf(os.path.join(golden_dir, "gate_50_curved.urdf"), (0.5, 1.0, 5.0), (0, 0, np.pi / 2))
    np.testing.assert_allclose(p.aabb[1], [0.5 + 0.56, 1.0 + 0.07, 5.4], rtol=0, atol=1e-6)
    both = s + p
    assert both.n_tri == 192 and both.n_bodies == 2 and list(np.unique(both.body)) == [0, 1] and both.body[96] == 1


def test_obj_reader_forms_and_fans(tmp_path):
    from dronesim_amd.obstacles import ObstacleSet, read_obj
    path = tmp_path / "m.obj"
    path.write_text("# c\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nv 0.5 2 0\nvn 0 0 1\nvt 0 0\n"
                    "f 1 2 3\nf 1/1 3/1 4/1\nf 1/1/1 2/1/1 3/1/1 4/1/1 5/1/1\nf 1//1 2//1 -1//1\n")
    v, f = read_obj(str(path))
    assert v.shape == (5, 3)
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 1, 4]]
    b = ObstacleSet.box((1, 2, 3), (2, 4, 6))
    assert b.n_tri == 12 and b.aabb[0].tolist() == [0, 0, 0] and b.aabb[1].tolist() == [2, 4, 6]
    # twelve triangles that close the box: area 2 (ab + bc + ca)
    t = b.triangles.astype(np.float64)
    assert abs(0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1).sum() - 2 * (8 + 24 + 12)) < 1e-9


URDF = """<?xml version="1.0" ?>
<robot name="x"><link {link} name="base_link">
<collision {col}><origin rpy="0 0 0" xyz="0 0 0.5"/><geometry>{shape}</geometry></collision>
</link></robot>
"""


def test_urdf_refusals_and_box(tmp_path, golden_dir):
    from dronesim_amd.obstacles import ObstacleSet
    mesh = f'<mesh filename="{os.path.join(golden_dir, "Gate_50_curved.obj")}" scale="1 1 1"/>'

    def urdf(link="", col="", shape=mesh):
        p = tmp_path / "b.urdf"
        p.write_text(URDF.format(link=link, col=col, shape=shape))
        return str(p)
    with pytest.raises(ValueError, match="concave"):
        ObstacleSet.from_urdf(urdf(), (0, 0, 0), (0, 0, 0))                       # Bullet would use the convex hull
    assert ObstacleSet.from_urdf(urdf(link='concave="yes"'), (0, 0, 0), (0, 0, 0)).n_tri == 96
    assert ObstacleSet.from_urdf(urdf(col='concave="yes"'), (0, 0, 0), (0, 0, 0)).n_tri == 96
    with pytest.raises(ValueError, match="sphere"):
        ObstacleSet.from_urdf(urdf(shape='<sphere radius="0.1"/>'), (0, 0, 0), (0, 0, 0))
    with pytest.raises(ValueError, match="cylinder"):
        ObstacleSet.from_urdf(urdf(shape='<cylinder radius="0.1" length="1"/>'), (0, 0, 0), (0, 0, 0))
    b = ObstacleSet.from_urdf(urdf(shape='<box size="1 2 3"/>'), (10, 0, 0), (0, 0, 0))
    assert b.n_tri == 12 and b.aabb[0].tolist() == [9.5, -1.0, -1.0] and b.aabb[1].tolist() == [10.5, 1.0, 2.0]


def test_urdf_with_joints_or_several_links_is_refused(tmp_path):
    """Joint origins are not composed: a body of more than one link would be misplaced, so it is refused."""
    from dronesim_amd.obstacles import ObstacleSet
    link = '<link name="{n}"><collision><geometry><box size="1 1 1"/></geometry></collision></link>'
    joint = '<joint name="j" type="fixed"><parent link="a"/><child link="b"/><origin xyz="0 0 2"/></joint>'
    p = tmp_path / "two.urdf"
    p.write_text(f'<robot name="x">{link.format(n="a")}{link.format(n="b")}{joint}</robot>')
    with pytest.raises(ValueError, match="2 links and 1 joints"):
        ObstacleSet.from_urdf(str(p), (0, 0, 0), (0, 0, 0))
    p.write_text(f'<robot name="x">{link.format(n="a")}{link.format(n="b")}</robot>')
    with pytest.raises(ValueError, match="2 links and 0 joints"):
        ObstacleSet.from_urdf(str(p), (0, 0, 0), (0, 0, 0))
    p.write_text(f'<robot name="x">{link.format(n="a")}</robot>')
    assert ObstacleSet.from_urdf(str(p), (0, 0, 0), (0, 0, 0)).n_tri == 12


# ---- the host grid ---------------------------------------------------------------------------------------------------------------
def _plan(nat, tri, reach):
    tri = np.ascontiguousarray(tri, dtype=np.float32).reshape(-1, 9)
    g = nat.ObstacleGrid()
    rc = nat.load().dsim_obstacle_grid_plan(tri.ctypes.data, tri.shape[0], float(reach), ctypes.byref(g))
    return rc, g


def test_plan_refusals_write_nothing(nat):
    lib = nat.load()
    tri = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1, 1, 0, 1, 0, 1, 1]], dtype=np.float32)
    untouched = bytes(nat.ObstacleGrid())
    ok, g = _plan(nat, tri, 0.5)
    assert ok == 0 and g.nx * g.ny * g.nz <= 1 << 18 and g.list_len > 0 and g.reach == 0.5
    for bad_reach in (0.0, -1.0, float("nan"), float("inf")):
        rc, g = _plan(nat, tri, bad_reach)
        assert rc == -1 and bytes(g) == untouched
    flat = tri.copy()
    flat[1, 6:9] = flat[1, 0:3] + 2.0 * (flat[1, 3:6] - flat[1, 0:3])              # c on the line a b: zero area
    rc, g = _plan(nat, flat, 0.5)
    assert rc == -1 and bytes(g) == untouched
    tiny = tri.copy()
    tiny[1, 3:9] = np.tile(tiny[1, 0:3], 2) + np.array([1e-6, 0, 0, 0, 1e-6, 0], dtype=np.float32)   # 5e-13 m^2
    assert _plan(nat, tiny, 0.5)[0] == -1
    nan = tri.copy()
    nan[0, 4] = np.nan
    assert _plan(nat, nan, 0.5)[0] == -1
    g = nat.ObstacleGrid()
    assert lib.dsim_obstacle_grid_plan(tri.ctypes.data, 0, 0.5, ctypes.byref(g)) == -1
    assert lib.dsim_obstacle_grid_plan(tri.ctypes.data, 65537, 0.5, ctypes.byref(g)) == -1
    assert lib.dsim_obstacle_grid_plan(None, 2, 0.5, ctypes.byref(g)) == -1
    assert bytes(g) == untouched
    # a soup a kilometre long with a small reach: the edge is doubled until the caps hold
    far = np.concatenate([tri, tri + np.float32(1000.0)])
    ok, g = _plan(nat, far, 0.05)
    assert ok == 0 and g.nx * g.ny * g.nz <= 1 << 18 and max(g.nx, g.ny, g.nz) <= 4096 and g.cell > 0.05
    # build refuses a grid that is not the plan of the soup, with nothing written
    ok, g = _plan(nat, tri, 0.5)
    start = np.full(g.nx * g.ny * g.nz + 1, -3, dtype=np.int32)
    lst = np.full(g.list_len, -3, dtype=np.int32)
    g.nx += 1
    assert lib.dsim_obstacle_grid_build(tri.ctypes.data, 2, ctypes.byref(g), start.ctypes.data, lst.ctypes.data) == -1
    assert (start == -3).all() and (lst == -3).all()


def _soup():
    rng = np.random.default_rng(2024)
    ctr = rng.uniform(-9.2, 9.2, (3000, 1, 3))
    return (ctr + rng.uniform(-0.75, 0.75, (3000, 3, 3))).astype(np.float32)


def _gate(golden_dir):
    from dronesim_amd.obstacles import ObstacleSet
    return ObstacleSet.from_urdf(os.path.join(golden_dir, "gate_50_curved.urdf"), (0.5, 1.0, 5.0), (0, 0, 0)).triangles


@pytest.mark.parametrize("what, reach", [("gate", 1.158), ("gate", 0.3), ("one", 0.75), ("soup", 0.9)])
def test_cell_lists_are_complete(nat, golden_dir, what, reach):
    """Every triangle whose fp64 brute-force distance to a point is below `reach` is in the list of the point's cell, for
    20 000 random points in the grown box; points outside the grown box have no triangle within `reach`."""
    from dronesim_amd.obstacles import ObstacleSet
    tri = {"gate": lambda: _gate(golden_dir), "soup": _soup,
           "one": lambda: np.array([[[0.0, 0.0, 1.0], [2.0, 0.0, 1.0], [0.5, 1.5, 1.3]]], dtype=np.float32)}[what]()
    s = ObstacleSet(tri, 0)
    g, start, lst = s.grid(reach)
    cells, T = g.nx * g.ny * g.nz, s.n_tri
    assert cells <= 1 << 18 and start[0] == 0 and start[-1] == g.list_len == len(lst) and (np.diff(start) >= 0).all()
    assert lst.min() >= 0 and lst.max() < T
    lo, hi = np.array(list(g.lo), dtype=np.float64), np.array(list(g.hi), dtype=np.float64)
    vmin, vmax = tri.reshape(-1, 3).min(0).astype(np.float64), tri.reshape(-1, 3).max(0).astype(np.float64)
    r32 = float(np.float32(reach))
    assert (lo <= vmin - r32).all() and (hi >= vmax + r32).all() and (lo > vmin - 1.001 * r32 - 1e-5).all()
    assert list(g.origin) == list(g.lo) and (lo + np.array([g.nx, g.ny, g.nz]) * float(g.cell) > hi).all()
    key = np.unique(np.repeat(np.arange(cells, dtype=np.int64), np.diff(start)) * T + lst)
    assert len(key) == len(lst)                                                  # no triangle twice in a cell
    rng = np.random.default_rng(7)
    pts = rng.uniform(lo, hi, (20000, 3))
    missing = within = 0
    nn = np.array([g.nx, g.ny, g.nz])
    for k0 in range(0, len(pts), 1000):
        p = pts[k0:k0 + 1000]
        c3 = np.clip(np.floor((p - lo) / float(g.cell)).astype(np.int64), 0, nn - 1)
        cell = (c3[:, 2] * g.ny + c3[:, 1]) * g.nx + c3[:, 0]
        pi, ti = np.nonzero(tri_dist(p, tri, chunk=125) < r32)
        within += len(pi)
        missing += int((~np.isin(cell[pi] * T + ti, key)).sum())
    assert within > 1000 and missing == 0, (within, missing)
    out = rng.uniform(lo - 2.0 * r32, hi + 2.0 * r32, (3000, 3))
    out = out[((out < lo) | (out > hi)).any(1)]
    assert len(out) > 500 and tri_dist(out, tri, chunk=125).min() >= r32
