"""CPU-side checks of the nearest-neighbour observation (dsim_knn): the ABI surface, the refusals that need no device, the tests' own
fp64 reference (tests/knn_ref.py) on a hand example, the exemption caps of every world the GPU tests use, the env's keyword
validation, and what Downwash.nearest hands the library.  tests/README_knn.md."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

import __graft_entry__ as graft
from tests import knn_ref as kr

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
    assert re.search(r"^int\s+dsim_knn\s*\(", hdr, flags=re.M)
    assert re.search(r"^int64_t\s+dsim_knn_workspace\s*\(", hdr, flags=re.M)
    for f in ("dsim_knn", "dsim_knn_workspace"):
        assert f in nat.EXPORTS and getattr(lib, f) is not None
    assert lib.dsim_knn.argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, nat.View, ctypes.POINTER(nat.KnnArgs)]
    assert lib.dsim_knn_workspace.argtypes == [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]
    assert lib.dsim_knn_workspace.restype is ctypes.c_int64
    # ABI 11.1 stands: new functions and a new struct only
    assert re.search(r"#define DSIM_ABI_VERSION 11\b", hdr) and re.search(r"#define DSIM_ABI_MINOR 1\b", hdr)
    assert (nat.ABI_VERSION, nat.ABI_MINOR) == (11, 1) and lib.dsim_abi_version() == 11 and lib.dsim_abi_minor() == 1
    assert os.path.join(ROOT, "dronesim_amd", "csrc", "dsim_knn.hip") in graft.HIP_DEPS and len(graft.HIP_SRCS) == 6
    fields = [f for f, _ in nat.KnnArgs._fields_]
    lines = ['printf("size %zu\\n", sizeof(dsim_knn_args));']
    lines += [f'printf("{f} %zu\\n", offsetof(dsim_knn_args, {f}));' for f in fields]
    src = tmp_path / "knn.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dronesim_amd.h"\nint main(void) {\n' + "\n".join(lines)
                   + "\nreturn 0; }\n")
    exe = tmp_path / "knn"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(nat.KnnArgs)
    for f in fields:
        assert int(got[f]) == getattr(nat.KnnArgs, f).offset, f
    assert nat.KNN_MAX_K == 16
    # the workspace is the grid's own (the counting-sort form, as dsim_adjacency takes it)
    for m, nx, ny in ((1, 1, 1), (257, 9, 7), (1000, 30, 23), (65536, 300, 200)):
        assert lib.dsim_knn_workspace(m, nx, ny) == lib.dsim_downwash_workspace(m, nx, ny) > 0
    assert lib.dsim_knn_workspace(-1, 4, 4) == -1 and lib.dsim_knn_workspace(4, 0, 4) == -1


def test_library_refuses_before_it_touches_a_device(nat):
    """No context on this machine: every call is DSIM_E_ARG, a null args or grid among them (nothing is dereferenced), and the
    outputs stay as they were."""
    lib = nat.load()
    idx = np.full((4, 64), 99, dtype=np.int32)
    g = nat.DownwashArgs()

    def call(ctx=None, grid=g, k=4, radius=1.5, flags=0, index=idx.ctypes.data, null_args=False):
        a = nat.KnnArgs(ctypes.addressof(grid) if grid is not None else None, radius, k, flags, index, None, None, None, None)
        return lib.dsim_knn(ctx, None, 1, nat.View(), None if null_args else ctypes.byref(a))
    assert call() == -1 and call(null_args=True) == -1 and call(grid=None) == -1 and call(index=None) == -1
    assert np.all(idx == 99)


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def test_reference_on_a_hand_example():
    """Five drones on a line and off it: receiver 0 at the origin; 1 at 1 m, 2 at 0.5 m, 3 at 3 m (outside the radius of 2), 4 at
    (0, 1.2, 0.9) = 1.5 m."""
    pos = np.array([[0, 0, 0], [1, 0, 0], [0.5, 0, 0], [3, 0, 0], [0, 1.2, 0.9]], dtype=np.float64)
    vel = np.array([[1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 0, 0], [0, 0, 2]], dtype=np.float64)
    ref = kr.brute(pos, 2.0, 2, vel32=vel)
    assert ref.count.tolist() == [3, 3, 3, 0, 3]
    assert ref.index.tolist() == [[2, 1], [2, 0], [0, 1], [-1, -1], [0, 2]]
    np.testing.assert_allclose(ref.dist[0], [0.5, 1.0], atol=1e-15)
    np.testing.assert_allclose(ref.sorted_d[0], [0.5, 1.0, 1.5], atol=1e-15)
    assert np.all(np.isposinf(ref.dist[3])) and np.all(ref.rel_pos[3] == 0.0) and np.all(ref.rel_vel[3] == 0.0)
    assert ref.rel_pos[0].tolist() == [[0.5, 0, 0], [1, 0, 0]] and ref.rel_vel[0].tolist() == [[0, 1, 0], [-1, 1, 0]]
    # drone 2 sees 0 and 1 at exactly 0.5 m: a tie (stable: the lower index first); drone 1 sees 3 at exactly the radius: ambiguous
    assert ref.tie.tolist() == [False, False, True, False, False]
    assert ref.edge.tolist() == [False, True, False, True, False]
    assert ref.exempt.tolist() == [False, True, True, True, False]
    # the radius stands in for a missing (k + 1)-th distance: drone 4 has two neighbours, the second within 1e-5 of a radius ...
    d42 = float(np.linalg.norm(pos[4] - pos[2]))
    close = kr.brute(pos, d42 + 0.5e-5, 2)
    assert close.count[4] == 2 and close.tie[4] and close.edge[4]
    # ... and a slice of the world gives world indices
    part = kr.brute(pos, 2.0, 2, 1, 3, vel32=vel)
    assert part.index.tolist() == ref.index[1:3].tolist() and part.count.tolist() == [3, 3]
    # a position that is not finite: no neighbours, nobody's neighbour
    pos[2, 0] = np.nan
    lost = kr.brute(pos, 2.0, 2)
    assert lost.count.tolist() == [2, 2, 0, 0, 2] and lost.index[0].tolist() == [1, 4] and not lost.exempt[2]


def test_exemption_caps_of_the_worlds():
    """For every world the GPU tests use, on the reference alone: at most 1 % of the drones are exempt from the exact comparison,
    and the standard world has what the tests look for — full, short and empty lists and a crowd."""
    for seed in (17, 18, 19):
        pos, _ = kr.standard_world(seed)
        for k in (4, 8, 16):
            ref = kr.brute(pos, kr.RADIUS, k)
            print(f"standard world seed {seed} k {k}: tie {ref.tie.mean():.4f} radius {ref.edge.mean():.4f} full {(ref.count >= k).mean():.2f} "
                  f"busiest {ref.count.max()} alone {(ref.count == 0).mean():.4f}")
            assert ref.exempt.mean() <= kr.EXEMPT_CAP
            assert 0.3 < (ref.count >= k).mean() < 0.95 and ref.count.max() > 100
            if seed == 17:
                assert (ref.count == 0).any() and (ref.count < k).any() and (ref.count > k).mean() > 0.3
    pos, _ = kr.standard_world(17)
    assert kr.brute(pos, 0.8 + 2.0 * 0.0475, 1).exempt.mean() <= kr.EXEMPT_CAP          # (the k = 1 test's radius, near enough)
    assert kr.brute(kr.ragged_world()[0], kr.RADIUS, 8).exempt.mean() <= kr.EXEMPT_CAP
    h = kr.hetero_world()
    assert kr.brute(h, kr.RADIUS, 8).exempt.mean() <= kr.EXEMPT_CAP and kr.brute(h, 1.0, 3).exempt.mean() <= kr.EXEMPT_CAP
    w = kr.slice_world()
    assert kr.brute(w, kr.RADIUS, 8, 300, 700).exempt.mean() <= kr.EXEMPT_CAP
    for k in (3, 4, 7, 8, 16):
        ref = kr.brute(kr.planted_world(k), kr.RADIUS, k)
        assert not ref.exempt[0] and ref.count[0] == k + 1 and ref.index[0].tolist() == list(range(k + 1, 1, -1))
    m = kr.brute(kr.mirror_world(), kr.RADIUS, 4)
    assert m.index[0].tolist() == [3, 1, 2, -1] and m.dist[0, 1] == m.dist[0, 2] and m.tie[0]


# ---- the env's keywords --------------------------------------------------------------------------------------------------------------
class _TwoRanks:
    is_initialized = staticmethod(lambda: True)
    get_world_size = staticmethod(lambda: 2)
    get_rank = staticmethod(lambda: 0)


def test_env_refuses_before_a_context_is_made(nat, monkeypatch):
    from dronesim_amd.envs import CtrlAviary, VelocityAviary, fleet_aviary

    def no_context(*a, **k):
        raise AssertionError("a context was made")
    monkeypatch.setattr(fleet_aviary, "Context", no_context)
    xyz = np.zeros((4, 3))
    make = lambda cls=CtrlAviary, **kw: cls(["tello"], 4, initial_xyzs=xyz, dict_io=False, noise_seed=0, **kw)
    with pytest.raises(ValueError, match="without neighbor_obs"):
        make(neighbor_radius=1.0)
    with pytest.raises(ValueError, match="without neighbor_obs"):
        make(neighbor_vel=False)
    for k in (0, 17, -1, 2.5, True):
        with pytest.raises(ValueError, match="neighbor_obs"):
            make(neighbor_obs=k, neighbor_radius=1.0)
    for r in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="neighbor_radius"):
            make(neighbor_obs=4, neighbor_radius=r)
    with pytest.raises(ValueError, match="neighbor_radius"):
        make(neighbor_obs=4)                                          # (the default neighbourhood_radius is infinite)
    with pytest.raises(NotImplementedError, match="sharded"):
        make(neighbor_obs=4, neighbor_radius=1.0, dist=_TwoRanks())
    with pytest.raises(ValueError, match="without neighbor_obs"):
        make(VelocityAviary, neighbor_radius=1.0)
    # in order: the keywords pass, and the next thing the constructor does is make its context
    for kw in (dict(neighbor_obs=4, neighbor_radius=1.0), dict(neighbor_obs=16, neighbourhood_radius=2.0, neighbor_vel=False)):
        with pytest.raises(AssertionError, match="a context was made"):
            make(**kw)


# ---- what Downwash.nearest hands the library ------------------------------------------------------------------------------------------
class _Lib:
    def __init__(self, log):
        self._log = log

    def __getattr__(self, name):
        def call(*a):
            self._log.append((name, a))
            return 0
        return call


def test_nearest_marshals_the_argument_record(nat):
    import torch
    from dronesim_amd.downwash import Downwash, Neighbors
    log = []
    ctx = types.SimpleNamespace(lib=_Lib(log), handle=11, stream_ptr=lambda: 22, device=torch.device("cpu"), types=[])
    state = types.SimpleNamespace(n=500, n_pad=512, view=lambda: "view", version=0)
    dw = Downwash(ctx, state)
    box = (-4.0, -2.0, 4.0, 2.0)
    nb = dw.nearest(1.5, 6, box=box)
    name, (h, s, n, view, ref) = log[-1]
    assert (name, h, s, n, view) == ("dsim_knn", 11, 22, 500, "view")
    q = ref._obj
    assert isinstance(q, nat.KnnArgs) and (q.k, q.flags) == (6, 0) and q.radius == np.float32(1.5)
    g = ctypes.cast(q.grid, ctypes.POINTER(nat.DownwashArgs)).contents
    assert g.pos_all is None and (g.m, g.m_pad, g.local_offset) == (500, 500, 0) and g.halo is None
    assert g.cell >= np.float32(1.5) and g.cell == np.float32(1.5 * (1.0 + 2.0 ** -10))       # a thousandth above the radius
    assert abs(g.xmin - (-4.0 - g.cell)) < 1e-5 and abs(g.ymin - (-2.0 - g.cell)) < 1e-5 and g.xmin + g.nx * g.cell > 4.0 and g.ymin + g.ny * g.cell > 2.0
    assert [x[0] for x in log].count("dsim_knn_workspace") == 1
    assert nb.index.shape == (6, 500) and nb.dist.shape == (6, 500) and nb.rel_pos.shape == (6, 3, 500) and nb.rel_vel.shape == (6, 3, 500)
    assert nb.count.shape == (500,) and nb.index.dtype == torch.int32 and nb.count.dtype == torch.int32
    assert (q.index_out, q.dist_out, q.rel_pos_out, q.rel_vel_out, q.count_out) == tuple(t.data_ptr() for t in nb)
    # outputs that are not asked for are null pointers and None
    nb = dw.nearest(1.5, 6, box=box, rel_pos=False, rel_vel=False, count=False)
    q = log[-1][1][4]._obj
    assert (q.dist_out, q.rel_pos_out, q.rel_vel_out, q.count_out) == (nb.dist.data_ptr(), None, None, None)
    assert nb.rel_pos is None and nb.rel_vel is None and nb.count is None
    # a record at fixed addresses: the call writes there and returns views of the first n drones
    out = Neighbors(torch.zeros((6, 512), dtype=torch.int32), None, torch.zeros((6, 3, 512)), None, torch.zeros(512, dtype=torch.int32))
    nb = dw.nearest(1.5, 6, out=out, box=box)
    q = log[-1][1][4]._obj
    assert (q.index_out, q.dist_out, q.rel_pos_out, q.rel_vel_out, q.count_out) == (out.index.data_ptr(), None, out.rel_pos.data_ptr(),
                                                                                    None, out.count.data_ptr())
    assert nb.index.data_ptr() == out.index.data_ptr() and nb.index.shape == (6, 500) and nb.dist is None and nb.rel_vel is None
    # the world form: the positions of the world, this block's drones at local_offset, and no relative velocity
    wp = torch.zeros((3, 900))
    dw.nearest(1.5, 2, world_pos=wp, local_offset=300, box=box, rel_vel=False)
    q = log[-1][1][4]._obj
    g = ctypes.cast(q.grid, ctypes.POINTER(nat.DownwashArgs)).contents
    assert (g.m, g.m_pad, g.local_offset, q.k, q.rel_vel_out) == (900, 900, 300, 2, None) and g.pos_all is not None
    # refusals, with nothing handed to the library
    calls = len(log)
    for bad in (dict(radius=1.5, k=0), dict(radius=1.5, k=17), dict(radius=0.0, k=4), dict(radius=float("inf"), k=4),
                dict(radius=float("nan"), k=4), dict(radius=1.5, k=2, world_pos=wp, local_offset=300),
                dict(radius=1.5, k=6, out=out._replace(index=torch.zeros((6, 32), dtype=torch.int32))),
                dict(radius=1.5, k=6, out=out._replace(count=torch.zeros(512))),
                dict(radius=1.5, k=4, out=out)):
        with pytest.raises(ValueError):
            dw.nearest(box=box, **bad)
    assert len(log) == calls
    dw.dist = _TwoRanks()
    with pytest.raises(NotImplementedError):
        dw.nearest(1.5, 4, box=box)
