"""The range scanner where it meets OTHER DRONES, at the edges case_lattice never shows it (tests/README_scan.md): the DRONES block of
k_range_scan is the camera's 2-D grid walk (dsim_camera_drones.inc, included by both), and this is its edge suite.  Level drones
whose axis beams have components of d that are exactly 0, drones stacked above one another, a second and ragged tile, cell borders through the drones'
centres, a fleet 4 km from the origin, task offsets beside a set, lost drones as targets, a doubled cell, beam chunks over
blockIdx.y, and beams "used as given" through the raw ABI.

The references are scan_ref.scan_brute (fp64, no grid); the rule is test_gpu_scan.py's: outside the mask (at most 1 % of each case's
rays, asserted on the CPU) hit / no-hit and ids EXACTLY, t within SCAN_EDGE_TOL (= SCAN_TOL: the edge cases' restated error is not
above the recorded one).  tests/test_scan_cpu.py shows without a device that the walk AS DESIGNED finds every sphere on these very
inputs (walked_scan == restated_scan bit for bit); what is tested here is whether the HIP text does what the design says."""
import numpy as np
import pytest
import torch

from dronesim_amd import params
from tests import scan_ref as sf
from tests.test_gpu_scan import check, gpu, load, raw_call, scan, tello_ctx  # noqa: F401  (gpu: the fixture)

pytestmark = pytest.mark.gpu
TOL = sf.SCAN_EDGE_TOL


def stack_scanner(fleet, c, world=None, layout="soa", limits=sf.STACK_LIMITS, **kw):
    """A scanner over one of the stack cases: the mixed two-type context, the fleet stored in the caller's order with its type_id."""
    from dronesim_amd.scanner import RangeScanner
    ctx = fleet.Context([params.builtin_type(m) for m in sf.STACK_MODELS])
    state = load(fleet, ctx, c["st"], layout)
    tid = torch.zeros((state.n_pad,), dtype=torch.uint8, device=ctx.device)
    tid[: state.n] = torch.from_numpy((np.arange(state.n) % 2).astype(np.uint8)).to(ctx.device)
    t_min, t_max, rng = limits
    return RangeScanner(ctx, state, world, c["beams"], t_min, t_max, type_id=tid, drones=True, drone_range=rng, **kw)


def same_grid(sc, grid):
    """The scanner binned on the grid the CPU's walked_scan was shown to be right on."""
    cell, xmin, ymin, nx, ny = grid
    return sc._grid.cell == cell and tuple(sc._grid._box) == (xmin, ymin, nx, ny)


def nobody_sees_itself(h):
    from dronesim_amd.scanner import RangeScanner
    who = RangeScanner.hit_drone(h)
    return not (who == np.arange(h.shape[1])[None, :]).any()


@pytest.mark.parametrize("box", ["measured", "pinned"])
@pytest.mark.parametrize("layout", ["soa", "tile64"])
def test_axis_beams_among_stacked_drones(gpu, layout, box):
    nat, fleet = gpu
    c = sf.case_stack()
    st, rad = c["st"], c["rad"]
    sc = stack_scanner(fleet, c, layout=layout)
    assert sc.state.n == 300 and sc.state.n_pad > 300           # two tiles, the second ragged
    t, h = scan(sc)
    if box == "pinned":
        pinned = stack_scanner(fleet, c, layout=layout, drone_box=sf.stack_pinned_box())
        tp, hp = scan(pinned)
        assert same_grid(pinned, sf.scan_grid(st, sf.stack_pinned_box())) and pinned.drones_outside() >= 20
        assert np.array_equal(tp, t) and np.array_equal(hp, h)  # bit-equal to the measured box's
        t, h = tp, hp
    else:
        assert same_grid(sc, sf.scan_grid(st)) and sc.drones_outside() == 0
    check(f"stack, {layout}, {box} box", t, h, c["ref"], tol=TOL)
    assert nobody_sees_itself(h)
    # the up beam of a bottom-layer drone on an unshifted column: the drone 100 above it, at 0.75 m less that drone's radius
    i = np.nonzero(np.arange(100) % 5 != 3)[0]
    assert np.array_equal(st[i + 100, :2], st[i, :2]) and np.array_equal(h[4, i], -3 - (i + 100))
    want = 0.75 - rad[i + 100].astype(np.float64)
    assert (np.abs(t[4, i] - want) / want).max() <= TOL
    down = 0.75 - rad[i].astype(np.float64)                    # ... and that drone's down beam: the one below
    assert np.array_equal(h[5, i + 100], -3 - i) and (np.abs(t[5, i + 100] - down) / down).max() <= TOL
    assert int((h[:, 256:] <= -3).sum()) >= 200                 # the second tile's lanes see, and are seen
    assert int(((h <= -3) & (-3 - h >= 256)).sum()) >= 200


def test_a_fleet_far_from_the_origin(gpu):
    nat, fleet = gpu
    c, near = sf.case_stack(sf.FAR_SHIFT), sf.case_stack()
    assert not near["ref"]["ambiguous"].any() and not c["ref"]["ambiguous"].any()
    sc = stack_scanner(fleet, c)
    t, h = scan(sc)
    assert same_grid(sc, sf.scan_grid(c["st"]))
    check("stack, 4 km out, measured box", t, h, c["ref"], tol=TOL)
    assert np.array_equal(h, near["ref"]["hit"])               # the near fleet's ids
    pinned = stack_scanner(fleet, c, drone_box=sf.stack_pinned_box(sf.FAR_SHIFT))
    tp, hp = scan(pinned)
    assert same_grid(pinned, sf.scan_grid(c["st"], sf.stack_pinned_box(sf.FAR_SHIFT))) and pinned.drones_outside() >= 20
    check("stack, 4 km out, pinned box", tp, hp, c["ref"], tol=TOL)
    assert np.array_equal(tp, t) and np.array_equal(hp, h)


@pytest.mark.parametrize("subdiv", [0, 2])
def test_offsets_with_a_set_and_drones(gpu, subdiv):
    nat, fleet = gpu
    from dronesim_amd.obstacles import ObstacleScenes
    c = sf.case_stack_offsets(subdiv)
    sc = stack_scanner(fleet, c, c["sc"], ground=True, offsets=c["off"])
    t, h = scan(sc)
    check(f"stack, offsets, scene({subdiv})", t, h, c["ref"], tol=TOL)
    assert nobody_sees_itself(h) and int((h >= 0).sum()) >= 20 and int((h == -2).sum()) >= 100 and int((h <= -3).sum()) >= 2000
    # the same through the identity placement: the PLACED + DRONES instances with offsets
    placed = stack_scanner(fleet, c, ObstacleScenes(c["sc"], np.zeros((1, 1, 3)), np.zeros((1, 1, 3))), ground=True, offsets=c["off"],
                           scene_id=np.zeros(300, dtype=np.int64))
    tp, hp = scan(placed)
    assert np.array_equal(tp, t) and np.array_equal(hp, h)
    sc.close()
    placed.close()


def test_lost_drones_are_not_seen_and_see_nothing(gpu):
    nat, fleet = gpu
    from dronesim_amd.scanner import RangeScanner
    c = sf.case_stack_lost()
    lost = list(sf.STACK_LOST)
    sc = stack_scanner(fleet, c, c["sc"], ground=True, offsets=c["off"])
    raw = sc.state.rigid_aos()
    assert np.isnan(raw[55, 0]) and np.isinf(raw[155, 1]) and not raw[255, 3:7].any()
    t, h = scan(sc)
    assert np.isinf(t[:, lost]).all() and (t[:, lost] > 0).all() and (h[:, lost] == -1).all()
    who = RangeScanner.hit_drone(h)
    assert not np.isin(who, lost[:2]).any() and int((who == 255).sum()) >= 1
    rest = np.setdiff1d(np.arange(300), lost)
    check("stack, lost drones", t[:, rest], h[:, rest], {k: v[:, rest] for k, v in c["ref"].items()}, tol=TOL)
    # the box is measured over the drones whose position is finite: not stretched to the origin, 70 m away
    assert same_grid(sc, sf.scan_grid(c["st"])) and sc.drones_outside() == 0
    sc.close()


def test_long_walks_over_doubled_cells(gpu):
    nat, fleet = gpu
    c = sf.case_sparse()
    sc = stack_scanner(fleet, c, limits=(sf.STACK_LIMITS[0], sf.SPARSE_RANGE, sf.SPARSE_RANGE))
    t, h = scan(sc)
    assert same_grid(sc, sf.scan_grid(c["st"])) and sc._grid.cell >= 4.0 * sf.scan_grid(sf.case_stack()["st"])[0]
    check("sparse layer, doubled cells", t, h, c["ref"], tol=TOL)
    assert nobody_sees_itself(h) and int((h <= -3).sum()) >= 200 and float(t[h <= -3].max()) > 15.0


def test_beam_chunks_with_drones(gpu):
    nat, fleet = gpu
    c = sf.case_big()
    n, B, sample = sf.BIG_N, c["beams"].shape[0], c["sample"]
    tiles = (n + 255) // 256
    want = min(B, -(-1024 // tiles))
    assert -(-B // -(-B // want)) == 4                          # the host's rule (dsim_scan.hip: scan_beams_per_block): 3, 3, 3 and 1
    sc = stack_scanner(fleet, c)
    t, h = scan(sc)
    check("65 536 drones, 4 beam chunks, 512 sampled lanes", t[:, sample], h[:, sample], c["ref"], tol=TOL)
    assert nobody_sees_itself(h)
    t2, _ = scan(sc, hits=False)
    assert np.array_equal(t, t2)


def test_beams_are_used_as_given(gpu):
    """The raw ABI: d = R beam is not normalised, t is in units of |beam|, and a beam that is zero, not finite or of a squared
    length that float32 does not hold misses, without disturbing its neighbours or the reach of the good ones."""
    nat, fleet = gpu
    from dronesim_amd.downwash import Downwash
    c = sf.case_raw_beams()
    ctx = tello_ctx(fleet)
    st = load(fleet, ctx, c["st"])
    n = st.n
    dev = c["sc"].to_device(ctx, 1.0).enable_rays()
    good, bad = list(sf.RAW_GOOD), list(sf.RAW_BAD)

    def run(table, **kw):
        tb = torch.from_numpy(np.ascontiguousarray(table, dtype=np.float32)).to(ctx.device)
        r_out = torch.full((tb.shape[0], st.n_pad), -7.0, dtype=torch.float32, device=ctx.device)
        h_out = torch.full((tb.shape[0], st.n_pad), -7, dtype=torch.int32, device=ctx.device)
        assert raw_call(nat, ctx, st, tb, r_out, h_out, **kw) == 0
        torch.cuda.synchronize()
        assert bool((r_out[:, n:] == -7.0).all()) and bool((h_out[:, n:] == -7).all()) and not bool((r_out[:, :n] == -7.0).any())
        return r_out[:, :n].cpu().numpy().astype(np.float64), h_out[:, :n].cpu().numpy()
    t, h = run(c["beams"], h=dev.handle, flags=nat.SCAN_GROUND)
    check("raw table, the good rows", t[good], h[good], c["ref"], tol=TOL)
    assert np.isinf(t[bad]).all() and (t[bad] > 0).all() and (h[bad] == -1).all()
    tc, hc = run(c["beams"], h=dev.handle, flags=nat.SCAN_GROUND | nat.SCAN_CLAMP)
    assert np.array_equal(tc[bad], np.full((5, n), 8.0)) and (hc[bad] == -1).all()
    check("raw table, clamped", tc[good], hc[good], c["ref"], tol=TOL, miss=8.0)
    # the last unit beam, scanned alone: bit-equal
    t1, h1 = run(c["beams"][11:], h=dev.handle, flags=nat.SCAN_GROUND)
    assert np.array_equal(t1[0], t[11]) and np.array_equal(h1[0], h[11]) and int((h1 == -2).sum()) >= 400
    # the bad rows alone with t_min = 0: a beam of 2e19 has d . d = inf and -ez / dz of 1e-19; it must not report the ground
    t0, h0 = run(c["beams"][bad], h=dev.handle, flags=nat.SCAN_GROUND, t_min=0.0)
    assert np.isinf(t0).all() and (t0 > 0).all() and (h0 == -1).all()
    dev.close()

    # the scaling law: beams times 2^k with t_min, t_max and the drones' range times 2^-k.  Every operation on d scales by an exact
    # power of two (no overflow, nothing subnormal at these sizes), so the ranges are 2^-k times the unit scan's BIT FOR BIT.
    lat = sf.case_lattice("set")
    st = load(fleet, ctx, lat["st"])
    n = st.n
    dev = sf.lattice_scene(0).to_device(ctx, 1.0).enable_rays()
    binner = Downwash(ctx, st, None, None)                     # (kept: it owns the grid's workspace)
    grid = binner.sphere_grid(None)
    outside = torch.zeros((1,), dtype=torch.int64, device=ctx.device)
    unit = sf.fan(8, down=True)

    def scaled(k):
        s = 2.0 ** k
        return run(unit * np.float32(s), h=dev.handle, flags=nat.SCAN_GROUND, t_min=0.05 / s, t_max=8.0 / s, grid=grid, outside=outside,
                   drones={"range": 6.0 / s})
    tu, hu = scaled(0)
    assert int((hu >= 0).sum()) >= 20 and int((hu == -2).sum()) >= 100 and int((hu <= -3).sum()) >= 100
    for k in (-6, -1, 3, 6):
        tk, hk = scaled(k)
        differ = np.argwhere((tk != tu * 2.0 ** -k) | (hk != hu))
        print(f"beams x 2^{k}: {len(differ)} of {tu.size} rays differ from 2^{-k} x the unit scan", [(int(b), int(i), tk[b, i], tu[b, i] * 2.0 ** -k) for b, i in differ[:5]])
        assert len(differ) == 0
    dev.close()
