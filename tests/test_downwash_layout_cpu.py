"""Sizes and predicates of the neighbour downwash's workspaces, pinned on the CPU: dsim_downwash_workspace, _workspace_halo,
_keep_workspace, _keep_ok and _prebin_ok touch no HIP call, so the library answers without a device.  The library derives each size
and the pointers it hands its kernels from ONE description per workspace; the values below were recorded from the library as it
was while sizes were closed formulas written beside the layouts, and every later library must reproduce each of them: a piece added
to a layout moves a number here, in the open, instead of running over a caller-owned buffer.

Boundaries covered (dsim_kernels.h dw_use_buckets, dsim_downwash.hip keep_shape_ok / dw_dense):
 - the bucket form: 65 536 cells against 65 537, and m on either side of 40 entries per cell;
 - bucket form or counting-sort form of the workspace: the bucket form is the larger for every cell count (258 against 3 words per
   cell), so the two sides of that choice are the two sides of dw_use_buckets: both numbers are pinned;
 - kept lists: 2 cell >= 10 + 2 skin (cell 5.2 with skins 0.1 / 0.11, and the pairs that straddle the bound: cell 5.1 with
   0.1 / 0.11, cell 5.2 with 0.2 / 0.21), cells of 10 m, and 128 entries per 5 x 5 neighbourhood (5.12 per cell);
 - the invalid inputs that return -1 (sizes) or 0 (predicates)."""
import math

import pytest

import __graft_entry__ as graft


@pytest.fixture(scope="module")
def lib():
    graft.build()
    from dronesim_amd import _native
    return _native.load()


# ((m, nx, ny), int32 words)
WORKSPACE = [
    ((4000, 10, 10), 41816),
    ((4001, 10, 10), 16310),
    ((1, 1, 1), 278),
    ((40, 1, 1), 434),
    ((41, 1, 1), 173),
    ((0, 3, 3), 2338),
    ((65536, 256, 256), 17170448),
    ((65536, 65537, 1), 458761),
    ((65536, 1, 65537), 458761),
    ((2621440, 256, 256), 27394064),
    ((2621441, 256, 256), 10682378),
    ((65536, 52, 52), 959792),
    ((1600, 8, 8), 22928),
    ((100000, 10, 10), 400306),
    ((7, 3, 5), 3914),
    ((4194304, 410, 410), 17281522),
    ((-1, 4, 4), -1),
    ((10, 0, 4), -1),
    ((10, 4, 0), -1),
    ((10, -1, 4), -1),
]
# ((n, h, nx, ny), words): the local grid with the halo grid behind it, or the one-grid form where that is larger
WORKSPACE_HALO = [
    ((3000, 1000, 10, 10), 67636),
    ((3000, 1001, 10, 10), -1),
    ((65536, 4096, 52, 52), 1673828),
    ((1, 0, 1, 1), 556),
    ((40, 0, 1, 1), 712),
    ((40, 1, 1, 1), -1),
    ((1000, 0, 256, 256), 33820612),
    ((1000, 0, 65537, 1), -1),
    ((0, 10, 4, 4), -1),
    ((10, -1, 4, 4), -1),
    ((10, 10, 0, 4), -1),
    ((10, 10, 4, 0), -1),
]
# ((n_pad, nx, ny), words)
KEEP_WORKSPACE = [
    ((1, 1, 1), 1796),
    ((1600, 8, 8), 118064),
    ((65536, 52, 52), 4977968),
    ((65792, 51, 53), 4977248),
    ((256, 256, 256), 114295856),
    ((0, 4, 4), -1),
    ((16, 0, 4), -1),
    ((16, 4, 0), -1),
]
# ((m, nx, ny, cell, skin), 0 / 1)
KEEP_OK = [
    ((65536, 50, 50, 5.2, 0.1), 1),
    ((65536, 50, 50, 5.2, 0.11), 1),
    ((65536, 50, 50, 5.1, 0.1), 1),
    ((65536, 50, 50, 5.1, 0.11), 0),
    ((65536, 50, 50, 5.2, 0.2), 1),
    ((65536, 50, 50, 5.2, 0.21), 0),
    ((65536, 50, 50, 5.0, 0.1), 0),
    ((65536, 50, 50, 10.0, 0.1), 0),
    ((65536, 50, 50, 9.99, 0.1), 1),
    ((512, 10, 10, 5.2, 0.1), 0),
    ((513, 10, 10, 5.2, 0.1), 1),
    ((128, 5, 5, 5.2, 0.1), 0),
    ((129, 5, 5, 5.2, 0.1), 1),
    ((327, 8, 8, 5.2, 0.1), 0),
    ((328, 8, 8, 5.2, 0.1), 1),
    ((4000, 10, 10, 5.2, 0.1), 1),
    ((4001, 10, 10, 5.2, 0.1), 0),
    ((400000, 256, 256, 5.2, 0.1), 1),
    ((400000, 65537, 1, 5.2, 0.1), 0),
    ((0, 10, 10, 5.2, 0.1), 0),
    ((1000, 0, 10, 5.2, 0.1), 0),
    ((1000, 10, 0, 5.2, 0.1), 0),
    ((1000, 10, 10, 5.2, 0.0), 0),
    ((1000, 10, 10, 5.2, -0.1), 0),
    ((1000, 10, 10, 5.2, math.nan), 0),
    ((1000, 10, 10, 0.0, 0.1), 0),
    ((1000, 10, 10, math.nan, 0.1), 0),
]
# ((m, nx, ny), 0 / 1)
PREBIN_OK = [
    ((4000, 10, 10), 1),
    ((4001, 10, 10), 0),
    ((65536, 256, 256), 1),
    ((65536, 65537, 1), 0),
    ((2621440, 256, 256), 1),
    ((2621441, 256, 256), 0),
    ((1, 1, 1), 1),
    ((0, 4, 4), 0),
    ((-1, 4, 4), 0),
    ((10, 0, 4), 0),
    ((10, 4, 0), 0),
]


@pytest.mark.parametrize("name,table", [("dsim_downwash_workspace", WORKSPACE), ("dsim_downwash_workspace_halo", WORKSPACE_HALO),
                                        ("dsim_downwash_keep_workspace", KEEP_WORKSPACE), ("dsim_downwash_keep_ok", KEEP_OK),
                                        ("dsim_downwash_prebin_ok", PREBIN_OK)])
def test_sizes_and_predicates_are_what_they_were(lib, name, table):
    got = [(args, int(getattr(lib, name)(*args))) for args, _ in table]
    assert [g for _, g in got] == [want for _, want in table], [(a, g, w) for (a, g), (_, w) in zip(got, table) if g != w]

