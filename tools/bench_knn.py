"""Times the nearest-neighbour observation against the adjacency list on the same grid, fleet and radius.

A = dsim_adjacency(max_k = k) (count + up to k indices in grid order), B = dsim_knn(k) (count + the k nearest, sorted, with
distances; "rel": with rel_pos and rel_vel as well).  Both bin the fleet per call on the same counting-sort grid (count, scan,
scatter: the same three launches), so the paired difference is the query kernels'.  Two fleets: "config5" = 65 536 tellos uniform
in 128 x 512 x [0.5, 20.5] m, BASELINE config 5's density (one drone per m^2 of ground), radius 5 m (about 26 neighbours);
"lattice" = 4 194 304 tellos on a 2048 x 2048 lattice of 1 m pitch at z = 0.5, the headline fleet's pitch and height (its 1 024
replicas side by side, not on top of each other), radius 1.5 m (8 neighbours inside).  Device events around batches of --iters
calls behind a warm-up, the two interleaved round by round (tools/bench_passage.py's protocol); one JSON line per case.

    python tools/bench_knn.py [--fleets config5 lattice] [--k 4 8 16] [--iters 20] [--warmup 5] [--pairs 7]
    python tools/bench_knn.py --only B --fleets config5 --k 8 --iters 50      (one side alone: the form a counter run takes)
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fleet_positions(name):
    if name == "config5":
        rng = np.random.default_rng(1234)
        n = 65536
        return np.stack([rng.uniform(0, 128, n), rng.uniform(0, 512, n), rng.uniform(0.5, 20.5, n)], 1), 5.0
    if name == "lattice":
        ij = np.arange(4194304)
        return np.stack([(ij % 2048) * 1.0, (ij // 2048) * 1.0, np.full(ij.size, 0.5)], 1), 1.5
    raise SystemExit(f"unknown fleet {name}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fleets", nargs="+", default=["config5", "lattice"])
    ap.add_argument("--k", type=int, nargs="+", default=[4, 8, 16])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--only", choices=["A", "B"], default=None, help="run one side alone, untimed pairs left out")
    ap.add_argument("--rel", type=int, nargs="+", default=[0, 1], help="B without (0) / with (1) rel_pos and rel_vel")
    a = ap.parse_args()
    import torch
    from dronesim_amd import _native as nat
    from dronesim_amd import fleet, params
    from dronesim_amd.downwash import Downwash
    if not torch.cuda.is_available():
        raise SystemExit("bench_knn needs a HIP device")
    ctx = fleet.Context([params.builtin_type("tello")])
    lib, dev = ctx.lib, ctx.device
    r = lambda x: round(float(x), 2)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters

    for name in a.fleets:
        pos, radius = fleet_positions(name)
        n = pos.shape[0]
        st = fleet.FleetState(ctx, n, "soa")
        st.set_fields(0, torch.from_numpy(np.ascontiguousarray(pos.astype(np.float32).T)))
        vel = np.random.default_rng(5).uniform(-2.0, 2.0, (3, n)).astype(np.float32)
        st.set_fields(7, torch.from_numpy(vel))
        n_pad = st.n_pad
        dw = Downwash(ctx, st)
        first = dw.nearest(radius, 16)                              # chooses the grid both sides use; also the fleet's figures
        grid = dw._knn_args[0]
        cnt = first.count.float()
        shape = {"neighbours_mean": r(cnt.mean().item()), "neighbours_max": int(cnt.max().item()), "cell": r(grid.cell),
                 "cells": [grid.nx, grid.ny], "drones_per_cell": r(n / (grid.nx * grid.ny))}
        view = st.view()
        for k in a.k:
            count = torch.empty((n_pad,), dtype=torch.int32, device=dev)
            lst = torch.empty((k, n_pad), dtype=torch.int32, device=dev)
            dist = torch.empty((k, n_pad), dtype=torch.float32, device=dev)
            rp, rv = (torch.empty((k, 3, n_pad), dtype=torch.float32, device=dev) for _ in range(2))
            fa = lambda: nat.check(lib.dsim_adjacency(ctx.handle, ctx.stream_ptr(), n, view, ctypes.byref(grid), radius, count.data_ptr(),
                                                      lst.data_ptr(), k))
            for rel in a.rel:
                q = nat.KnnArgs(ctypes.addressof(grid), radius, k, 0, lst.data_ptr(), dist.data_ptr(), rp.data_ptr() if rel else None,
                                rv.data_ptr() if rel else None, count.data_ptr())
                fb = lambda: nat.check(lib.dsim_knn(ctx.handle, ctx.stream_ptr(), n, view, ctypes.byref(q)))
                sides = [s for s, on in ((fa, a.only != "B"), (fb, a.only != "A")) if on]
                for _ in range(a.warmup):
                    for f in sides:
                        f()
                torch.cuda.synchronize()
                ta, tb = [], []
                for _ in range(a.pairs):
                    if a.only != "B":
                        ta.append(timed(fa))
                    if a.only != "A":
                        tb.append(timed(fb))
                line = {"what": "dsim_knn vs dsim_adjacency", "fleet": name, "drones": n, "radius": radius, "k": k, "rel_outputs": bool(rel),
                        "iters": a.iters, "pairs": a.pairs, **shape}
                if ta:
                    ta = np.array(ta)
                    line.update({"A_adjacency_us_median": r(np.median(ta)), "A_adjacency_us_min_max": [r(ta.min()), r(ta.max())]})
                if tb:
                    tb = np.array(tb)
                    line.update({"B_knn_us_median": r(np.median(tb)), "B_knn_us_min_max": [r(tb.min()), r(tb.max())]})
                if len(ta) and len(tb):
                    d = tb - ta
                    line.update({"B_minus_A_us_median": r(np.median(d)), "B_minus_A_us_min_max": [r(d.min()), r(d.max())],
                                 "B_over_A_median": round(float(np.median(tb / ta)), 3)})
                print(json.dumps(line), flush=True)
        del st, dw, first
    ctx.close()


if __name__ == "__main__":
    main()
