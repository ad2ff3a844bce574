"""Times the swept drone-drone contact watch against the point watch it stands beside: A = dsim_clearance, B = dsim_clearance_sweep,
the same fleet and margin, each on the grid its own cell rule asks for.  N robobees at the density of BASELINE config 5 (one per m^2
of ground: 65 536 uniform in a 128 x 512 x [0.5, 20.5] m box), chords of --chord metres in uniform directions behind every drone,
travel = the chord.  Device events around batches of --iters calls behind a warm-up, A and B interleaved in pairs; prints one JSON
line with the median and the spread of both and of the paired ratio.  B runs with KEEP_PREV, so every call sweeps the same chords
(a call that also writes prev is measured on its own: "B_write").  Both calls are count + scan + scatter + query; the grids are
chosen once, over the pinned box, and the timed calls go straight to the library.

    python tools/bench_clearance_sweep.py [--drones 65536] [--chord 0.2] [--margin 1.0] [--iters 50] [--warmup 20] [--pairs 9]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--drones", type=int, default=65536)
    ap.add_argument("--chord", type=float, default=0.2)
    ap.add_argument("--margin", type=float, default=1.0)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=9)
    a = ap.parse_args()
    import torch
    from dronesim_amd import fleet, params
    from dronesim_amd.downwash import Downwash
    if not torch.cuda.is_available():
        raise SystemExit("bench_clearance_sweep needs a HIP device")
    t = params.builtin_type("robobee")
    ctx = fleet.Context([t])
    n = a.drones
    width = 128.0 * n / 65536.0                                    # the config's slab: one drone per m^2 of ground
    rng = np.random.default_rng(7)
    pos = np.stack([rng.uniform(0.0, width, n), rng.uniform(0.0, 512.0, n), rng.uniform(0.5, 20.5, n)], 1).astype(np.float32)
    v = rng.normal(size=(n, 3))
    v *= a.chord * (1.0 - 1e-3) / np.linalg.norm(v, axis=1, keepdims=True)
    st = fleet.FleetState(ctx, n, "soa")
    st.set_fields(0, torch.from_numpy(np.ascontiguousarray(pos.T)))
    prev = torch.zeros((3, st.n_pad), dtype=torch.float32, device=ctx.device)
    prev[:, :n] = torch.from_numpy(np.ascontiguousarray((pos - v.astype(np.float32)).T)).to(ctx.device)
    keep = prev.clone()
    box = (0.0, 0.0, width, 512.0)
    point, swept = Downwash(ctx, st), Downwash(ctx, st)
    uns = torch.zeros((1,), dtype=torch.int64, device=ctx.device)
    # one call of each through the class chooses the grids and makes the workspaces; the timed calls go to the library with those
    # arguments and fixed outputs, so that the host's share of a call is a ctypes call and four launches
    import ctypes
    from dronesim_amd import _native as nat
    point.clearance(a.margin, box=box)
    swept.clearance_sweep(a.margin, 0.0, a.chord, prev, keep_prev=True, box=box)
    ga, gb = point._clr_args, swept._clr_args
    lib, h, view = ctx.lib, ctx.handle, st.view()
    outs = {k: (torch.empty((st.n_pad,), dtype=torch.float32, device=ctx.device),
                torch.empty((st.n_pad,), dtype=torch.int32, device=ctx.device)) for k in ("a", "b")}
    out = {k: (c[:n], i[:n]) for k, (c, i) in outs.items()}
    sb = nat.ClearanceSweepArgs(prev.data_ptr(), a.margin, 0.0, a.chord, nat.SWEEP_KEEP_PREV, outs["b"][0].data_ptr(),
                                outs["b"][1].data_ptr(), None, uns.data_ptr())
    sw = nat.ClearanceSweepArgs.from_buffer_copy(sb)
    sw.flags = 0

    def fa():
        nat.check(lib.dsim_clearance(h, ctx.stream_ptr(), n, view, ctypes.byref(ga), None, a.margin, outs["a"][0].data_ptr(),
                                     outs["a"][1].data_ptr(), None))

    def fb():
        nat.check(lib.dsim_clearance_sweep(h, ctx.stream_ptr(), n, view, ctypes.byref(gb), ctypes.byref(sb)))

    def fw():                                                      # (chords of length 0 after the first)
        nat.check(lib.dsim_clearance_sweep(h, ctx.stream_ptr(), n, view, ctypes.byref(gb), ctypes.byref(sw)))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters

    for _ in range(a.warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(a.pairs):
        ta.append(timed(fa))
        tb.append(timed(fb))
    in_reach = [float((out[k][1] >= 0).float().mean().item()) for k in ("a", "b")]
    # results must not differ in kind: the sweep never reports more room than the samples at the step's end
    above = float((out["b"][0] - out["a"][0]).max().item())
    tw = [timed(fw) for _ in range(3)]
    prev.copy_(keep)
    ratio = np.array(tb) / np.array(ta)
    r = lambda x: round(float(x), 2)
    print(json.dumps({"drones": n, "box_m": [r(width), 512.0, 20.0], "chord_m": a.chord, "travel_m": a.chord, "margin": a.margin,
                      "A_cell_m": round(point.cell, 4), "A_cells": [point._box[2], point._box[3]],
                      "B_cell_m": round(swept.cell, 4), "B_cells": [swept._box[2], swept._box[3]],
                      "in_reach_share_A_B": [round(x, 4) for x in in_reach], "unswept": int(uns.item()),
                      "swept_minus_point_clearance_max_m": above,
                      "A_point_us_median": r(np.median(ta)), "A_point_us_min_max": [r(min(ta)), r(max(ta))],
                      "B_sweep_us_median": r(np.median(tb)), "B_sweep_us_min_max": [r(min(tb)), r(max(tb))],
                      "B_over_A_median": round(float(np.median(ratio)), 3),
                      "B_over_A_min_max": [round(float(ratio.min()), 3), round(float(ratio.max()), 3)],
                      "B_write_prev_zero_chord_us_median": r(np.median(tw))}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
