"""Times the swept obstacle watch against the point watch it stands beside: A = dsim_obstacle_clearance, B = dsim_obstacle_sweep,
the same device set, fleet and margin.  N robobees on the gate scene, "far" (every wave rejects: the fleet stands 100 m away from
the gate) and "near" (the fleet inside the grown box), chords of --chord metres.  Device events around batches of --iters calls
behind a warm-up, A and B interleaved in pairs; prints one JSON line per case with the median and the spread of both and of the
paired ratio.  B runs with KEEP_PREV, so every call sweeps the same chords (the writes of prev are measured on their own: "B_write").

    python tools/bench_sweep.py [--drones 65536 4194304] [--chord 0.1] [--iters 50] [--warmup 20] [--pairs 9] [--lib PATH]

The bytes a call must move, per drone: A reads 3 floats and writes 2 (clearance, nearest); B reads 6 (position, prev) and writes 2,
and 3 more without KEEP_PREV.
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
    ap.add_argument("--drones", type=int, nargs="+", default=[65536, 4194304])
    ap.add_argument("--chord", type=float, default=0.1)
    ap.add_argument("--margin", type=float, default=1.0)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--lib", default=None, help="another build of the library (an A/B against the one in the tree)")
    a = ap.parse_args()
    import torch
    from dronesim_amd import _native as nat
    if a.lib:
        nat.load(a.lib)
    from dronesim_amd import fleet, params
    from dronesim_amd import obstacles as obs
    if not torch.cuda.is_available():
        raise SystemExit("bench_sweep needs a HIP device")
    t = params.builtin_type("robobee")
    ctx = fleet.Context([t])
    gate = obs.ObstacleSet.from_urdf(os.path.join(ROOT, "tests", "golden", "gate_50_curved.urdf"), (0, 0, 0), (0, 0, 0))
    dev = gate.to_device(ctx, obs.sweep_reach(ctx.types, a.margin, 0.0, a.chord))
    g, _, _ = gate.grid(dev.reach)
    lo, hi = np.array(list(g.lo), dtype=np.float64), np.array(list(g.hi), dtype=np.float64)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters

    for n in a.drones:
        for case in ("far", "near"):
            rng = np.random.default_rng(7)
            mid = rng.uniform(lo + a.chord, hi - a.chord, (n, 3)).astype(np.float32)
            if case == "far":
                mid[:, 0] += 100.0
            v = rng.normal(size=(n, 3)).astype(np.float32)
            v *= 0.5 * a.chord / np.linalg.norm(v, axis=1, keepdims=True)
            st = fleet.FleetState(ctx, n, "soa")
            st.set_fields(0, torch.from_numpy(np.ascontiguousarray((mid + v).T)))
            prev = torch.zeros((3, st.n_pad), dtype=torch.float32, device=ctx.device)
            prev[:, :n] = torch.from_numpy(np.ascontiguousarray((mid - v).T)).to(ctx.device)
            clr = torch.empty((st.n_pad,), dtype=torch.float32, device=ctx.device)
            near = torch.empty((st.n_pad,), dtype=torch.int32, device=ctx.device)
            uns = torch.zeros((1,), dtype=torch.int64, device=ctx.device)
            keep = prev.clone()
            fa = lambda: obs.query(ctx, st, dev, a.margin, clr, near)
            fb = lambda: obs.sweep(ctx, st, dev, a.margin, 0.0, prev, clr, near, unswept_out=uns, keep_prev=True)
            fw = lambda: obs.sweep(ctx, st, dev, a.margin, 0.0, prev, clr, near, unswept_out=uns)      # (chords of length 0 after the first)
            for _ in range(a.warmup):
                fa()
                fb()
            torch.cuda.synchronize()
            ta, tb = [], []
            for _ in range(a.pairs):
                ta.append(timed(fa))
                tb.append(timed(fb))
            in_reach = float((near[:n] >= 0).float().mean().item())
            tw = [timed(fw) for _ in range(3)]
            prev.copy_(keep)
            ratio = np.array(tb) / np.array(ta)
            r = lambda x: round(float(x), 2)
            print(json.dumps({"case": case, "drones": n, "n_tri": gate.n_tri, "chord_m": a.chord, "margin": a.margin, "reach": r(dev.reach),
                              "in_reach_share": round(in_reach, 4), "unswept": int(uns.item()),
                              "A_point_us_median": r(np.median(ta)), "A_point_us_min_max": [r(min(ta)), r(max(ta))],
                              "B_sweep_us_median": r(np.median(tb)), "B_sweep_us_min_max": [r(min(tb)), r(max(tb))],
                              "B_over_A_median": round(float(np.median(ratio)), 3),
                              "B_over_A_min_max": [round(float(ratio.min()), 3), round(float(ratio.max()), 3)],
                              "B_write_prev_zero_chord_us_median": r(np.median(tw)),
                              "A_bytes_per_drone": 20, "B_bytes_per_drone": 32,
                              "A_GBps": r(20 * n / np.median(ta) * 1e-3), "B_GBps": r(32 * n / np.median(tb) * 1e-3)}), flush=True)
            del st, prev, clr, near, keep
    dev.close()
    ctx.close()


if __name__ == "__main__":
    main()
