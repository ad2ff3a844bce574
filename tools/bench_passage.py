"""Times the gate passage watch against the placed clearance watch on the same scenes, fleet and box.

A = dsim_obstacle_clearance_scenes, B = dsim_gate_passage, both with G = 3 placements of the gate per scene and scene_id = i mod K.
K = 64 (the table of tools/bench_scenes.py: it stays in cache) and K = 2^20 (as good as a scene per drone: K G <= 2^22 is the
library's limit, so 4 194 304 drones share 1 048 576 scenes; every lane reads slot heads of its own).  "far": the fleet stands 100 m
from every placement, every slot is culled; "near": the fleet about its gates, chords of 0.5 m aimed like the tests'.  Device events
around batches of --iters calls behind a warm-up, the two interleaved round by round (tools/bench_camera.py's protocol); one JSON
line per case.  The passage watch runs with KEEP_PREV so that every call sees the same chords.

    python tools/bench_passage.py [--drones 4194304] [--scenes 64 1048576] [--iters 50] [--warmup 20] [--pairs 9]

The bytes a far drone must move: A reads 12 (position) + 4 (id) + 48 (heads) and writes 8; B reads 24 (position, prev) + 4 + 48
and writes 12 (the masks), and 12 more when prev moves on.
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
    ap.add_argument("--drones", type=int, nargs="+", default=[4194304])
    ap.add_argument("--scenes", type=int, nargs="+", default=[64, 1 << 20])
    ap.add_argument("--margin", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--move_prev", action="store_true", help="let prev move on (the per-step form: 12 more bytes written per drone)")
    a = ap.parse_args()
    import torch
    from dronesim_amd import fleet, params
    from dronesim_amd import obstacles as obs
    if not torch.cuda.is_available():
        raise SystemExit("bench_passage needs a HIP device")
    ctx = fleet.Context([params.builtin_type("robobee")])
    gate = obs.ObstacleSet.from_urdf(os.path.join(ROOT, "tests", "golden", "gate_50_curved.urdf"), (0, 0, 0), (0, 0, 0))
    opening = obs.Aperture((0, 0, 0), (1, 0, 0), (0, 1, 0), (0.30, 0.20), "rect", outer=(0.56, 0.40))
    dev = gate.to_device(ctx, obs.watch_reach(ctx.types, a.margin))
    r = lambda x: round(float(x), 2)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters

    for K in a.scenes:
        rng = np.random.default_rng(11)
        pos3 = rng.uniform([-2.0, -2.0, 1.0], [2.0, 2.0, 3.0], (K, 3, 3))
        rpy3 = rng.uniform([-0.5, -0.5, -np.pi], [0.5, 0.5, np.pi], (K, 3, 3))
        scenes = obs.ObstacleScenes(gate, pos3, rpy3)
        three = scenes.to_device(ctx, prototype_dev=dev)
        for n in a.drones:
            for case in ("far", "near"):
                rg = np.random.default_rng(7)
                sid = np.arange(n) % K
                p = pos3[sid, rg.integers(0, 3, n)] + rg.uniform(-0.8, 0.8, (n, 3))
                d = rg.normal(size=(n, 3))
                p0 = p - 0.5 * d / np.linalg.norm(d, axis=1, keepdims=True)
                if case == "far":
                    p[:, 0] += 100.0
                    p0[:, 0] += 100.0
                st = fleet.FleetState(ctx, n, "soa")
                st.set_fields(0, torch.from_numpy(np.ascontiguousarray(p.astype(np.float32).T)))
                dv, n_pad = ctx.device, st.n_pad
                clr = torch.empty((n_pad,), dtype=torch.float32, device=dv)
                near = torch.empty((n_pad,), dtype=torch.int32, device=dv)
                ids = (torch.arange(n_pad, dtype=torch.int32) % K).to(dv)
                prev = torch.zeros((3, n_pad), dtype=torch.float32, device=dv)
                prev[:, :n] = torch.from_numpy(np.ascontiguousarray(p0.astype(np.float32).T)).to(dv)
                due, laps = (torch.zeros((n_pad,), dtype=torch.int32, device=dv) for _ in range(2))
                fwd, back, miss = (torch.zeros((n_pad,), dtype=torch.int32, device=dv) for _ in range(3))
                cnt = torch.zeros((5,), dtype=torch.int64, device=dv)
                fa = lambda: obs.query_scenes(ctx, st, three, ids, a.margin, clr, near)
                fb = lambda: obs.gate_passage(ctx, st, three, ids, opening, 2.0, prev, due, laps, None, None, fwd, back, miss, None,
                                              cnt[0:1], cnt[1:2], cnt[2:3], cnt[3:4], cnt[4:5], keep_prev=not a.move_prev)
                for _ in range(a.warmup):
                    fa()
                    fb()
                torch.cuda.synchronize()
                ta, tb = [], []
                for _ in range(a.pairs):
                    ta.append(timed(fa))
                    tb.append(timed(fb))
                ta, tb = np.array(ta), np.array(tb)
                fa()
                cnt.zero_()
                fb()
                q = tb / ta
                print(json.dumps({
                    "what": "gate passage vs placed clearance", "case": case, "drones": n, "K": K, "G": 3, "move_prev": a.move_prev,
                    "in_reach_share_A": round(float((near[:n] >= 0).float().mean().item()), 4),
                    "event_share_B": round(float(((fwd[:n] | back[:n] | miss[:n]) != 0).float().mean().item()), 4),
                    "counts_B": cnt.tolist(),
                    "A_clearance_us_median": r(np.median(ta)), "A_clearance_us_min_max": [r(ta.min()), r(ta.max())],
                    "B_passage_us_median": r(np.median(tb)), "B_passage_us_min_max": [r(tb.min()), r(tb.max())],
                    "B_over_A_median": round(float(np.median(q)), 3), "B_over_A_min_max": [round(float(q.min()), 3), round(float(q.max()), 3)],
                    "far_bytes_per_drone_A_B": [72, 100 if a.move_prev else 88]}), flush=True)
                del st, clr, near, ids, prev, due, laps, fwd, back, miss, cnt
        three.close()
    dev.close()
    ctx.close()


if __name__ == "__main__":
    main()
