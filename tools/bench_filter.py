"""Times the velocity safety filter beside the two launches whose records it consumes (the protocol of tools/bench_witnesses.py).

One world: 64 scenes of three random placements of the gate and four boxes (144 triangles, 5 bodies) through
dsim_obstacle_witnesses_scenes with m = 3, and N robobees about them in one frame — a crowd, so that dsim_knn with k = 6 within
1.5 m finds neighbours.  K = dsim_knn, W = the witnesses, F = dsim_velocity_filter on the records the two just wrote (alpha 2,
buffers 0.05 / 0.1, the floor at 0), F0 = the filter on a wished velocity of zero (almost nobody violates a row: every record is
read once and nothing is solved).  Device events around batches of --iters calls behind a warm-up, the variants interleaved round
by round; one JSON line per fleet size with the median and the range of each and of the paired ratios to K, and what the filter did.

    python tools/bench_filter.py [--drones 65536 1048576] [--iters 50] [--warmup 20] [--pairs 9] [--lib PATH]

Bytes per drone of F: 32 per neighbour slot (index, dist, rel_pos, rel_vel), 20 per obstacle slot (32 with the witnesses'
velocities), 40 of its own (position, velocity, u, the offset's z), 16 written (v, dropped): 308 at k = 6, m = 3.  A violated row
reads the records of the rows kept before it again, from cache.
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
    ap.add_argument("--drones", type=int, nargs="+", default=[65536, 1048576])
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
    from dronesim_amd.avoid import Filtered, VelocityFilter
    from dronesim_amd.downwash import Downwash, Neighbors
    if not torch.cuda.is_available():
        raise SystemExit("bench_filter needs a HIP device")
    r = lambda x: round(float(x), 2)
    rng = np.random.default_rng(11)
    five = obs.ObstacleSet.from_urdf(os.path.join(ROOT, "tests", "golden", "gate_50_curved.urdf"), (0, 0, 0), (0, 0, 0))
    for c, size in (((0.3, -0.7, 0.5), (0.2, 0.3, 0.25)), ((-0.3, 0.75, -0.45), (0.25, 0.2, 0.3)), ((0.35, 0.6, 0.55), (0.15, 0.35, 0.2)),
                    ((-0.35, -0.65, -0.5), (0.3, 0.15, 0.2))):
        five = five + obs.ObstacleSet.box(c, size)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters

    def rounds(fns):
        for _ in range(a.warmup):
            for f in fns:
                f()
        torch.cuda.synchronize()
        t = [[] for _ in fns]
        for _ in range(a.pairs):
            for k, f in enumerate(fns):
                t[k].append(timed(f))
        return [np.array(x) for x in t]

    K, G, k, m, margin, radius = 64, 3, 6, 3, 1.0, 1.5
    ctx = fleet.Context([params.builtin_type("robobee")])
    dev = five.to_device(ctx, obs.watch_reach(ctx.types, margin))
    ppos = rng.uniform([-2.0, -2.0, 1.0], [2.0, 2.0, 3.0], (K, G, 3))
    prpy = rng.uniform([-0.5, -0.5, -np.pi], [0.5, 0.5, np.pi], (K, G, 3))
    placed = obs.ObstacleScenes(five, ppos, prpy).to_device(ctx, prototype_dev=dev)
    for n in a.drones:
        rg = np.random.default_rng(7)
        # a crowd of constant density: about two drones per cubic metre around the gates, the box growing with the fleet
        side = max(4.0, (n / 8.0) ** 0.5)
        p = np.stack([rg.uniform(-side / 2, side / 2, n), rg.uniform(-side / 2, side / 2, n), rg.uniform(0.5, 4.5, n)], 1)
        st = fleet.FleetState(ctx, n, "soa")
        state = np.zeros((10, n), dtype=np.float32)
        state[:3] = p.astype(np.float32).T
        state[6] = 1.0
        state[7:10] = rg.normal(size=(3, n)).astype(np.float32) * 0.5
        st.set_fields(0, torch.from_numpy(state))
        new = lambda shape, dt: torch.zeros(shape, dtype=dt, device=ctx.device)
        n_pad = st.n_pad
        wit = obs.ObstacleWitnesses(new((m, n_pad), torch.float32), new((m, n_pad), torch.int32), new((m, 3, n_pad), torch.float32), None,
                                    new((n_pad,), torch.int32))
        nb = Neighbors(new((k, n_pad), torch.int32), new((k, n_pad), torch.float32), new((k, 3, n_pad), torch.float32),
                       new((k, 3, n_pad), torch.float32), new((n_pad,), torch.int32))
        ids = (torch.arange(n_pad, dtype=torch.int32) % K).to(ctx.device)
        u = torch.from_numpy((rg.normal(size=(3, n_pad)) * 1.5 / np.sqrt(3.0)).astype(np.float32)).to(ctx.device)
        u0 = torch.zeros_like(u)
        dw = Downwash(ctx, st)
        box = (-side / 2, -side / 2, side / 2, side / 2)
        f, f0 = (VelocityFilter(ctx, st, 2.0, 0.05, 0.1, 0.5, floor=0.0) for _ in range(2))
        out = Filtered(new((3, n_pad), torch.float32), new((n_pad,), torch.int32))
        fns = [lambda: dw.nearest(radius, k, out=nb, box=box),
               lambda: obs.witnesses_scenes(ctx, st, placed, ids, margin, m, wit.clearance, wit.body, wit.rel, None, wit.count),
               lambda: f.apply(u, nb, wit, out=out), lambda: f0.apply(u0, nb, wit, out=out)]
        for fn in fns[:2]:
            fn()
        t = rounds(fns)
        torch.cuda.synchronize()
        f2 = VelocityFilter(ctx, st, 2.0, 0.05, 0.1, 0.5, floor=0.0)
        f2.apply(u, nb, wit, out=out)
        changed, lost = f2.counters()
        res = {"what": "filter", "drones": n, "k": k, "m": m, "neighbour_slots_filled": round(float((nb.index[:, :n] >= 0).float().mean().item()), 4),
               "obstacle_slots_filled": round(float((wit.body[:, :n] >= 0).float().mean().item()), 4),
               "changed_share": round(changed / n, 4), "dropped_share": round(lost / n, 4), "bytes_per_drone": 32 * k + 20 * m + 56}
        for nm, x in zip(("K_knn", "W_witnesses", "F_filter", "F0_filter_idle"), t):
            res[nm + "_us_median"], res[nm + "_us_min_max"] = r(np.median(x)), [r(x.min()), r(x.max())]
        for nm, x in zip(("W_witnesses", "F_filter", "F0_filter_idle"), t[1:]):
            q = x / t[0]
            res[nm + "_over_K_median"] = round(float(np.median(q)), 3)
            res[nm + "_over_K_min_max"] = [round(float(q.min()), 3), round(float(q.max()), 3)]
        res["F_GBps_median"] = r((32 * k + 20 * m + 56) * n / np.median(t[2]) / 1e3)
        print(json.dumps(res), flush=True)
        del st, nb, wit, u, u0, out, dw, f, f0, f2
    placed.close()
    dev.close()
    ctx.close()


if __name__ == "__main__":
    main()
