"""Times the obstacle witnesses (m = 1, 2, 4, 8) against the single witness on the same inputs (the protocol of tools/bench_witness.py).

Four worlds, so that every instance runs: "set_lds" the gate and four boxes (144 triangles, 5 bodies: records staged in LDS) through
dsim_obstacle_witness / dsim_obstacle_witnesses; "set_l2" a soup of 3 000 triangles in four bodies (records through L2);
"scenes_lds" 64 scenes of three random placements of the 5-body set through dsim_obstacle_witness_scenes /
dsim_obstacle_witnesses_scenes; "scenes_l2" 4 scenes of two placements of the soup.  N robobees about the world (hexa_6DOF on the
soup), "far" (the fleet stands 100 m away: nobody is in reach) and "near".  A = the witness (world axes, no triangle_out), M1, M2, M4,
M8 = the witnesses with that m (no triangle_out, with count_out): capacity 4 serves m <= 4, capacity 8 the rest.  Device events
around batches of --iters calls behind a warm-up, the variants interleaved round by round; one JSON line per case with the median
and the range of each and of the paired ratios to A.

    python tools/bench_witnesses.py [--drones 65536 1048576] [--iters 50] [--warmup 20] [--pairs 9] [--lib PATH]

Bytes written per drone, whatever it sees: the witness 20 (clearance, nearest, rel); the witnesses 20 m + 4 (count), slot-major, so
every store of a wave is contiguous.  A drone in reach reads one 64-byte record again per filled slot.
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
    if not torch.cuda.is_available():
        raise SystemExit("bench_witnesses needs a HIP device")
    r = lambda x: round(float(x), 2)
    rng = np.random.default_rng(11)
    five = obs.ObstacleSet.from_urdf(os.path.join(ROOT, "tests", "golden", "gate_50_curved.urdf"), (0, 0, 0), (0, 0, 0))
    for c, size in (((0.3, -0.7, 0.5), (0.2, 0.3, 0.25)), ((-0.3, 0.75, -0.45), (0.25, 0.2, 0.3)), ((0.35, 0.6, 0.55), (0.15, 0.35, 0.2)),
                    ((-0.35, -0.65, -0.5), (0.3, 0.15, 0.2))):
        five = five + obs.ObstacleSet.box(c, size)
    srng = np.random.default_rng(2024)
    soup = obs.ObstacleSet(srng.uniform(-9.2, 9.2, (3000, 1, 3)) + srng.uniform(-0.75, 0.75, (3000, 3, 3)), np.arange(3000) // 750)

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

    def report(head, names, t):
        out = dict(head)
        for nm, x in zip(names, t):
            out[nm + "_us_median"], out[nm + "_us_min_max"] = r(np.median(x)), [r(x.min()), r(x.max())]
        for nm, x in zip(names[1:], t[1:]):
            q = x / t[0]
            out[nm + "_over_" + names[0] + "_median"] = round(float(np.median(q)), 3)
            out[nm + "_over_" + names[0] + "_min_max"] = [round(float(q.min()), 3), round(float(q.max()), 3)]
        print(json.dumps(out), flush=True)

    for world, proto, model, margin, K, G, spread in (("set_lds", five, "robobee", 1.0, 0, 0, 1.0), ("set_l2", soup, "hexa_6DOF", 0.6, 0, 0, 10.0),
                                                      ("scenes_lds", five, "robobee", 1.0, 64, 3, 1.5),
                                                      ("scenes_l2", soup, "hexa_6DOF", 0.6, 4, 2, 10.0)):
        ctx = fleet.Context([params.builtin_type(model)])
        dev = proto.to_device(ctx, obs.watch_reach(ctx.types, margin))
        placed = None
        if K:
            ppos = rng.uniform([-2.0, -2.0, 1.0], [2.0, 2.0, 3.0], (K, G, 3))
            prpy = rng.uniform([-0.5, -0.5, -np.pi], [0.5, 0.5, np.pi], (K, G, 3))
            placed = obs.ObstacleScenes(proto, ppos, prpy).to_device(ctx, prototype_dev=dev)
        for n in a.drones:
            for case in ("far", "near"):
                rg = np.random.default_rng(7)
                p = rg.uniform(-spread, spread, (n, 3))
                if K:
                    p += ppos[np.arange(n) % K, rg.integers(0, G, n)]
                if case == "far":
                    p[:, 0] += 100.0
                st = fleet.FleetState(ctx, n, "soa")
                state = np.zeros((7, n), dtype=np.float32)
                state[:3] = p.astype(np.float32).T
                state[6] = 1.0
                st.set_fields(0, torch.from_numpy(state))
                new = lambda shape, dt: torch.empty(shape, dtype=dt, device=ctx.device)
                clr, near, rel = new((8, st.n_pad), torch.float32), new((8, st.n_pad), torch.int32), new((8, 3, st.n_pad), torch.float32)
                cnt = new((st.n_pad,), torch.int32)
                ids = (torch.arange(st.n_pad, dtype=torch.int32) % max(K, 1)).to(ctx.device)
                c1, n1, r1 = clr[0], near[0], rel[0]                 # (sliced once: the timed calls do no tensor work)
                if K:
                    one = lambda: obs.witness_scenes(ctx, st, placed, ids, margin, c1, n1, r1)
                    many = lambda m: (lambda: obs.witnesses_scenes(ctx, st, placed, ids, margin, m, clr, near, rel, None, cnt))
                else:
                    one = lambda: obs.witness(ctx, st, dev, margin, c1, n1, r1)
                    many = lambda m: (lambda: obs.witnesses(ctx, st, dev, margin, m, clr, near, rel, None, cnt))
                fns = [one] + [many(m) for m in (1, 2, 4, 8)]
                t = rounds(fns)
                fns[-1]()
                filled = [round(float((near[s, :n] >= 0).float().mean().item()), 4) for s in range(8)]
                report({"what": world, "case": case, "drones": n, "n_tri": proto.n_tri, "n_bodies": proto.n_bodies * max(G, 1),
                        "margin": margin, "filled_share_per_slot": filled,
                        "bytes_written_per_drone": {"A": 20, "M1": 24, "M2": 44, "M4": 84, "M8": 164}},
                       ["A_witness", "M1", "M2", "M4", "M8"], t)
                del st, clr, near, rel, cnt, ids, c1, n1, r1
        if placed is not None:
            placed.close()
        dev.close()
        ctx.close()


if __name__ == "__main__":
    main()
