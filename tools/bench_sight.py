"""Times line of sight: N tellos x k = 8 neighbour segments, device events around a batch of queries behind a settled warm-up (the
protocol of tools/bench_scan.py: five repeats, the median), and beside it, on the same fleet, the two yardsticks it is read
against: dsim_range_scan with 8 beams and t_max = 3 m (as many rays per drone, none longer than the knn radius) and the dsim_knn
that writes the record.

The fleet is N / 16 replicas of one task by offsets: 16 drones about the gate at (2, 0, 1) of THEIR task frame — on both sides of
it, so that neighbours are hidden —, stored at that place plus the replica's offset, 12 m apart on a square lattice: every drone
has its replica's 15 others within reach and nobody else.  World "set": the gate scene (tests/camera_ref.scene).  World "scenes":
per-drone scenes, 64 scenes of 3 placements of the gate prototype (tests/scenes_ref.random_placements), replica r in scene r mod 64.
One JSON line per world and fleet size.  --drones: beside them the same query with the other drones hiding too
(dsim_line_of_sight_drones, on the same record and the same device set), the share of it that the per-call binning of the fleet
takes (the same call with every index at -1: it bins and casts nothing) and, for scale, the scanner with drones=True.

    python tools/bench_sight.py [--sizes 65536 1048576] [--k 8] [--radius 3.0] [--subdiv 0] [--iters 200] [--warmup 50] [--lib PATH]
                                [--drones]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, call, a):
    for _ in range(a.warmup):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            call()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / a.iters)
    return float(np.median(times)), [round(t, 2) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=(65536, 1048576))
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--radius", type=float, default=3.0)
    ap.add_argument("--subdiv", type=int, default=0, help="subdivide the gate's 96 triangles this many times (x 4 each; world set)")
    ap.add_argument("--worlds", nargs="+", default=("set", "scenes"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--drones", action="store_true", help="also time the query with the other drones hiding (and its binning)")
    ap.add_argument("--lib", default=None, help="another build of the library (an A/B against the one in the tree)")
    a = ap.parse_args()
    from dronesim_amd import _native as nat
    if a.lib:
        nat.load(a.lib)
    import torch
    from dronesim_amd.downwash import Downwash, Neighbors
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.obstacles import ObstacleScenes
    from dronesim_amd.scanner import RangeScanner
    from dronesim_amd.sight import LineOfSight
    from tests import camera_ref as cr
    from tests import scenes_ref as sr
    K, G, GROUP = 64, 3, 16
    for world in a.worlds:
        for n in a.sizes:
            rng = np.random.default_rng(0)
            task = np.stack([rng.uniform(0.5, 3.5, n), rng.uniform(-1.5, 1.5, n), rng.uniform(0.5, 1.5, n)], 1)
            rep = np.arange(n) // GROUP
            side = int(np.ceil(np.sqrt(rep[-1] + 1)))
            off = np.stack([(rep % side) * 12.0, (rep // side) * 12.0, np.zeros(n)], 1)
            env = CtrlAviary(["tello"], n, initial_xyzs=task + off, noise_seed=0, dict_io=False, ground_plane=False)
            if world == "set":
                w, sid = cr.scene(a.subdiv), None
                n_tri = w.n_tri
            else:
                pos, rpy = sr.random_placements(np.random.default_rng(1), K, G)
                # (the placements of tests/scenes_ref lie about the origin: the replica's drones stand about (2, 0, 1))
                w, sid = ObstacleScenes(sr.gate(), pos + np.array([2.0, 0.0, 0.0]), rpy), (rep % K).astype(np.int64)
                n_tri = w.prototype.n_tri
            los = LineOfSight(env.ctx, env.state, w, a.k, offsets=off, scene_id=sid)
            dev, n_pad = env.ctx.device, env.state.n_pad
            f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
            out = Neighbors(torch.full((a.k, n_pad), -1, dtype=torch.int32, device=dev), f32(a.k, n_pad), f32(a.k, 3, n_pad), None,
                            torch.zeros((n_pad,), dtype=torch.int32, device=dev))
            grid = Downwash(env.ctx, env.state, None, None)
            knn = lambda: grid.nearest(a.radius, a.k, out=out)
            knn()
            scanner = RangeScanner(env.ctx, env.state, los.set, RangeScanner.fan(a.k), t_min=0.0, t_max=a.radius, ground=False, offsets=off,
                                   scene_id=sid)
            t_sight, all_sight = timed(torch, lambda: los.query(out.rel_pos, out.index), a)
            t_scan, all_scan = timed(torch, scanner.scan, a)
            t_knn, all_knn = timed(torch, knn, a)
            s = los.query(out.rel_pos, out.index)
            used = out.index[:, :n] >= 0
            extra = {}
            if a.drones:
                lod = LineOfSight(env.ctx, env.state, los.set, a.k, offsets=off, scene_id=sid, drones=True)
                scan_d = RangeScanner(env.ctx, env.state, los.set, RangeScanner.fan(a.k), t_min=0.0, t_max=a.radius, ground=False,
                                      offsets=off, scene_id=sid, drones=True)
                nobody = torch.full_like(out.index, -1)
                t_d, all_d = timed(torch, lambda: lod.query(out.rel_pos, out.index), a)
                t_bin, all_bin = timed(torch, lambda: lod.query(out.rel_pos, nobody), a)
                t_sd, all_sd = timed(torch, scan_d.scan, a)
                sd_ = lod.query(out.rel_pos, out.index)
                extra = {"us_per_sight_drones_median": round(t_d, 2), "us_per_sight_drones_all": all_d,
                         "us_per_binning_median": round(t_bin, 2), "us_per_binning_all": all_bin,
                         "binning_share_of_sight_drones": round(t_bin / t_d, 4), "sight_drones_over_sight": round(t_d / t_sight, 4),
                         "us_per_scan_drones_median": round(t_sd, 2), "us_per_scan_drones_all": all_sd,
                         "blocked_by_drones_share_of_used": round(float(((sd_.blocker <= -3) & used).sum().item()) / max(float(used.sum().item()), 1.0), 4),
                         "drones_outside": lod.drones_outside()}
                scan_d.close()
                lod.close()
            print(json.dumps({**extra, "world": world, "drones": n, "k": a.k, "radius": a.radius, "n_tri": int(n_tri),
                              "us_per_sight_median": round(t_sight, 2), "us_per_sight_all": all_sight,
                              "us_per_scan_median": round(t_scan, 2), "us_per_scan_all": all_scan,
                              "us_per_knn_median": round(t_knn, 2), "us_per_knn_all": all_knn,
                              "sight_share_of_knn_plus_sight": round(t_sight / (t_sight + t_knn), 4),
                              "sight_over_scan": round(t_sight / t_scan, 4),
                              "segments_per_s": round(float(used.sum().item()) / (t_sight * 1e-6), 0),
                              "used_share": round(float(used.float().mean().item()), 4),
                              "blocked_share_of_used": round(float(((s.visible == 0) & used).sum().item()) / max(float(used.sum().item()), 1.0), 4),
                              "scan_hit_share": round(float((scanner.hits >= 0).float().mean().item()), 4)}))
            scanner.close()
            los.close()
            env.close()


if __name__ == "__main__":
    main()
