"""Times corridor clearance: N tellos x k candidate segments (a fan of `length` metres about the forward direction), beside the two
queries it is read against on the same fleet, world and device set: dsim_line_of_sight on the same rel rows (the same segments,
with no thickness) and dsim_obstacle_sweep (one chord per drone, of one slot's length: the same arithmetic, one slot).  Interleaved
pairs: every repeat times corridor, sight and sweep in turn on device events around a batch of calls behind a settled warm-up, and
the median over the repeats is reported with every single figure beside it.

The fleet is N / 16 replicas of one task by offsets: 16 drones about the gate at (2, 0, 1) of THEIR task frame, stored at that place
plus the replica's offset (tools/bench_sight.py).  World "set": the gate scene (tests/camera_ref.scene).  World "scenes": per-drone
scenes, 64 scenes of 3 placements of the gate prototype, replica r in scene r mod 64.  World "soup": the 3000-triangle soup of the
tests (records through L2), the drones spread over its box.  One JSON line per world, fleet size and k.

    python tools/bench_corridor.py [--sizes 65536] [--ks 8 16] [--length 1.5] [--piece 0.5] [--worlds set scenes soup]
                                   [--iters 100] [--warmup 20] [--repeats 5] [--lib PATH]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fan_directions(k, spread=np.radians(60.0)):
    """k unit directions about +x: +x itself, then pairs yawed and pitched by growing angles up to ``spread``."""
    out = [np.array([1.0, 0.0, 0.0])]
    rings = max((k - 1 + 3) // 4, 1)
    for j in range(k - 1):
        ang = spread * (j // 4 + 1) / rings
        c, sn = np.cos(ang), np.sin(ang) * (1.0 if j % 2 == 0 else -1.0)
        out.append(np.array([c, sn, 0.0]) if (j // 2) % 2 == 0 else np.array([c, 0.0, sn]))
    return np.stack(out)


def interleaved(torch, calls, a):
    """{name: (median us per call, every repeat's figure)}: per repeat every call is timed once, in turn."""
    for _ in range(a.warmup):
        for c in calls.values():
            c()
    torch.cuda.synchronize()
    times = {name: [] for name in calls}
    for _ in range(a.repeats):
        for name, c in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                c()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / a.iters)
    return {name: (float(np.median(t)), [round(x, 2) for x in t]) for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=(65536,))
    ap.add_argument("--ks", type=int, nargs="+", default=(8, 16))
    ap.add_argument("--length", type=float, default=1.5, help="the length of every candidate segment [m]")
    ap.add_argument("--piece", type=float, default=0.5, help="what one cell lookup serves [m]")
    ap.add_argument("--margin", type=float, default=0.5)
    ap.add_argument("--worlds", nargs="+", default=("set", "scenes", "soup"))
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--lib", default=None, help="another build of the library (an A/B against the one in the tree)")
    a = ap.parse_args()
    from dronesim_amd import _native as nat
    if a.lib:
        nat.load(a.lib)
    import torch
    from dronesim_amd import obstacles as obs
    from dronesim_amd.corridor import Corridor
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.sight import LineOfSight
    from tests import camera_ref as cr
    from tests import scenes_ref as sr
    K, G, GROUP = 64, 3, 16
    for world in a.worlds:
        for n in a.sizes:
            rng = np.random.default_rng(0)
            rep = np.arange(n) // GROUP
            side = int(np.ceil(np.sqrt(rep[-1] + 1)))
            off = np.stack([(rep % side) * 12.0, (rep // side) * 12.0, np.zeros(n)], 1)
            sid = None
            if world == "soup":
                from tests.test_gpu_obstacles import soup
                w = soup()
                task = rng.uniform(-9.0, 9.0, (n, 3))
            else:
                task = np.stack([rng.uniform(0.5, 3.5, n), rng.uniform(-1.5, 1.5, n), rng.uniform(0.5, 1.5, n)], 1)
                if world == "set":
                    w = cr.scene(0)
                else:
                    pos, rpy = sr.random_placements(np.random.default_rng(1), K, G)
                    w, sid = obs.ObstacleScenes(sr.gate(), pos + np.array([2.0, 0.0, 0.0]), rpy), (rep % K).astype(np.int64)
            n_tri = w.prototype.n_tri if sid is not None else w.n_tri
            env = CtrlAviary(["tello"], n, initial_xyzs=task + off, noise_seed=0, dict_io=False, ground_plane=False)
            ctx, st = env.ctx, env.state
            dev = w.to_device(ctx, obs.corridor_reach(ctx.types, a.margin, 0.0, a.piece))
            dev.enable_rays()
            n_pad = st.n_pad
            # the swept watch beside it (sets only: it does not serve scenes): one chord per drone, prev = p - (length, 0, 0)
            sweep = None
            if sid is None:
                d_off = torch.from_numpy(np.ascontiguousarray(off.T)).float().to(ctx.device)
                d_off = torch.nn.functional.pad(d_off, (0, n_pad - n))
                prev = torch.zeros((3, n_pad), dtype=torch.float32, device=ctx.device)
                prev[:, :n] = st.pos                                 # [3, n]: one type, so the caller's numbering is the storage order
                prev[0] -= a.length
                s_clr = torch.empty((n_pad,), dtype=torch.float32, device=ctx.device)
                s_near = torch.empty((n_pad,), dtype=torch.int32, device=ctx.device)
                sweep = lambda: obs.sweep(ctx, st, dev, a.margin, 0.0, prev, s_clr, s_near, d_off, keep_prev=True)
            for k in a.ks:
                cor = Corridor(ctx, st, dev, k, a.margin, offsets=off, scene_id=sid)
                los = LineOfSight(ctx, st, dev, k, offsets=off, scene_id=sid)
                rel = cor.fan(fan_directions(k), a.length)
                calls = {"corridor": lambda: cor.query(rel), "sight": lambda: los.query(rel)}
                if sweep is not None:
                    calls["sweep"] = sweep
                t = interleaved(torch, calls, a)
                out = cor.query(rel)
                torch.cuda.synchronize()
                c = out.clearance
                line = {"world": world, "drones": n, "k": k, "length": a.length, "piece": a.piece, "margin": a.margin, "n_tri": int(n_tri),
                        "pieces_per_segment": int(np.ceil(a.length / (2.0 * cor.half * (1.0 - 2.0 ** -10)))),
                        "us_per_corridor_median": round(t["corridor"][0], 2), "us_per_corridor_all": t["corridor"][1],
                        "us_per_sight_median": round(t["sight"][0], 2), "us_per_sight_all": t["sight"][1],
                        "corridor_over_sight": round(t["corridor"][0] / t["sight"][0], 3),
                        "segments_per_s": round(k * n / (t["corridor"][0] * 1e-6), 0),
                        "within_margin_share": round(float((c < a.margin).float().mean().item()), 4),
                        "blocked_share": round(float((c < 0).float().mean().item()), 4), "unserved": cor.unserved()}
                if sweep is not None:
                    line.update({"us_per_sweep_median": round(t["sweep"][0], 2), "us_per_sweep_all": t["sweep"][1],
                                 "corridor_per_slot_over_sweep": round(t["corridor"][0] / k / t["sweep"][0], 3)})
                print(json.dumps(line), flush=True)
                los.close()
                cor.close()
            dev.close()
            env.close()


if __name__ == "__main__":
    main()
