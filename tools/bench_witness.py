"""Times the obstacle witness against the point watch it replaces, on the same fleet, set and margin (the protocol and the shapes of
tools/bench_scenes.py).

Unplaced: A = dsim_obstacle_clearance on the gate, B = dsim_obstacle_witness (world axes, no triangle_out), C = the same in the
body frame.  Placed: A = dsim_obstacle_clearance_scenes with G = 3 (64 scenes of three random gates, scene_id = i mod 64), B and C
as above through dsim_obstacle_witness_scenes.  N robobees, "far" (the fleet stands 100 m away: nobody is in reach) and "near" (the
fleet about the gates: about a quarter in reach).  Device events around batches of --iters calls behind a warm-up, the variants
interleaved round by round; prints one JSON line per case with the median and the range of each and of the paired ratios.

    python tools/bench_witness.py [--drones 65536 4194304] [--iters 50] [--warmup 20] [--pairs 9] [--lib PATH]

The bytes a far drone must move: the point watch reads 12 (position) and writes 8; the witness writes 12 more (rel = 0).  A drone in
reach reads one 64-byte record again (from LDS, or through L2) and, in the body frame, its quaternion (16).

Moving ("moving_G3"): the same 64 scenes under a motion of every term (dsim_scenes_motion_set), the clock at 7.  D = dsim_scenes_move
+ dsim_obstacle_witness_scenes, what an env with obstacle_motion and obstacle_witness launches behind a step; E =
dsim_scenes_move_twist + dsim_obstacle_witness_scenes_vel, the same with obstacle_witness_velocity; F and G the two moves alone.
E costs 32 bytes written per moving slot, and 32 read and 12 written per drone in reach (12 written per far drone: vel = 0).  A
build without the twist entries (an older library's tree) prints D and F only: run the tool from both trees in alternation for
an A/B against it.
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
    ap.add_argument("--margin", type=float, default=0.5)
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
        raise SystemExit("bench_witness needs a HIP device")
    ctx = fleet.Context([params.builtin_type("robobee")])
    gate = obs.ObstacleSet.from_urdf(os.path.join(ROOT, "tests", "golden", "gate_50_curved.urdf"), (0, 0, 0), (0, 0, 0))
    K = 64
    rng = np.random.default_rng(11)
    pos3 = rng.uniform([-2.0, -2.0, 1.0], [2.0, 2.0, 3.0], (K, 3, 3))
    rpy3 = rng.uniform([-0.5, -0.5, -np.pi], [0.5, 0.5, np.pi], (K, 3, 3))
    dev = gate.to_device(ctx, obs.watch_reach(ctx.types, a.margin))
    three = obs.ObstacleScenes(gate, pos3, rpy3).to_device(ctx, prototype_dev=dev)
    # the same scenes twice more, moving: one moved plainly, one with its twist table (where the build has one)
    mrng = np.random.default_rng(13)
    axis = mrng.normal(size=(K, 3, 3))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    scenes_m = obs.ObstacleScenes(gate, pos3, rpy3)
    motion = obs.SceneMotion(scenes_m, velocity=mrng.uniform(-1.5, 1.5, (K, 3, 3)), amplitude=mrng.uniform(-0.4, 0.4, (K, 3, 3)),
                             omega=mrng.uniform(3.0, 6.0, (K, 3)), phase=mrng.uniform(-1.0, 1.0, (K, 3)), axis=axis,
                             rate=mrng.uniform(2.0, 4.0, (K, 3)), swing=mrng.uniform(0.3, 0.9, (K, 3)))
    moved = scenes_m.to_device(ctx, prototype_dev=dev).set_motion(motion)
    has_twist = hasattr(obs.DeviceScenes, "enable_twist")
    twisted = scenes_m.to_device(ctx, prototype_dev=dev).enable_twist().set_motion(motion) if has_twist else None
    clock = torch.full((1,), 7, dtype=torch.int64, device=ctx.device)
    dt = 1.0 / 48.0
    r = lambda x: round(float(x), 2)

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

    for n in a.drones:
        for case in ("far", "near"):
            rg = np.random.default_rng(7)
            p = pos3[np.arange(n) % K, rg.integers(0, 3, n)] + rg.uniform(-1.5, 1.5, (n, 3))
            p[::4] = rg.uniform(-0.6, 0.6, (len(p[::4]), 3))
            if case == "far":
                p[:, 0] += 100.0
            st = fleet.FleetState(ctx, n, "soa")
            state = np.zeros((7, n), dtype=np.float32)
            state[:3] = p.astype(np.float32).T
            quat = rg.normal(size=(4, n))
            state[3:7] = (quat / np.linalg.norm(quat, axis=0)).astype(np.float32)
            st.set_fields(0, torch.from_numpy(state))
            clr = torch.empty((st.n_pad,), dtype=torch.float32, device=ctx.device)
            near = torch.empty((st.n_pad,), dtype=torch.int32, device=ctx.device)
            rel = torch.empty((3, st.n_pad), dtype=torch.float32, device=ctx.device)
            id3 = (torch.arange(st.n_pad, dtype=torch.int32) % K).to(ctx.device)
            for what, fns in (("unplaced", [lambda: obs.query(ctx, st, dev, a.margin, clr, near),
                                            lambda: obs.witness(ctx, st, dev, a.margin, clr, near, rel),
                                            lambda: obs.witness(ctx, st, dev, a.margin, clr, near, rel, body_frame=True)]),
                              ("placed_G3", [lambda: obs.query_scenes(ctx, st, three, id3, a.margin, clr, near),
                                             lambda: obs.witness_scenes(ctx, st, three, id3, a.margin, clr, near, rel),
                                             lambda: obs.witness_scenes(ctx, st, three, id3, a.margin, clr, near, rel, body_frame=True)])):
                t = rounds(fns)
                fns[0]()
                share = round(float((near[:n] >= 0).float().mean().item()), 4)
                report({"what": what, "case": case, "drones": n, "n_tri": gate.n_tri, "margin": a.margin, "in_reach_share": share,
                        "far_bytes_per_drone_A_B": [20, 32] if what == "unplaced" else [72, 84]},
                       ["A_point", "B_witness", "C_witness_body"], t)
            vel = torch.empty((3, st.n_pad), dtype=torch.float32, device=ctx.device)

            def plain_pair():
                moved.move(clock, dt)
                obs.witness_scenes(ctx, st, moved, id3, a.margin, clr, near, rel)

            def twist_pair():
                twisted.move(clock, dt)
                obs.witness_scenes_vel(ctx, st, twisted, id3, a.margin, clr, near, rel, vel)
            fns, names = [plain_pair, lambda: moved.move(clock, dt)], ["D_move_witness", "F_move"]
            if has_twist:
                fns, names = fns + [twist_pair, lambda: twisted.move(clock, dt)], names + ["E_movetwist_witnessvel", "G_move_twist"]
            t = rounds(fns)
            plain_pair()
            share = round(float((near[:n] >= 0).float().mean().item()), 4)
            report({"what": "moving_G3", "case": case, "drones": n, "n_tri": gate.n_tri, "margin": a.margin, "in_reach_share": share,
                    "moving_slots": int(motion.moving.sum())}, names, t)
            del st, clr, near, rel, vel, id3
    moved.close()
    if twisted is not None:
        twisted.close()
    three.close()
    dev.close()
    ctx.close()


if __name__ == "__main__":
    main()
