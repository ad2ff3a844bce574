"""Times dsim_scenes_move, the kernel that rewrites the scenes' placement table in stream order (dsim_scene_motion.hip).

Two tables — K = 65 536 scenes x G = 4 and K = 1 048 576 x G = 1 (a scene per drone) — each with every slot moving and with one
slot in eight moving (the others static: a lane reads the 16 bytes that hold its flag and stops).  Every moving slot has the whole
law on (velocity, oscillation, spin and swing).  Device events around batches of --iters calls behind a warm-up, the cases
interleaved round by round (tools/bench_camera.py's protocol); one JSON line per case, the float4-copy rate of the same box
(tools/membench) beside it.

    python tools/bench_motion.py [--iters 200] [--warmup 50] [--rounds 7] [--lib PATH] [--twist]

The bytes a slot must move: a moving one reads 64 (motion record) + 48 (base pose) and writes 64 = 176; a static one reads 16.
With --twist the call is dsim_scenes_move_twist, which writes 32 more per moving slot (its twist): 208.
Each case is timed at clock 7 and at clock 2^33: the bytes are the same, but at 2^33 the phase is ~1e9 rad and the fp64 sin/cos
take their large-argument reduction.  Equal times say the bytes bound the kernel; a slower 2^33 says the sin/cos show.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def copy_rate():
    """float4_copy_GBps of tools/membench --json (a child process), or None."""
    try:
        out = subprocess.run([os.path.join(ROOT, "tools", "membench"), "--json", "1048576"], capture_output=True, text=True, timeout=120)
        return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])["float4_copy_GBps"]
    except Exception as e:
        print(f"bench_motion: tools/membench did not run ({e!r})", file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", type=int, nargs="+", default=[65536, 4, 1048576, 1], help="K G pairs")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--lib", default=None, help="another build of the library (an A/B against the one in the tree)")
    ap.add_argument("--twist", action="store_true", help="time dsim_scenes_move_twist: the move that also writes the twist table")
    a = ap.parse_args()
    import torch
    from dronesim_amd import _native as nat
    if a.lib:
        nat.load(a.lib)
    from dronesim_amd import fleet, params
    from dronesim_amd import obstacles as obs
    if not torch.cuda.is_available():
        raise SystemExit("bench_motion needs a HIP device")
    copy = copy_rate()
    ctx = fleet.Context([params.builtin_type("robobee")])
    gate = obs.ObstacleSet.from_urdf(os.path.join(ROOT, "tests", "golden", "gate_50_curved.urdf"), (0, 0, 0), (0, 0, 0))
    proto = gate.to_device(ctx, obs.watch_reach(ctx.types, 0.5))
    dt = 1.0 / 48.0

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters

    for K, G in zip(a.tables[0::2], a.tables[1::2]):
        rng = np.random.default_rng(11)
        pos = rng.uniform([-2.0, -2.0, 1.0], [2.0, 2.0, 3.0], (K, G, 3))
        rpy = rng.uniform([-0.5, -0.5, -np.pi], [0.5, 0.5, np.pi], (K, G, 3))
        scenes = obs.ObstacleScenes(gate, pos, rpy)
        axis = rng.normal(size=(K, G, 3))
        axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
        cases = {}
        for share in (1, 8):
            on = (np.arange(K * G).reshape(K, G) % share) == 0
            m = obs.SceneMotion(scenes, velocity=np.where(on[..., None], rng.uniform(-1.5, 1.5, (K, G, 3)), 0.0),
                                amplitude=np.where(on[..., None], rng.uniform(-0.4, 0.4, (K, G, 3)), 0.0),
                                omega=np.where(on, rng.uniform(3.0, 6.0, (K, G)), 0.0), phase=np.where(on, rng.uniform(-1, 1, (K, G)), 0.0),
                                axis=np.where(on[..., None], axis, 0.0), rate=np.where(on, rng.uniform(2.0, 4.0, (K, G)), 0.0),
                                swing=np.where(on, rng.uniform(0.3, 0.9, (K, G)), 0.0))
            assert int(m.moving.sum()) == int(on.sum())
            dev = scenes.to_device(ctx, prototype_dev=proto)
            if a.twist:
                dev.enable_twist()
            dev.set_motion(m)
            for clock in (7, 2 ** 33):
                c = torch.tensor([clock], dtype=torch.int64, device=ctx.device)
                cases[(share, clock)] = (dev, c, int(on.sum()), K * G - int(on.sum()))
        fns = {key: (lambda d=d, c=c: d.move(c, dt)) for key, (d, c, _, _) in cases.items()}
        for fn in fns.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        t = {key: [] for key in fns}
        for _ in range(a.rounds):
            for key, fn in fns.items():
                t[key].append(timed(fn))
        for (share, clock), (dev, c, moving, static) in cases.items():
            us = np.array(t[(share, clock)])
            nbytes = (208 if a.twist else 176) * moving + 16 * static
            print(json.dumps({
                "what": "dsim_scenes_move_twist" if a.twist else "dsim_scenes_move", "lib": a.lib or "tree", "K": K, "G": G, "slots": K * G, "moving_one_in": share, "clock": clock,
                "us_median": round(float(np.median(us)), 2), "us_min_max": [round(float(us.min()), 2), round(float(us.max()), 2)],
                "algorithmic_bytes": nbytes, "GBps_at_median": round(nbytes / float(np.median(us)) / 1e3, 1),
                "float4_copy_GBps": copy, "iters": a.iters, "rounds": a.rounds}), flush=True)
        for dev in {id(v[0]): v[0] for v in cases.values()}.values():
            dev.close()
    proto.close()
    ctx.close()


if __name__ == "__main__":
    main()
