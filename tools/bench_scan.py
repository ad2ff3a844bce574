"""Times the range scanner: N tellos x 16 beams on the gate scene, device events around a batch of scans behind a settled warm-up
(the protocol of tools/bench_camera.py: five repeats, the median).  The fleet is N replicas of one task by offsets: every drone
stands in front of the gate at (2, 0, 1) of ITS task frame and is stored at that place plus its own offset, 8 m apart on a square
lattice.  One JSON line per fleet size: us per scan and rays per second.

    python tools/bench_scan.py [--sizes 65536 1048576] [--beams 16] [--subdiv 0] [--iters 200] [--warmup 50] [--lib PATH]

For the camera's time at the same 16 rays per drone run tools/bench_camera.py --cameras 65536 --res 4 4: the only other way to
get 16 rays per drone.

--drones: the drones case instead.  The 4 096-drone lattice of tests/camera_drones_ref.lattice_fleet() (1 m pitch at z = 1), the
gate in the middle of it, every drone scanning: drones=False, drones=True and drones=True, drone_range=20, one JSON line each (the
binning of the fleet is part of a scan with drones).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, scanner, a):
    for _ in range(a.warmup):
        scanner.scan()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            scanner.scan()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / a.iters)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=(65536, 1048576))
    ap.add_argument("--beams", type=int, default=16)
    ap.add_argument("--subdiv", type=int, default=0, help="subdivide the gate's 96 triangles this many times (x 4 each)")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--lib", default=None, help="another build of the library (an A/B against the one in the tree)")
    ap.add_argument("--drones", action="store_true", help="the drones case (see above)")
    a = ap.parse_args()
    from dronesim_amd import _native as nat
    if a.lib:
        nat.load(a.lib)
    import torch
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.scanner import RangeScanner
    from tests import camera_ref as cr
    if a.drones:
        return drones_case(a, torch)
    beams = RangeScanner.fan(a.beams)
    sc = cr.scene(a.subdiv)
    for n in a.sizes:
        # in its task frame every drone stands in a disc in front of the gate, as tools/bench_camera.py lays its cameras out
        rng = np.random.default_rng(0)
        task = np.stack([rng.uniform(-2.0, 1.2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(0.5, 1.5, n)], 1)
        rpy = np.stack([rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n), rng.uniform(-np.pi, np.pi, n)], 1)
        side = int(np.ceil(np.sqrt(n)))
        off = np.stack([(np.arange(n) % side) * 8.0, (np.arange(n) // side) * 8.0, np.zeros(n)], 1)
        env = CtrlAviary(["tello"], n, initial_xyzs=task + off, initial_rpys=rpy, noise_seed=0, dict_io=False, ground_plane=False)
        scanner = RangeScanner(env.ctx, env.state, sc, beams, t_min=0.05, t_max=10.0, ground=True, offsets=off)
        times = timed(torch, scanner, a)
        med = float(np.median(times))
        print(json.dumps({"drones": n, "beams": a.beams, "n_tri": sc.n_tri, "us_per_scan_median": round(med, 2),
                          "us_per_scan_all": [round(t, 2) for t in times], "rays_per_s": round(n * a.beams / (med * 1e-6), 0),
                          "hit_share": round(float((scanner.hits >= 0).float().mean().item()), 4),
                          "ground_share": round(float((scanner.hits == -2).float().mean().item()), 4)}))
        scanner.close()
        env.close()


def drones_case(a, torch):
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.obstacles import ObstacleSet
    from dronesim_amd.scanner import RangeScanner
    from tests import camera_drones_ref as dr
    from tests import camera_ref as cr
    st = dr.lattice_fleet()
    n = st.shape[0]
    env = CtrlAviary(["tello"], n, initial_xyzs=st[:, :3].astype(np.float64), noise_seed=0, dict_io=False, ground_plane=False)
    env.state.set_fields(0, torch.from_numpy(np.ascontiguousarray(st.T)))
    gate = ObstacleSet.from_urdf(os.path.join(cr.GOLDEN, "gate_50_curved.urdf"), (32.5, 32.5, 1.0), (0, 0, 0))
    beams = RangeScanner.fan(a.beams)
    for label, kw in (("drones=False", {}), ("drones=True", dict(drones=True)), ("drones=True, drone_range=20", dict(drones=True, drone_range=20.0))):
        scanner = RangeScanner(env.ctx, env.state, gate, beams, t_min=0.05, t_max=1000.0, ground=True, **kw)
        times = timed(torch, scanner, a)
        med = float(np.median(times))
        print(json.dumps({"case": label, "drones": n, "beams": a.beams, "n_tri": gate.n_tri, "us_per_scan_median": round(med, 2),
                          "us_per_scan_all": [round(t, 2) for t in times], "rays_per_s": round(n * a.beams / (med * 1e-6), 0),
                          "drone_hit_share": round(float((scanner.hits <= -3).float().mean().item()), 4),
                          "outside": scanner.drones_outside() if scanner.drones else None}))
        scanner.close()
    env.close()


if __name__ == "__main__":
    main()
