"""Times the depth camera: N cameras x W x H rays on the gate scene, device events around a batch of captures behind a settled
warm-up.  Prints one JSON line: us per capture, rays per second and, with a counting build (--lib a library built with
-DDSIM_CAM_COUNT), the mean triangle tests per ray.  DSIM_RAY_ONE_CELL=1 in the environment makes the set's ray grid one cell
that lists every triangle: the brute-force baseline the grid has to beat (run both and compare).

    python tools/bench_camera.py [--cameras 4096] [--res 64 48] [--subdiv 0] [--iters 200] [--warmup 50] [--lib PATH]

--drones: the drones case instead.  4 096 tellos on a 64 x 64 lattice of 1 m pitch at z = 1, 64 cameras among them at 64 x 48
looking along +x with the nose 0.011 rad up (one pixel row lies in the layer of spheres), the gate scene in the middle of the lattice: the same
capture with drones=False, with drones=True and with drones=True, drone_range=20, one JSON line each (the binning of the fleet is
part of a capture with drones).
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", type=int, default=4096)
    ap.add_argument("--res", type=int, nargs=2, default=(64, 48))
    ap.add_argument("--subdiv", type=int, default=0, help="subdivide the gate's 96 triangles this many times (x 4 each)")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--lib", default=None, help="another build of the library (the counting build)")
    ap.add_argument("--drones", action="store_true", help="the drones case (see above)")
    a = ap.parse_args()
    if a.drones:
        return drones_case(a)
    from dronesim_amd import _native as nat
    if a.lib:
        nat.load(a.lib)
    import torch
    from dronesim_amd.camera import DepthCamera
    from dronesim_amd.envs import CtrlAviary
    from tests import camera_ref as cr
    n, (w, h) = a.cameras, a.res
    # the fleet stands in a disc in front of the gate at (2, 0, 1), every drone looking at it from its own place
    rng = np.random.default_rng(0)
    xyz = np.stack([rng.uniform(-2.0, 1.2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(0.5, 1.5, n)], 1)
    yaw = np.arctan2(-xyz[:, 1], 2.0 - xyz[:, 0]) + rng.uniform(-0.3, 0.3, n)
    rpy = np.stack([rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n), yaw], 1)
    env = CtrlAviary(["tello"], n, initial_xyzs=xyz, initial_rpys=rpy, noise_seed=0, dict_io=False, ground_plane=False)
    sc = cr.scene(a.subdiv)
    cam = DepthCamera(env.ctx, env.state, sc, res=(w, h), ground=True)
    for _ in range(a.warmup):
        cam.capture()
    torch.cuda.synchronize()
    if a.lib and hasattr(env.ctx.lib, "dsim_camera_tests"):
        c = ctypes.c_uint64()
        env.ctx.lib.dsim_camera_tests(ctypes.byref(c))          # (zeroes the counter)
    times = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            cam.capture()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / a.iters)
    rays = n * w * h
    out = {"cameras": n, "res": [w, h], "n_tri": sc.n_tri, "one_cell": os.environ.get("DSIM_RAY_ONE_CELL", "0") == "1",
           "us_per_capture_median": round(float(np.median(times)), 2), "us_per_capture_all": [round(t, 2) for t in times],
           "rays_per_s": round(rays / (float(np.median(times)) * 1e-6), 0),
           "hit_share": round(float((cam.seg >= 0).float().mean().item()), 4)}
    if a.lib and hasattr(env.ctx.lib, "dsim_camera_tests"):
        c = ctypes.c_uint64()
        env.ctx.lib.dsim_camera_tests(ctypes.byref(c))
        out["tri_tests_per_ray"] = round(c.value / (rays * a.iters * a.repeats), 3)
    print(json.dumps(out))
    cam.close()
    env.close()


def drones_case(a):
    from dronesim_amd import _native as nat
    if a.lib:
        nat.load(a.lib)
    import torch
    from dronesim_amd.camera import DepthCamera
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.obstacles import ObstacleSet
    from tests import camera_ref as cr
    n, n_cam, (w, h) = 4096, 64, a.res
    i = np.arange(n)
    xyz = np.stack([i % 64, i // 64, np.ones(n)], 1).astype(np.float64)
    rpy = np.tile([0.0, -0.011, 0.0], (n, 1))
    env = CtrlAviary(["tello"], n, initial_xyzs=xyz, initial_rpys=rpy, noise_seed=0, dict_io=False, ground_plane=False)
    gate = ObstacleSet.from_urdf(os.path.join(cr.GOLDEN, "gate_50_curved.urdf"), (32.5, 32.5, 1.0), (0, 0, 0))
    cams = (np.arange(n_cam) * 61 + 7) % n                     # spread over the lattice
    for label, kw in (("drones=False", {}), ("drones=True", dict(drones=True)), ("drones=True, drone_range=20", dict(drones=True, drone_range=20.0))):
        cam = DepthCamera(env.ctx, env.state, gate, res=(w, h), ground=True, cameras=cams, **kw)
        for _ in range(a.warmup):
            cam.capture()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                cam.capture()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3 / a.iters)
        print(json.dumps({"case": label, "drones_in_world": n, "cameras": n_cam, "res": [w, h], "n_tri": gate.n_tri,
                          "us_per_capture_median": round(float(np.median(times)), 2), "us_per_capture_all": [round(t, 2) for t in times],
                          "drone_pixel_share": round(float((cam.seg <= -3).float().mean().item()), 4),
                          "outside": cam.drones_outside() if cam.drones else None}))
        cam.close()
    env.close()


if __name__ == "__main__":
    main()
