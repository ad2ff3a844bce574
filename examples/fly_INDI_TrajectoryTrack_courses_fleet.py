#!/usr/bin/env python3
"""The loop of examples/fly_INDI_TrajectoryTrack_fleet.py with a course PER DRONE, made on the device.

    python examples/fly_INDI_TrajectoryTrack_courses_fleet.py --num_drones 65536 --duration_sec 5

Every drone gets three seeded random gates, cumsum(uniform(-3, 3)) + (0, 0, 6) kept above 1 m, and its own minimum-snap course
through them: what the reference's trajGenerator(gates, max_vel=0.7, gamma=1e6) (fly_INDI_TrajectoryTrack.py:127-131) computes per
call on the host, 5-60 ms each, is one launch for the whole fleet here (fleet.TrajectoryBank), and the per-step sampling reads
each drone's own course (fleet.BankTrajectoryTargets).  240 Hz physics, 2 physics steps per control step, every drone offset on
a 10 m grid.  A course made here is exactly at rest at t = 0, where the reference's yaw-from-velocity rule has no heading (NaN);
the flight starts one control step into the course.

--gates: the committed gate stands at each drone's own three waypoints (obstacles.ObstacleScenes: one prototype on the device, a
scene of three placements per drone), yawed so that its normal lies along the xy direction of the course's velocity there; the
flight is watched (obstacle_watch=scenes) and the run prints obstacle_contacts() and the least clearance per gate slot.  With
--vision every drone also carries a camera that sees its own gates, and one depth frame is saved (--out).  With --scan N every
drone carries a ring of N range beams (scanner.RangeScanner through the env's range_scan=) against its own gates, scanned behind
every step, and the fleet's least range per gate slot is printed beside the clearances.  --gates also turns the gate passage watch
on (gate_watch=Aperture: the rectangle |y| <= 0.30, |z| <= 0.20 m on the gate's plane x = 0, inside the mesh's opening): the run
prints how many drones flew through 0 / 1 / 2 / 3 of their gates in order, the misses and wrong-way crossings, and the fleet's
median passage time per slot.  Every drone starts AT its gate 0, on the plane, which is no forward crossing: gate 1 is due first.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dronesim_amd.envs import CtrlAviary  # noqa: E402
from dronesim_amd.fleet import BankTrajectoryTargets, TrajectoryBank  # noqa: E402


def random_gates(n, seed):
    """[n, 3, 3]: three gates per drone, the lowest above 1 m."""
    rng = np.random.default_rng(seed)
    g = np.cumsum(rng.uniform(-3.0, 3.0, (n, 3, 3)), axis=1) + np.array([0.0, 0.0, 6.0])
    low = g[:, :, 2].min(axis=1) < 1.0
    g[low, :, 2] += (1.0 - g[low, :, 2].min(axis=1))[:, None]
    return g


def gate_scenes(ctx, bank, gates, dt):
    """One scene per drone: the gate prototype at the drone's three waypoints, its normal (the prototype's x axis) along the xy
    direction of the course's velocity there.  The velocity comes from the bank's coefficients through its own sampler; a course
    is at rest at both ends, so the first and last gate take the direction a control step inside the course."""
    from dronesim_amd.obstacles import ObstacleScenes, ObstacleSet
    n = gates.shape[0]
    proto = ObstacleSet.from_urdf(os.path.join(ROOT, "tests", "golden", "gate_50_curved.urdf"), (0, 0, 0), (0, 0, 0))
    TS = bank.ts[:3, :n].T.cpu().numpy()                                   # [n, 3]: when course k passes its waypoints
    rpy = np.zeros((n, 3, 3))
    for j in range(3):
        t = np.clip(TS[:, j], dt, np.maximum(TS[:, 2] - dt, dt))
        probe = BankTrajectoryTargets(ctx, n, bank, t0=t)
        probe.sample(0.0)
        v = probe.fields(3, 3).T.cpu().numpy()
        rpy[:, j, 2] = np.arctan2(v[:, 1], v[:, 0])
    return ObstacleScenes(proto, gates, rpy)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_drones", type=int, default=4096)
    ap.add_argument("--duration_sec", type=float, default=5.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--times", default="optimize", choices=["optimize", "tmin"],
                    help="optimize: the reference's behaviour (segment times searched per course); tmin: distance / max_vel")
    ap.add_argument("--gates", action="store_true", help="stand a gate at each drone's own waypoints and watch it (ObstacleScenes)")
    ap.add_argument("--vision", action="store_true", help="with --gates: every drone carries a camera; one depth frame is saved")
    ap.add_argument("--out", default="courses_depth.npy", help="where --vision saves its frame")
    ap.add_argument("--margin", type=float, default=1.0, help="obstacle_margin of --gates [m]")
    ap.add_argument("--scan", type=int, default=0, metavar="N",
                    help="with --gates: every drone carries a ring of N range beams (1 .. 64) against its own gates")
    A = ap.parse_args(argv)
    if A.vision and not A.gates:
        ap.error("--vision needs --gates")
    if A.scan and not A.gates:
        ap.error("--scan needs --gates")
    if not 0 <= A.scan <= 64:
        ap.error("--scan takes 1 .. 64 beams")
    n, AGGR, FREQ = A.num_drones, 2, 240                                   # fly_INDI_TrajectoryTrack.py:108,162-164
    side = int(np.ceil(np.sqrt(n)))
    off = 10.0 * np.stack([np.arange(n) % side, np.arange(n) // side, np.zeros(n)], 1).astype(np.float64)
    gates = random_gates(n, A.seed)
    if A.gates:
        # the scenes need the courses and the env's keywords need the scenes: the bank is made on a context of its own first
        from dronesim_amd.fleet import Context
        from dronesim_amd.params import builtin_type
        ctx0 = Context([builtin_type("robobee")])
        scenes = gate_scenes(ctx0, TrajectoryBank(ctx0, gates, max_vel=0.7, gamma=1e6, times=A.times), gates, AGGR / FREQ)
        ctx0.close()
        from dronesim_amd.obstacles import Aperture
        opening = Aperture((0, 0, 0), (1, 0, 0), (0, 1, 0), (0.30, 0.20), "rect", outer=(0.56, 0.40))
        watch = dict(obstacle_watch=scenes, obstacle_scene_id=np.arange(n), obstacle_offsets=off, obstacle_margin=A.margin,
                     gate_watch=opening, gate_start=1)        # (gate_scenes=None: the watch's scenes and their device object)
        if A.vision:
            watch["vision_attributes"] = True
        if A.scan:
            # (the scanner shares the watch's device scenes; the plane is left out: the least range is then a gate's)
            from dronesim_amd.scanner import RangeScanner
            watch.update(range_scan=RangeScanner.fan(A.scan), range_max=10.0, range_ground=False)
    else:
        watch = {}
    env = CtrlAviary(["robobee"], n, initial_xyzs=gates[:, 0, :] + off, aggregate_phy_steps=AGGR, freq=FREQ, dict_io=False, **watch)
    t_gen = time.time()
    bank = TrajectoryBank(env.ctx, gates, max_vel=0.7, gamma=1e6, times=A.times)
    status, evals = bank.status, bank.evals                                # (host copies: the launch has finished after this)
    t_gen = time.time() - t_gen
    print(f"{n} courses made on the device in {t_gen * 1e3:.1f} ms wall (launch + read-back); {int((status != 0).sum())} could not "
          f"be made; evaluations of J per course: median {int(np.median(evals))}, most {int(evals.max())}")
    dt_ctrl = AGGR / FREQ
    tgt = BankTrajectoryTargets(env.ctx, n, bank, t0=np.full(n, dt_ctrl), offsets=off)
    steps = int(A.duration_sec * FREQ / AGGR)
    least = np.full((n, 3), np.inf) if A.gates else None
    least_range = np.full(3, np.inf)                                       # --scan: the fleet's least range per gate slot
    frame = None
    START = time.time()
    for k in range(steps):
        tgt.sample(dt_ctrl)
        env.step_fused(tgt, control_timestep=dt_ctrl, action=np.full((n, 4), 0.4, dtype=np.float32) if k == 0 else None)
        if A.gates:
            clr, near = (x.cpu().numpy() for x in env.last_obstacle_clearance)
            seen = near >= 0                                               # (one body per gate: `nearest` is the gate's slot)
            np.minimum.at(least, (np.nonzero(seen)[0], near[seen]), clr[seen])
        if A.scan:
            rng_, hit = env.ranges, env.range_hits                         # [N beams, n]; one body per gate: a hit is the gate's slot
            for j in range(3):
                least_range[j] = min(least_range[j], float(torch.where(hit == j, rng_, torch.full_like(rng_, float("inf"))).min()))
        if A.vision and frame is None and bool((env.seg >= 0).any()):
            frame = env.dep.clone()
    pos = env.state.pos.T.cpu().numpy()
    el = time.time() - START
    want = tgt.fields(0, 3).T.cpu().numpy()
    err = np.linalg.norm(pos - want, axis=1)
    print(f"{n} drones x {steps} env steps in {el:.2f} s wall ({n * steps / el:.3e} drone-steps/s incl. host loop); "
          f"distance to the own target: median {np.median(err):.3f} m, worst {err.max():.3f} m")
    if A.gates:
        per_slot = [f"gate {j}: {least[:, j].min():.3f} m ({int(np.isfinite(least[:, j]).sum())} drones within {A.margin} m)"
                    + (f", least range of {A.scan} beams {least_range[j]:.3f} m" if A.scan else "") for j in range(3)]
        print(f"obstacle_contacts() = {env.obstacle_contacts()} drone x steps with the bounding sphere on a gate; least clearance per "
              f"gate slot: " + "; ".join(per_slot))
        due, when = env.gate_due.cpu().numpy(), env.gate_pass_time.cpu().numpy() * dt_ctrl       # (one query per control step)
        passed = np.bincount(np.clip(due - 1, 0, 3), minlength=4)
        med = ["-" if np.isnan(when[j]).all() else f"{np.nanmedian(when[j]):.2f} s" for j in range(3)]
        print(f"gates passed in order (gate 0 is the start): " + ", ".join(f"{passed[k]} drones passed {k}" for k in range(3))
              + f"; gate_passes() = {env.gate_passes()}, gate_misses() = {env.gate_misses()}, gate_wrong_way() = "
              f"{env.gate_wrong_way()}, gate_out_of_order() = {env.gate_out_of_order()}, gate_unswept() = {env.gate_unswept()}; "
              f"median passage time per slot: " + ", ".join(f"gate {j}: {med[j]}" for j in range(3)))
    if A.vision:
        np.save(A.out, (frame if frame is not None else env.dep).cpu().numpy())
        print(f"depth frame [{n}, 48, 64] saved to {A.out}" + ("" if frame is not None else " (no gate came into view)"))
    env.close()
    return pos - off, gates


if __name__ == "__main__":
    main()
