#!/usr/bin/env python3
"""The loop of examples/fly_INDI_TrajectoryTrack_fleet.py with a course PER DRONE, made on the device.

    python examples/fly_INDI_TrajectoryTrack_courses_fleet.py --num_drones 65536 --duration_sec 5

Every drone gets three seeded random gates, cumsum(uniform(-3, 3)) + (0, 0, 6) kept above 1 m, and its own minimum-snap course
through them: what the reference's trajGenerator(gates, max_vel=0.7, gamma=1e6) (fly_INDI_TrajectoryTrack.py:127-131) computes per
call on the host, 5-60 ms each, is one launch for the whole fleet here (fleet.TrajectoryBank), and the per-step sampling reads
each drone's own course (fleet.BankTrajectoryTargets).  240 Hz physics, 2 physics steps per control step, every drone offset on
a 10 m grid.  A course made here is exactly at rest at t = 0, where the reference's yaw-from-velocity rule has no heading (NaN);
the flight starts one control step into the course.
"""
import argparse
import os
import sys
import time

import numpy as np

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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_drones", type=int, default=4096)
    ap.add_argument("--duration_sec", type=float, default=5.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--times", default="optimize", choices=["optimize", "tmin"],
                    help="optimize: the reference's behaviour (segment times searched per course); tmin: distance / max_vel")
    A = ap.parse_args(argv)
    n, AGGR, FREQ = A.num_drones, 2, 240                                   # fly_INDI_TrajectoryTrack.py:108,162-164
    side = int(np.ceil(np.sqrt(n)))
    off = 10.0 * np.stack([np.arange(n) % side, np.arange(n) // side, np.zeros(n)], 1).astype(np.float64)
    gates = random_gates(n, A.seed)
    env = CtrlAviary(["robobee"], n, initial_xyzs=gates[:, 0, :] + off, aggregate_phy_steps=AGGR, freq=FREQ, dict_io=False)
    t_gen = time.time()
    bank = TrajectoryBank(env.ctx, gates, max_vel=0.7, gamma=1e6, times=A.times)
    status, evals = bank.status, bank.evals                                # (host copies: the launch has finished after this)
    t_gen = time.time() - t_gen
    print(f"{n} courses made on the device in {t_gen * 1e3:.1f} ms wall (launch + read-back); {int((status != 0).sum())} could not "
          f"be made; evaluations of J per course: median {int(np.median(evals))}, most {int(evals.max())}")
    dt_ctrl = AGGR / FREQ
    tgt = BankTrajectoryTargets(env.ctx, n, bank, t0=np.full(n, dt_ctrl), offsets=off)
    steps = int(A.duration_sec * FREQ / AGGR)
    START = time.time()
    for k in range(steps):
        tgt.sample(dt_ctrl)
        env.step_fused(tgt, control_timestep=dt_ctrl, action=np.full((n, 4), 0.4, dtype=np.float32) if k == 0 else None)
    pos = env.state.pos.T.cpu().numpy()
    el = time.time() - START
    want = tgt.fields(0, 3).T.cpu().numpy()
    err = np.linalg.norm(pos - want, axis=1)
    print(f"{n} drones x {steps} env steps in {el:.2f} s wall ({n * steps / el:.3e} drone-steps/s incl. host loop); "
          f"distance to the own target: median {np.median(err):.3f} m, worst {err.max():.3f} m")
    env.close()
    return pos - off, gates


if __name__ == "__main__":
    main()
