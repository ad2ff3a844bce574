#!/usr/bin/env python3
"""A decentralised controller on a fleet: every VelocityAviary drone flies Reynolds' three rules (separation, alignment,
cohesion) from its own nearest-neighbour observation alone — env.last_neighbors, the k closest drones within a radius with
their relative position and velocity (dsim_knn behind every step) — plus a common cruise direction.  No drone reads another
drone's state, and nothing leaves the device: the rules are a few torch ops on [k, 3, N].

    python examples/fly_velocity_flock_fleet.py --num_drones 4096 --duration_sec 5

--sight stands the committed gate (tests/golden/gate_50_curved.urdf) in the flock's way and lets a drone flock only with the
neighbours it can SEE: env.last_neighbor_sight (dsim_line_of_sight behind every step's dsim_knn) says, per slot, whether the gate's
frame hides that neighbour, and hidden ones are dropped from the three sums.  --sight-drones lets the other drones hide
neighbours too, as their bounding spheres (dsim_line_of_sight_drones): in open air, or together with --sight's gate.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dronesim_amd.envs import VelocityAviary  # noqa: E402

GATE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "gate_50_curved.urdf")


def reynolds(nb, cruise, w_sep=0.6, w_ali=0.5, w_coh=0.15, sight=None):
    """[3, N] velocity wish from a Neighbors record: unused slots hold rel = 0 and dist = +inf, so they add nothing.  ``sight``: the
    Sight of that record; a neighbour that is not visible adds nothing either."""
    if sight is not None:
        see = (sight.visible != 0).unsqueeze(1)                      # [k, 1, N]; an unused slot is not visible
        seen = see.sum(0).squeeze(0).clamp(min=1)
        separation = -(nb.rel_pos * see / nb.dist.square().clamp(min=1e-4).unsqueeze(1)).sum(0)
        return cruise[:, None] + w_sep * separation + w_ali * (nb.rel_vel * see).sum(0) / seen + w_coh * (nb.rel_pos * see).sum(0) / seen
    seen = (nb.index >= 0).sum(0).clamp(min=1)                       # [N]
    separation = -(nb.rel_pos / nb.dist.square().clamp(min=1e-4).unsqueeze(1)).sum(0)
    alignment = nb.rel_vel.sum(0) / seen
    cohesion = nb.rel_pos.sum(0) / seen
    return cruise[:, None] + w_sep * separation + w_ali * alignment + w_coh * cohesion


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--drone", default="tello")
    ap.add_argument("--num_drones", type=int, default=4096)
    ap.add_argument("--duration_sec", type=float, default=5.0)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--radius", type=float, default=3.0)
    ap.add_argument("--sight", action="store_true", help="stand the gate in the flock and drop the neighbours it hides")
    ap.add_argument("--sight-drones", action="store_true", help="the other drones hide neighbours too (alone: open air, no gate)")
    A = ap.parse_args(argv)
    n, AGGR, FREQ = A.num_drones, 5, 240
    rng = np.random.default_rng(0)
    side = int(np.ceil(np.sqrt(n)))
    xyz = np.stack([(np.arange(n) % side) * 1.5, (np.arange(n) // side) * 1.5, np.full(n, 2.0)], 1) + rng.uniform(-0.3, 0.3, (n, 3))
    kw = {}
    if A.sight:
        # the gate a little ahead of the flock's middle along the cruise direction, its opening at the flock's height
        from dronesim_amd.obstacles import ObstacleSet
        mid = 0.75 * (side - 1)
        kw = dict(neighbor_sight=True, neighbor_sight_scene=ObstacleSet.from_urdf(GATE, (mid + 1.0, mid + 0.3, 2.0), (0, 0, 0)))
    if A.sight_drones:
        kw.update(neighbor_sight=True, neighbor_sight_drones=True)
    see = A.sight or A.sight_drones
    env = VelocityAviary([A.drone], n, initial_xyzs=xyz, initial_vels=rng.uniform(-0.5, 0.5, (n, 3)), aggregate_phy_steps=AGGR,
                         freq=FREQ, dict_io=False, neighbor_obs=A.k, neighbor_radius=A.radius, drone_watch=True, **kw)
    cruise = torch.tensor([0.6, 0.2, 0.0], device=env.ctx.device)
    limit = float(env.SPEED_LIMIT[0])
    steps = int(A.duration_sec * FREQ / AGGR)
    nb, sight = env.neighbor_sight() if see else (env.nearest_neighbors(), None)
    hidden = by_drones = 0
    START = time.time()
    for _ in range(steps):
        wish = reynolds(nb, cruise, sight=sight)
        speed = wish.norm(dim=0)
        action = torch.cat([wish / speed.clamp(min=1e-6), (speed / limit).clamp(max=1.0)[None, :]], 0).T.contiguous()
        env.step(action)
        nb = env.last_neighbors
        if see:
            sight = env.last_neighbor_sight
            hidden += int(((sight.visible == 0) & (nb.index >= 0)).sum().item())
            by_drones += int((sight.blocker <= -3).sum().item())
    nearest = nb.dist[0][torch.isfinite(nb.dist[0])]
    q = torch.quantile(nearest, torch.tensor([0.0, 0.05, 0.5, 0.95], device=nearest.device)).cpu().numpy()
    contacts = env.drone_contacts()
    print(f"{n} drones x {steps} env steps in {time.time() - START:.2f} s wall; nearest neighbour at min / 5 % / median / 95 % = "
          f"{q.round(3)} m, {int(nb.count.float().mean().item() * 10) / 10} drones within {A.radius} m on average; "
          f"drone_contacts() = {contacts}")
    if see:
        print(f"neighbour slots hidden, summed over the steps: {hidden}" + (f", {by_drones} of them by another drone" if A.sight_drones else " (by the gate)"))
    env.close()
    return q, contacts


if __name__ == "__main__":
    main()
