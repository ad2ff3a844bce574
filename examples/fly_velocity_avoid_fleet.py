#!/usr/bin/env python3
"""Obstacle avoidance from the obstacle witness: every VelocityAviary drone cruises along +x through a field of gates placed
in its own scene, and adds to that goal velocity a repulsion away from the closest point of the world — env.last_obstacle_witness,
the vector from the drone to that point (dsim_obstacle_witness_scenes in place of the point watch behind every step).  The flight
is flown twice, without and with the term, and prints obstacle_contacts() of both.  Nothing leaves the device: the term is a few
torch ops on [3, N].  With --moving the gates swing across the course (obstacle_motion=SceneMotion: a sideways oscillation of
every gate, each at its own pace and phase, evaluated on the device before every step's watch); the repulsion is the same.
With --moving --lead a third flight adds env.last_obstacle_witness_velocity (obstacle_witness_velocity=True: the velocity of the
closest point as a point of its moving gate, from dsim_obstacle_witness_scenes_vel), weighted by the repulsion's own falloff: the
drone is carried along with the gate that closes on it, so the repulsion leads the gate instead of answering where it was.  The
least clearance of each flight is printed; no figure is promised for it.
With --witnesses M (1..8) the env answers with the M closest gates of every drone (obstacle_witnesses=M:
env.last_obstacle_witnesses, dsim_obstacle_witnesses_scenes in the witness's place) and the repulsion is summed over the filled
slots: a drone between two gates is pushed by both, and nothing jumps when the nearer one changes.  With --moving --lead each slot
is led by its own gate's velocity.
With --filter one more flight replaces the repulsion by the velocity safety filter (velocity_filter=dict(alpha=...),
env.step_velocity: dsim_velocity_filter on the witnesses the env keeps behind each step, M = --witnesses or 3 of them, with their
velocities when the gates swing): the goal velocity is changed only where a control-barrier row h' + alpha h >= 0 is violated, and
then as little as the rows allow.  It prints the same two figures and env.filter_counts().  The filter certifies the velocity it
returns, not the flight: the vehicle follows a velocity command with a lag, which --buffer has to cover, and the speed fraction is
clamped at 1 after the filter, which can undo a row.  A drone whose goal points straight into a bar stops in front of it (the
projection has nowhere to slide), and obstacle_contacts() counts drone x steps, so a drone that stands close counts for long: no
figure is promised for it.
With --plan B (2..32) one more flight plans before it steps: every control step each drone forms B candidate velocities — the goal
direction and B - 1 yawed or pitched about it —, asks env.corridor_clearance (corridor=dict(k=B, ...): dsim_corridor_clearance,
its bounding sphere swept along v_c x --horizon against the gates where they stand and the ground) and takes the candidate nearest
the goal direction whose corridor is free, or, where none is, the one with the largest clearance.  With --filter the chosen
velocity goes through the velocity filter.  The corridor is a straight one over a short horizon: no figure is promised for it.

    python examples/fly_velocity_avoid_fleet.py --num_drones 4096 --duration_sec 6 [--moving [--lead]] [--witnesses 3] [--filter] [--plan 9]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dronesim_amd.envs import VelocityAviary  # noqa: E402
from dronesim_amd.obstacles import ObstacleScenes, ObstacleSet, SceneMotion  # noqa: E402

GATE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "gate_50_curved.urdf")


def repulsion(rel, clearance, radius, margin, gain):
    """[3, N]: away from the closest point, growing as the clearance shrinks (a potential field's gradient, 1 / c - 1 / margin,
    capped); zero for a drone with nothing within the margin, whose rel is 0 and whose clearance is the margin."""
    d = (clearance + radius).clamp(min=1e-3)                         # |rel|, guarded where the distance vanishes
    away = -rel / d
    push = (1.0 / clearance.clamp(min=0.05) - 1.0 / margin).clamp(min=0.0, max=10.0)
    return gain * push * away


def lead_term(vel, clearance, margin):
    """[3, N]: the closest point's own velocity, faded in as the repulsion is — 0 at the margin and beyond (where vel is 0 too),
    whole where the repulsion has reached its cap."""
    weight = ((1.0 / clearance.clamp(min=0.05) - 1.0 / margin) / 10.0).clamp(min=0.0, max=1.0)
    return weight * vel


def candidates(B, spread):
    """[B, 3] unit directions about +x, nearest the goal direction first: +x itself, then pairs yawed and pitched by growing
    angles up to ``spread`` [rad]."""
    out = [np.array([1.0, 0.0, 0.0])]
    rings = max((B - 1 + 3) // 4, 1)
    for j in range(B - 1):
        ang = spread * (j // 4 + 1) / rings
        c, sn = np.cos(ang), np.sin(ang) * (1.0 if j % 2 == 0 else -1.0)
        out.append(np.array([c, sn, 0.0]) if (j // 2) % 2 == 0 else np.array([c, 0.0, sn]))
    return np.stack(out)


def fly_planned(A, filtered: bool):
    """The planned flight: corridor_clearance on a fan of candidate velocities, then a step (through the filter with --filter)."""
    n, AGGR, FREQ, K, B = A.num_drones, 5, 240, 64, A.plan
    scenes, moving, off, xyz = world(A)
    if filtered:
        moving.update(velocity_filter=dict(alpha=A.alpha, buffer_obstacle=A.buffer, floor=0.0))
    env = VelocityAviary([A.drone], n, initial_xyzs=xyz, aggregate_phy_steps=AGGR, freq=FREQ, dict_io=False, obstacle_watch=scenes,
                         obstacle_scene_id=np.arange(n) % K, obstacle_offsets=off, obstacle_margin=A.margin,
                         obstacle_witness="world" if filtered else None, obstacle_witness_velocity=filtered and A.moving,
                         obstacle_witnesses=(A.witnesses or 3) if filtered else 0,
                         corridor=dict(k=B, piece=0.5, sag=A.buffer, ground=True), **moving)
    dev = env.ctx.device
    limit = float(env.SPEED_LIMIT[0])
    cand = torch.from_numpy(candidates(B, np.radians(A.spread)).astype(np.float32)).to(dev) * A.speed      # [B, 3] velocities
    rel = (cand * A.horizon)[:, :, None].expand(B, 3, n).contiguous()
    rank = torch.arange(B, device=dev)[:, None]
    steps = int(A.duration_sec * FREQ / AGGR)
    closest, blocked = float("inf"), 0
    START = time.time()
    for _ in range(steps):
        c = env.corridor_clearance(rel).clearance                        # [B, N]
        free = c > 0.0
        first_free = torch.where(free, rank, B).min(0).values           # the candidate nearest the goal whose corridor is free
        pick = torch.where(first_free < B, first_free, c.argmax(0))
        blocked += int((first_free == B).sum().item())
        wish = cand[pick].T                                              # [3, N]
        if filtered:
            env.step_velocity(wish)
        else:
            speed = wish.norm(dim=0)
            env.step(torch.cat([wish / speed.clamp(min=1e-6), (speed / limit).clamp(max=1.0)[None, :]], 0).T.contiguous())
        closest = min(closest, float(env.last_obstacle_clearance[0].min().item()))
    contacts = env.obstacle_contacts()
    print(f"planned on {B} corridors of {A.horizon:.2f} s{' through the velocity filter' if filtered else ''}{', swinging gates' if A.moving else ''}: "
          f"{n} drones x {steps} env steps in {time.time() - START:.2f} s wall; obstacle_contacts() = {contacts} drone x steps, "
          f"least clearance {closest:.3f} m; {blocked} drone x steps with no free corridor, corridor_unserved() = {env.corridor_unserved()}")
    env.close()
    return contacts


def world(A):
    """(scenes, the motion keywords, offsets, initial positions) of every flight."""
    n, K, G = A.num_drones, 64, 6
    rng = np.random.default_rng(0)
    gate = ObstacleSet.from_urdf(GATE, (0, 0, 0), (0, 0, 0))
    # G gates per scene, strung along the course with a sideways scatter and any yaw: some stand in the way
    pos = np.stack([2.0 + 2.0 * np.arange(G)[None, :] + rng.uniform(-0.5, 0.5, (K, G)), rng.uniform(-1.0, 1.0, (K, G)),
                    2.0 + rng.uniform(-0.6, 0.6, (K, G))], 2)
    rpy = np.stack([np.zeros((K, G)), np.zeros((K, G)), rng.uniform(-np.pi, np.pi, (K, G))], 2)
    scenes = ObstacleScenes(gate, pos, rpy)
    moving = {}
    if A.moving:
        # every gate swings across the course: +-0.8 m along y, a period of 2 .. 4 s, its own phase
        amp = np.zeros((K, G, 3))
        amp[..., 1] = 0.8
        moving = dict(obstacle_motion=SceneMotion(scenes, amplitude=amp, omega=rng.uniform(0.5 * np.pi, np.pi, (K, G)),
                                                  phase=rng.uniform(-np.pi, np.pi, (K, G))))
    side = int(np.ceil(np.sqrt(n)))
    off = np.stack([(np.arange(n) % side) * 40.0, (np.arange(n) // side) * 40.0, np.zeros(n)], 1)      # a frame per drone
    xyz = off + np.array([0.0, 0.0, 2.0]) + rng.uniform(-0.5, 0.5, (n, 3))
    return scenes, moving, off, xyz


def fly(A, avoid: bool, lead: bool = False, filtered: bool = False):
    n, AGGR, FREQ, K = A.num_drones, 5, 240, 64
    scenes, moving, off, xyz = world(A)
    if filtered:
        # the filter's rows come from the witnesses record (and its velocities on moving gates); the floor is the plane z = 0
        moving.update(velocity_filter=dict(alpha=A.alpha, buffer_obstacle=A.buffer, floor=0.0))
        lead = A.moving
    env = VelocityAviary([A.drone], n, initial_xyzs=xyz, aggregate_phy_steps=AGGR, freq=FREQ, dict_io=False, obstacle_watch=scenes,
                         obstacle_scene_id=np.arange(n) % K, obstacle_offsets=off, obstacle_margin=A.margin,
                         obstacle_witness="world", obstacle_witness_velocity=lead,
                         obstacle_witnesses=(A.witnesses or 3) if filtered else A.witnesses, **moving)
    dev = env.ctx.device
    radius = float(np.float32(env.ctx.types[0].collision_sphere))
    goal = torch.tensor([A.speed, 0.0, 0.0], device=dev)[:, None].expand(3, n)
    limit = float(env.SPEED_LIMIT[0])
    if filtered:
        steps = int(A.duration_sec * FREQ / AGGR)
        closest = float("inf")
        START = time.time()
        for _ in range(steps):
            env.step_velocity(goal)
            closest = min(closest, float(env.last_obstacle_clearance[0].min().item()))
        contacts, (changed, lost) = env.obstacle_contacts(), env.filter_counts()
        print(f"with the velocity filter{', swinging gates' if A.moving else ''}: {n} drones x {steps} env steps in {time.time() - START:.2f} s wall; "
              f"obstacle_contacts() = {contacts} drone x steps, least clearance {closest:.3f} m; filter_counts() = {changed} drone x steps "
              f"changed, {lost} with a dropped row")
        env.close()
        return contacts
    if A.witnesses:
        w = env.obstacle_witnesses()                                 # [M, N], [M, 3, N]: unfilled slots push by nothing
        clr, rel = w.clearance, w.rel
    else:
        clr, _, rel = env.obstacle_witness()
    vel = torch.zeros_like(rel)
    steps = int(A.duration_sec * FREQ / AGGR)
    closest = float("inf")
    START = time.time()
    for _ in range(steps):
        # (with --witnesses the terms are [M, 3, N] against clearances [M, 1, N]: summed over the slots)
        c = clr[:, None, :] if A.witnesses else clr
        push = repulsion(rel, c, radius, A.margin, A.gain)
        wish = goal + (push.sum(0) if A.witnesses else push) if avoid else goal
        if lead:
            carry = lead_term(vel, c, A.margin)
            wish = wish + (carry.sum(0) if A.witnesses else carry)
        speed = wish.norm(dim=0)
        action = torch.cat([wish / speed.clamp(min=1e-6), (speed / limit).clamp(max=1.0)[None, :]], 0).T.contiguous()
        env.step(action)
        if A.witnesses:
            w = env.last_obstacle_witnesses
            clr, rel, vel = w.clearance, w.rel, w.vel if lead else vel
        else:
            (clr, _), rel = env.last_obstacle_clearance, env.last_obstacle_witness
            if lead:
                vel = env.last_obstacle_witness_velocity
        closest = min(closest, float(clr.min().item()))
    contacts = env.obstacle_contacts()
    print(f"{'with' if avoid else 'without'} the repulsion term{' and the lead term' if lead else ''}{', swinging gates' if A.moving else ''}: {n} drones x {steps} env steps in {time.time() - START:.2f} s wall; "
          f"obstacle_contacts() = {contacts} drone x steps, least clearance {closest:.3f} m")
    env.close()
    return contacts


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--drone", default="tello")
    ap.add_argument("--num_drones", type=int, default=4096)
    ap.add_argument("--duration_sec", type=float, default=6.0)
    ap.add_argument("--speed", type=float, default=2.0)
    ap.add_argument("--margin", type=float, default=1.0)
    ap.add_argument("--gain", type=float, default=1.5)
    ap.add_argument("--moving", action="store_true", help="the gates swing across the course (obstacle_motion=SceneMotion)")
    ap.add_argument("--lead", action="store_true", help="with --moving: a third flight adds the closest point's own velocity "
                                                        "(obstacle_witness_velocity=True), weighted by the repulsion's falloff")
    ap.add_argument("--witnesses", type=int, default=0, help="the M closest gates per drone (obstacle_witnesses=M, 1..8): the "
                                                             "repulsion is summed over the filled slots; 0: the one witness")
    ap.add_argument("--filter", action="store_true", help="one more flight with the velocity safety filter in the repulsion's place "
                                                          "(velocity_filter=dict(alpha=...), env.step_velocity)")
    ap.add_argument("--alpha", type=float, default=1.5, help="with --filter: the barrier's rate [1/s]")
    ap.add_argument("--buffer", type=float, default=0.2, help="with --filter: metres kept between the bounding sphere and the gates; it "
                                                              "has to cover the lag with which the vehicle follows a velocity "
                                                              "(with --plan: the corridor's sag)")
    ap.add_argument("--plan", type=int, default=0, help="one more flight that picks among B candidate velocities by their corridor "
                                                        "clearance (corridor=dict(k=B, ...), env.corridor_clearance); 0: none")
    ap.add_argument("--horizon", type=float, default=0.75, help="with --plan: the corridor of a candidate is v x horizon [s] long")
    ap.add_argument("--spread", type=float, default=60.0, help="with --plan: the widest yaw or pitch of a candidate [deg]")
    A = ap.parse_args(argv)
    if A.lead and not A.moving:
        ap.error("--lead needs --moving: a static world's points stand still")
    if A.plan and not 2 <= A.plan <= 32:
        ap.error("--plan takes 2 .. 32 candidates")
    out = fly(A, False), fly(A, True)
    out = out + (fly(A, True, True),) if A.lead else out
    out = out + (fly(A, False, filtered=True),) if A.filter else out
    return out + (fly_planned(A, A.filter),) if A.plan else out


if __name__ == "__main__":
    main()
