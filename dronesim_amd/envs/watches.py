"""The services that follow every step of the fleet env on its stream: the drone-drone contact watch (``drone_watch``), the
static-obstacle watch (``obstacle_watch``), the depth camera (``vision_attributes``), the range scanner (``range_scan``), the gate
passage watch (``gate_watch``), the nearest-neighbour observation (``neighbor_obs``) and its line of sight (``neighbor_sight``), and
the velocity safety filter that consumes their records on demand (``velocity_filter``).  Their keywords, set-up, state and public
calls, the one epilogue of a launch (``_stepped``) and the four hooks a captured sequence goes through (``_capture_prepare``,
``_captured_step``, ``_capture_keepalive``, ``_replayed``).  A mix-in of ``CtrlAviary``: it uses the env's attributes as they are."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .. import _native as nat


class StepWatches:
    # (class-level "nothing on": an env made without __init__ steps with no service behind it)
    _drone_watch = False          # the drone-drone contact watch behind every step (set by _watch_options)
    _drone_sweep = False          # ... queried along the chords between two samples (drone_sweep=True)
    _drone_prev = None            # ... from where the previous query saw every drone (set by _watch_setup)
    _obst = None                  # the static-obstacle watch's device set (set by _watch_setup)
    _obst_sweep = False           # ... queried along the chord between two samples (obstacle_sweep=True)
    _obst_placed = False          # ... an ObstacleScenes: per-drone placements of one prototype (obstacle_scene_id)
    _obst_ids = None              # ... and then the scene of every drone, in storage order (set by _obstacle_setup)
    _obst_wit = None              # ... with the witness query in the point query's place: "world" or "body" (obstacle_witness=)
    _obst_rel = None              # ... and the vector it writes behind every launch (set by _obstacle_setup)
    _obst_vel = None              # ... and, with obstacle_witness_velocity=True, the velocity of that point behind every launch
    _wit_vel = False
    _obst_m = 0                   # ... with the witnesses query in the witness's place: slots per drone (obstacle_witnesses=m)
    _obst_wits = None             # ... and what it writes behind every launch, slot-major (set by _obstacle_setup)
    _motion = None                # the SceneMotion of the watch's scenes (obstacle_motion=; attached by _obstacle_setup)
    _scene_clock = None           # ... and the Env.steps since reset() its scene time counts, on the device
    _vision = None                # the depth camera of vision_attributes=True (set by _watch_setup)
    _scan = None                  # the range scanner of range_scan= (set by _watch_setup)
    _scan_args = None
    _gate = None                  # the gate passage watch's device scenes (set by _watch_setup)
    _knn_k = 0                    # the nearest-neighbour observation behind every step: how many neighbours (set by _watch_options)
    _knn_sharded = False          # ... refused on demand too when the fleet is sharded
    _knn = None                   # ... its grid, built on first use
    last_neighbors = None         # ... and what it saw behind the last step
    _sight_on = False             # line of sight behind every step's neighbour query (neighbor_sight=True; set by _watch_options)
    _sight = None                 # ... its LineOfSight (set by _watch_setup)
    _sight_demand = None          # ... and those of the on-demand queries, by k
    _sight_drones = False         # ... with the other drones hiding too (neighbor_sight_drones=True)
    _sight_box = None
    last_neighbor_sight = None    # ... and what it saw behind the last step
    _filter_opts = None           # the velocity safety filter's constants (velocity_filter=dict(...); set by _watch_options)
    _filter = None                # ... its VelocityFilter (set by _watch_setup)
    _filter_fresh = False         # ... whether the records behind the last launch describe the current state
    _filter_sampled = False
    _corr_opts = None             # corridor clearance's constants (corridor=dict(...); set by _watch_options)
    _corr = None                  # ... its Corridor (set by _watch_setup)

    # ------------------------------------------------------------------ construction
    def _watch_options(self, *, num_drones, freq, aggregate_phy_steps, dist, drone_watch, drone_watch_margin, obstacle_watch,
                       obstacle_margin, obstacle_sweep, obstacle_sweep_sag, obstacle_sweep_travel, vision_attributes, vision_scene,
                       vision_drones, vision_res, vision_ground, vision_see_drones, vision_drone_range, obstacle_scene_id=None,
                       drone_sweep=False, drone_sweep_sag=0.0, drone_sweep_travel=None, range_scan=None, range_scene=None,
                       range_min=0.0, range_max=10.0, range_ground=True, range_clamp=False, range_see_drones=False,
                       range_drone_range=None, gate_watch=None, gate_scenes=None, gate_start=0, gate_laps=False,
                       gate_travel=None, neighbor_obs=None, neighbor_radius=None, neighbor_vel=None,
                       neighbourhood_radius=np.inf, obstacle_witness=None, neighbor_sight=False,
                       neighbor_sight_scene=None, obstacle_motion=None, obstacle_witness_velocity=False,
                       obstacle_witnesses=0, velocity_filter=None, neighbor_sight_drones=False,
                       neighbor_sight_drone_box=None, corridor=None) -> None:
        """The services' keywords of ``CtrlAviary.__init__``: checked and stashed (the set-up follows in _watch_setup, when the
        context and the storage order exist)."""
        # The reference's Bullet world lets the vehicles' collision shapes act on each other; here every drone is integrated
        # alone.  drone_watch=True: every step / step_fused / adaptor step is followed, on the env's stream, by one
        # dsim_clearance on the state it left (once per Env.step, like the ground watch): drone_contacts() reports how many
        # pairs of bounding spheres overlapped so far, last_clearance holds (clearance, nearest) of the last step
        # (drone_clearance()).  Off by default: nothing is launched.
        if drone_watch and dist is not None and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("drone_watch on a sharded fleet: the radii of the other ranks' drones would have to travel "
                                      "with their positions (Downwash.clearance takes world_pos / world_radius)")
        self._drone_watch, self._drone_watch_margin = bool(drone_watch), float(drone_watch_margin)
        self.last_clearance = None
        self._clearance = None    # grid for drone_clearance(), built on first use
        self._clr_on_demand = None    # int64 [1]: pairs the on-demand queries counted (not Env.steps: drone_contacts() leaves them out)
        # drone_sweep=True: the query behind a launch is dsim_clearance_sweep instead, every drone a sphere of radius
        # R + drone_sweep_sag that moves along the chord from the position the previous query saw (reset() primes it) to the state
        # the launch left, both drones of a pair at the same parameter: with sag >= obstacles.sweep_sag(a_max, time between two
        # queries) and drone_unswept() == 0, drone_contacts() == 0 certifies every state in between as well.
        # drone_sweep_travel [m]: the longest chord that is swept (None: 10 m/s x one Env.step); a longer one is a point sample and is
        # counted by drone_unswept(); the grid's cells grow by twice the travel.  Off by default: nothing new is allocated or launched.
        if not drone_watch and (drone_sweep or drone_sweep_sag != 0.0 or drone_sweep_travel is not None):
            raise ValueError("drone_sweep / drone_sweep_sag / drone_sweep_travel without drone_watch=True")
        if not drone_sweep and (drone_sweep_sag != 0.0 or drone_sweep_travel is not None):
            raise ValueError("drone_sweep_sag / drone_sweep_travel without drone_sweep=True")
        self._drone_sweep, self._drone_sag = bool(drone_sweep), float(drone_sweep_sag)
        self._drone_travel = 10.0 * int(aggregate_phy_steps) / float(freq) if drone_sweep_travel is None else float(drone_sweep_travel)
        if drone_sweep and (not np.isfinite(self._drone_sag) or self._drone_sag < 0.0):
            raise ValueError("drone_sweep_sag must be >= 0")
        if drone_sweep and (not np.isfinite(self._drone_travel) or not self._drone_travel >= 1e-3):
            raise ValueError("drone_sweep_travel must be at least a millimetre")
        self._drone_prev = self._drone_unswept = None
        # The reference puts the dense N x N adjacency row into every observation; neighbors() is its sparse stand-in, cut in grid
        # order and without distances.  neighbor_obs=k (1 .. 16): every launch is followed, on the env's stream, by one dsim_knn on
        # the state it left: last_neighbors holds, per drone, its k closest drones within neighbor_radius (None:
        # neighbourhood_radius, which must then be finite) in ascending order of distance — (index, dist, rel_pos, rel_vel, count)
        # in the caller's numbering, None before the first step; neighbor_vel=False leaves rel_vel out.  nearest_neighbors() asks
        # on demand.  (Without a storage order the record's tensors are the query's own, at fixed addresses: the next launch writes
        # them again, so clone what must outlive a step.)  Two limits: a sharded fleet (the velocities of the other ranks' drones do not travel) and graph capture
        # (the grid's box is re-measured on the host).  Off by default: nothing is allocated or launched.
        if neighbor_obs is None:
            if neighbor_radius is not None or neighbor_vel is not None:
                raise ValueError("neighbor_radius / neighbor_vel without neighbor_obs=k")
        else:
            if isinstance(neighbor_obs, bool) or int(neighbor_obs) != neighbor_obs or not 1 <= int(neighbor_obs) <= nat.KNN_MAX_K:
                raise ValueError(f"neighbor_obs must be a whole number of neighbours in 1 .. {nat.KNN_MAX_K}")
            r = float(neighbourhood_radius if neighbor_radius is None else neighbor_radius)
            if not (np.isfinite(r) and r > 0.0):
                raise ValueError("neighbor_radius must be finite and positive (None: a finite neighbourhood_radius)")
            if dist is not None and dist.is_initialized() and dist.get_world_size() > 1:
                raise NotImplementedError("neighbor_obs on a sharded fleet: the velocities of the other ranks' drones do not travel "
                                          "(Downwash.nearest takes world_pos, without rel_vel)")
        self._knn_k = 0 if neighbor_obs is None else int(neighbor_obs)
        self._knn_radius = float(neighbourhood_radius if neighbor_radius is None else neighbor_radius)
        self._knn_vel = True if neighbor_vel is None else bool(neighbor_vel)
        self._knn_sharded = dist is not None and dist.is_initialized() and dist.get_world_size() > 1
        self._knn_out = None
        # neighbor_sight=True: every launch's dsim_knn is followed, on the env's stream, by one dsim_line_of_sight on the record it
        # just wrote (rel_pos and index, in storage order): last_neighbor_sight holds, per drone and slot, whether the segment to
        # that neighbour is clear of neighbor_sight_scene (default: the obstacle_watch world, whose device set is then shared; an
        # ObstacleScenes goes by obstacle_scene_id), what hides it first and where — a Sight (visible, blocker, frac) [k, N] in the
        # caller's numbering on the drone axis, None before the first step; unused slots read 0 / -1 / +inf.  neighbor_sight()
        # asks on demand.  The world lies in the frame of obstacle_offsets, and the segment of drone i in ITS task frame, from
        # p_i - offset_i to p_j - offset_i: two drones of different replicas (different offsets) may disagree on whether they see
        # each other.  The other drones hide nobody unless neighbor_sight_drones=True: then the query is
        # dsim_line_of_sight_drones, every other drone hides too as its bounding sphere about its stored position (never drone i
        # itself, never the slot's own neighbour; blocker names drone j of the caller's numbering as -3 - j,
        # LineOfSight.seg_drone), the fleet is binned per query on a grid over its bounding box or neighbor_sight_drone_box =
        # (xmin, ymin, xmax, ymax), and a world becomes optional (open air).  A sharded fleet and graph capture are refused by
        # neighbor_obs itself.  Off by default: nothing is allocated or launched.
        if neighbor_sight and neighbor_obs is None:
            raise ValueError("neighbor_sight=True without neighbor_obs=k")
        if neighbor_sight_scene is not None and not neighbor_sight:
            raise ValueError("neighbor_sight_scene without neighbor_sight=True")
        if (neighbor_sight_drones or neighbor_sight_drone_box is not None) and not neighbor_sight:
            raise ValueError("neighbor_sight_drones / neighbor_sight_drone_box without neighbor_sight=True")
        if neighbor_sight_drone_box is not None and not neighbor_sight_drones:
            raise ValueError("neighbor_sight_drone_box without neighbor_sight_drones=True")
        if neighbor_sight and neighbor_sight_scene is None and obstacle_watch is None and not neighbor_sight_drones:
            raise ValueError("neighbor_sight=True needs a world to look at: neighbor_sight_scene=ObstacleSet (or obstacle_watch), "
                             "or neighbor_sight_drones=True")
        from ..drone_targets import check_drone_args
        self._sight_drones = bool(neighbor_sight_drones)
        self._sight_box = check_drone_args(self._sight_drones, None, neighbor_sight_drone_box)
        self._sight_on, self._sight_scene = bool(neighbor_sight), neighbor_sight_scene
        self.last_neighbor_sight = None
        # The reference's Bullet world also holds static bodies (p.loadURDF of a gate); here they act on nothing.
        # obstacle_watch=ObstacleSet: every step / step_fused / adaptor step is followed, on the env's stream, by one
        # dsim_obstacle_clearance on the state it left (once per LAUNCH: a step_fused with n_steps > 1 is sampled once, at its end);
        # obstacle_contacts() reports the drone x Env.step count, last_obstacle_clearance the tensors of the last step.
        # obstacle_offsets [N, 3] (the caller's numbering): the set lies in the frame of each drone's task, p_i - offset_i.
        # Set up at the end of __init__ (_obstacle_setup), when the context and the storage order exist.
        self._obst_set, self._obst_margin, self._obst = obstacle_watch, float(obstacle_margin), None
        # Obstacle scenes: obstacle_watch= and vision_scene= also take an ObstacleScenes, K scenes of up to G placements of one
        # prototype set, with obstacle_scene_id [N] (ints, the caller's numbering; required with scenes, refused without): drone i
        # is watched against, and sees, the placements of scene obstacle_scene_id[i] in the frame p_i - offset_i, an id outside
        # [0, K) meaning no obstacles.  `nearest` and seg then hold the instance-major body index g n_bodies + body.  Two deliberate
        # cuts: the swept watch and the other drones in the images are not implemented on scenes (the unplaced forms are).
        from ..obstacles import ObstacleScenes
        # gate_watch=Aperture: every launch is followed, on the env's stream, by one dsim_gate_passage: the chord from the position
        # the previous query saw (reset() primes it) to the state the launch left, against the aperture at every placement of each
        # drone's scene.  gate_scenes: the ObstacleScenes whose placements are the gates (None: the ObstacleScenes of obstacle_watch,
        # and its device object); obstacle_scene_id and obstacle_offsets are shared either way.  A plain world common to all drones
        # is a scenes object of K = 1 with every id 0.  gate_start: the slot due first (every drone; a course that starts AT gate 0
        # has s0 = 0 there, which is no forward crossing, so it starts at 1).  gate_laps: at the end of a scene's gates the course
        # starts again and gate_laps counts.  gate_travel [m]: the longest chord that is a passage (None: 10 m/s x one Env.step); a
        # longer one is a reset and is counted by gate_unswept().  On a sharded fleet it works per rank: nothing of the other
        # ranks' drones is needed.  Off by default: nothing is allocated or launched.
        from ..obstacles import Aperture
        if gate_watch is None:
            if gate_scenes is not None or gate_start != 0 or gate_laps or gate_travel is not None:
                raise ValueError("gate_scenes / gate_start / gate_laps / gate_travel without gate_watch=Aperture")
        else:
            if not isinstance(gate_watch, Aperture):
                raise ValueError("gate_watch takes an obstacles.Aperture")
            world = gate_scenes if gate_scenes is not None else obstacle_watch
            if not isinstance(world, ObstacleScenes):
                raise ValueError("gate_watch needs the gates' placements: gate_scenes=ObstacleScenes, or obstacle_watch=ObstacleScenes "
                                 "to share")
            if not 0 <= int(gate_start) <= world.G:
                raise ValueError(f"gate_start must be a slot in 0 .. {world.G}")
        self._gate_ap, self._gate_scenes, self._gate_start, self._gate_wrap = gate_watch, gate_scenes, int(gate_start), bool(gate_laps)
        self._gate_travel = 10.0 * int(aggregate_phy_steps) / float(freq) if gate_travel is None else float(gate_travel)
        if gate_watch is not None and (not np.isfinite(self._gate_travel) or not self._gate_travel >= 1e-3):
            raise ValueError("gate_travel must be at least a millimetre")
        placed = [x for x in (obstacle_watch, vision_scene, range_scene, gate_scenes, neighbor_sight_scene) if isinstance(x, ObstacleScenes)]
        if placed and obstacle_scene_id is None:
            raise ValueError("obstacle_scene_id [N] is required with an ObstacleScenes")
        if not placed and obstacle_scene_id is not None:
            raise ValueError("obstacle_scene_id without an ObstacleScenes (obstacle_watch=, vision_scene=, range_scene=, gate_scenes= or "
                             "neighbor_sight_scene=)")
        if placed:
            ids = np.asarray(obstacle_scene_id)
            if ids.shape != (num_drones,) or not np.issubdtype(ids.dtype, np.integer):
                raise ValueError(f"obstacle_scene_id must be [{num_drones}] ints")
            if isinstance(obstacle_watch, ObstacleScenes) and obstacle_sweep:
                raise NotImplementedError("obstacle_sweep=True with an ObstacleScenes: the swept watch on scenes is a follow-up, "
                                          "the chord in the placement's frame (both ends through R^T (q - t))")
            if vision_attributes and vision_see_drones and isinstance(obstacle_watch if vision_scene is None else vision_scene,
                                                                      ObstacleScenes):
                raise NotImplementedError("vision_see_drones=True with an ObstacleScenes: the other drones in placed images are a "
                                          "follow-up (there is no placed dsim_depth_image_drones)")
        self._scene_ids = obstacle_scene_id
        # obstacle_motion=SceneMotion (made for the ObstacleScenes of obstacle_watch): the watch's world moves.  The env owns a device
        # clock of Env.steps since reset(); every launch first advances it, then one dsim_scenes_move puts the table to scene time
        # clock x (one Env.step) on the env's stream, then the watches run: the world stands where it is at the time of the state
        # they see.  reset() returns it to scene time 0.  The camera, the scanner and line of sight see the motion when they share
        # the watch's device scenes (the default); with a vision_scene=, range_scene= or neighbor_sight_scene= of their own they
        # look at a static copy.  A captured sequence captures both calls, and a replay reads the clock from the device.  On a
        # sharded fleet every rank moves its own copy.  scene_time() and scene_placements() report it.  Off by default: nothing
        # new is allocated or launched.
        if obstacle_motion is not None:
            from ..obstacles import SceneMotion
            if not isinstance(obstacle_motion, SceneMotion):
                raise ValueError("obstacle_motion takes an obstacles.SceneMotion")
            if not isinstance(obstacle_watch, ObstacleScenes) or obstacle_motion.scenes is not obstacle_watch:
                raise ValueError("obstacle_motion must be made for the ObstacleScenes given as obstacle_watch")
            if gate_watch is not None and (gate_scenes is None or gate_scenes is obstacle_watch):
                raise NotImplementedError("gate_watch on the scenes obstacle_motion moves: a passage through a moving opening needs "
                                          "the chord's start in the pose of the PREVIOUS query, a change to k_gate_passage and a "
                                          "follow-up (gate_scenes= of their own stay static and work)")
        self._motion = obstacle_motion
        # obstacle_sweep=True: the query behind a launch is dsim_obstacle_sweep instead, the chord from the position the previous
        # query saw (reset() primes it) to the state the launch left, as a sphere of radius R + obstacle_sweep_sag swept along it:
        # with sag >= obstacles.sweep_sag(a_max, time between two queries) every sub-step state in between lies in the tested
        # volume.  obstacle_sweep_travel [m]: the chord length one cell lookup serves (None: 10 m/s x one Env.step); it sizes the
        # device set's reach and decides speed only.  Off by default: nothing new is allocated or launched.
        if obstacle_sweep and obstacle_watch is None:
            raise ValueError("obstacle_sweep=True without obstacle_watch=ObstacleSet")
        if not obstacle_sweep and (obstacle_sweep_sag != 0.0 or obstacle_sweep_travel is not None):
            raise ValueError("obstacle_sweep_sag / obstacle_sweep_travel without obstacle_sweep=True")
        self._obst_sweep, self._obst_sag = bool(obstacle_sweep), float(obstacle_sweep_sag)
        self._obst_travel = 10.0 * int(aggregate_phy_steps) / float(freq) if obstacle_sweep_travel is None else float(obstacle_sweep_travel)
        if obstacle_sweep and (not np.isfinite(self._obst_sag) or self._obst_sag < 0.0):
            raise ValueError("obstacle_sweep_sag must be >= 0")
        if obstacle_sweep and (not np.isfinite(self._obst_travel) or not self._obst_travel >= 1e-3):
            raise ValueError("obstacle_sweep_travel must be at least a millimetre")
        # obstacle_witness="world" | "body": the query behind a launch is dsim_obstacle_witness (_scenes) instead of the point
        # query — one launch, not two: the same clearance, nearest and counters, and beside them the vector from every drone's
        # query point to the closest point of its world, in world axes or in the drone's body axes.  last_obstacle_witness holds
        # it [3, N] in the caller's numbering (zeros for a drone with nothing within the margin; None before the first step),
        # obstacle_witness() asks on demand.  On a sharded fleet it works per rank: nothing of the other ranks' drones is needed.
        # Off by default: nothing new is allocated or launched.
        if obstacle_witness is not None:
            if obstacle_witness not in ("world", "body"):
                raise ValueError(f"obstacle_witness must be None, 'world' or 'body', got {obstacle_witness!r}")
            if obstacle_watch is None:
                raise ValueError("obstacle_witness without obstacle_watch=ObstacleSet (or ObstacleScenes)")
            if obstacle_sweep:
                raise NotImplementedError("obstacle_witness with obstacle_sweep=True: the witness of a chord is another quantity "
                                          "(the closest pair of a segment and the set, and where on the chord it lies)")
        self._obst_wit = obstacle_witness
        # obstacle_witness_velocity=True (with obstacle_witness and obstacle_motion): every launch moves the world with its twist
        # (dsim_scenes_move_twist) and the query behind it is dsim_obstacle_witness_scenes_vel — still one watch launch: the same
        # clearance, nearest, witness and counters, and beside them the velocity of every drone's closest obstacle point as a
        # material point of the moving placement that holds it, in the witness's axes.  last_obstacle_witness_velocity holds it
        # [3, N] in the caller's numbering (None before the first step), obstacle_witness_velocity() asks on demand,
        # scene_twists() reports the table.  The obstacle's own velocity, not the relative one: h' = n . (v_drone - v_obstacle)
        # is the caller's to form.  Off by default: nothing new is allocated or launched.
        if obstacle_witness_velocity:
            if obstacle_witness is None:
                raise ValueError("obstacle_witness_velocity without obstacle_witness='world' or 'body'")
            if obstacle_motion is None:
                raise ValueError("obstacle_witness_velocity without obstacle_motion=SceneMotion: a static world's points stand still")
        self._wit_vel = bool(obstacle_witness_velocity)
        # obstacle_witnesses=m (1..8, with obstacle_witness): the query behind a launch is dsim_obstacle_witnesses (_scenes) in the
        # witness's place — still one watch launch: per drone the m closest BODIES within the margin, sorted, each with its
        # clearance, its vector and (with obstacle_witness_velocity) its velocity.  last_obstacle_witnesses holds the record in the
        # caller's numbering (None before the first step), obstacle_witnesses() asks on demand.  Slot 0 is the witness bit for
        # bit: last_obstacle_clearance, last_obstacle_witness, last_obstacle_witness_velocity and obstacle_contacts() read row 0
        # of the new buffers and keep their values.  0 by default: nothing new is allocated or launched.
        if isinstance(obstacle_witnesses, bool) or not isinstance(obstacle_witnesses, (int, np.integer)) \
                or not 0 <= int(obstacle_witnesses) <= nat.WITNESSES_MAX:
            raise ValueError(f"obstacle_witnesses must be an int in 0..{nat.WITNESSES_MAX}, got {obstacle_witnesses!r}")
        if obstacle_witnesses and obstacle_witness is None:
            raise ValueError("obstacle_witnesses without obstacle_witness='world' or 'body'")
        self._obst_m = int(obstacle_witnesses)
        # velocity_filter=dict(alpha=..., buffer_drone=0, buffer_obstacle=0, share=0.5, floor=None): the consumer of the records
        # above.  filter_velocity(u) turns a wished velocity [3, N] into the closest one that meets the control-barrier rows of
        # every drone's floor, obstacle witnesses (obstacle_witnesses=m with obstacle_witness="world"; their velocities with
        # obstacle_witness_velocity=True) and neighbours (neighbor_obs=k with the relative velocities), in one dsim_velocity_filter
        # on the storage-order records the env keeps behind each launch; last_filter_dropped says which rows could not be kept,
        # filter_counts() how many drones were changed and how many lost a row; VelocityAviary.step_velocity(u) filters, encodes
        # and steps.  It runs when asked, outside the launch: a captured sequence neither captures nor refuses it.  On a sharded
        # fleet it works with the witnesses alone.  None by default: nothing is allocated or launched.
        if velocity_filter is not None:
            from ..avoid import check_options
            if not isinstance(velocity_filter, dict) or "alpha" not in velocity_filter:
                raise ValueError("velocity_filter takes a dict(alpha=..., buffer_drone=, buffer_obstacle=, share=, floor=)")
            unknown = set(velocity_filter) - {"alpha", "buffer_drone", "buffer_obstacle", "share", "floor"}
            if unknown:
                raise ValueError(f"velocity_filter: unknown keys {sorted(unknown)}")
            opts = check_options(**velocity_filter)
            if obstacle_witness == "body":
                raise ValueError("velocity_filter needs the witnesses in world axes: obstacle_witness='world', not 'body'")
            if neighbor_obs is not None and neighbor_vel is False:
                raise ValueError("velocity_filter needs the neighbours' relative velocities: neighbor_vel=False leaves them out")
            if neighbor_obs is None and not obstacle_witnesses:
                raise ValueError("velocity_filter needs a source of rows: neighbor_obs=k (with neighbor_vel) or obstacle_witnesses=m "
                                 "with obstacle_witness='world'")
            self._filter_opts = dict(zip(("alpha", "buffer_drone", "buffer_obstacle", "share", "floor"), opts))
        # BaseAviary(vision_attributes=True) keeps self.rgb / self.dep / self.seg per drone at IMG_RES = [64, 48] and refreshes them
        # from _getDroneImages whenever step_counter % IMG_CAPTURE_FREQ == 0 (BaseAviary.py:236-261, 453-502, 794-853).  Here:
        # env.dep / env.seg ([n, H, W] device tensors; no rgb) of the static world `vision_scene` (default: the obstacle_watch
        # set, whose device copy the camera then shares), captured on the env's stream behind the step the cadence names; a
        # step_fused launch with n_steps > 1 captures once, at its end, when a capture fell due inside it.  vision_drones: the
        # drones that carry a camera (the caller's numbering; None: all).  The set lies in the frame of obstacle_offsets.  The
        # other drones are not drawn unless vision_see_drones=True (vision_drones already says who carries a camera): then every
        # other drone appears in dep and seg as its bounding sphere, up to vision_drone_range metres (None: the far plane), seg
        # naming drone k of the caller's numbering as -3 - k (DepthCamera.seg_drone); the camera's own drone is never drawn, and
        # vision_scene becomes optional (a world of drones and the plane).  Checked here, set up at the end of __init__
        # (_vision_setup).
        if vision_see_drones and dist is not None and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("vision_see_drones on a sharded fleet: the radii of the other ranks' drones would have to "
                                      "travel with their positions (dsim_depth_image_drones takes pos_all / radius_all)")
        if (vision_see_drones or vision_drone_range is not None) and not vision_attributes:
            raise ValueError("vision_see_drones / vision_drone_range without vision_attributes=True")
        if vision_drone_range is not None and not vision_see_drones:
            raise ValueError("vision_drone_range without vision_see_drones=True")
        if vision_drone_range is not None and not float(vision_drone_range) > 0.0:
            raise ValueError("vision_drone_range must be positive")
        self._vision_args = None
        if vision_attributes:
            self.IMG_RES = np.array([int(vision_res[0]), int(vision_res[1])])
            self.IMG_FRAME_PER_SEC = 24
            self.IMG_CAPTURE_FREQ = int(freq) // self.IMG_FRAME_PER_SEC
            if self.IMG_CAPTURE_FREQ < 1 or self.IMG_CAPTURE_FREQ % int(aggregate_phy_steps) != 0:
                raise ValueError(f"aggregate_phy_steps = {aggregate_phy_steps} is incompatible with the image capture rate of "
                                 f"{self.IMG_FRAME_PER_SEC} Hz at freq = {freq}: IMG_CAPTURE_FREQ = {self.IMG_CAPTURE_FREQ} physics "
                                 "steps must be a positive multiple of it (BaseAviary.py:247-253)")
            if not (1 <= self.IMG_RES[0] <= 1024 and 1 <= self.IMG_RES[1] <= 1024):
                raise ValueError(f"vision_res must be (width, height) with 1 <= each <= 1024, got {vision_res!r}")
            if vision_scene is None and obstacle_watch is None and not vision_see_drones:
                raise ValueError("vision_attributes=True needs a world to look at: vision_scene=ObstacleSet (or obstacle_watch)")
            if vision_drones is not None:
                vd = np.asarray(vision_drones, dtype=np.int64).ravel()
                if vd.size < 1 or vd.min() < 0 or vd.max() >= num_drones:
                    raise ValueError(f"vision_drones must name drones in [0, {num_drones})")
            self._vision_args = (vision_scene, vision_drones, bool(vision_ground), bool(vision_see_drones), vision_drone_range)
        elif vision_scene is not None or vision_drones is not None:
            raise ValueError("vision_scene / vision_drones without vision_attributes=True")
        # range_scan=beams [B, 3] (body frame; RangeScanner.fan(...) builds the usual tables): every drone carries that fan of
        # range beams, cast behind every launch, on the env's stream, against range_scene (default: the obstacle_watch world,
        # whose device set the scanner then shares; an ObstacleScenes goes by obstacle_scene_id), the plane z = 0 (range_ground)
        # and, with range_see_drones=True, the other drones as their bounding spheres up to range_drone_range metres (None:
        # range_max).  env.ranges / env.range_hits [B, N] hold the last scan in the caller's numbering (None before the first
        # step); a beam reports hits with range_min <= t <= range_max, a miss +inf or, with range_clamp, range_max.  The world
        # lies in the frame of obstacle_offsets.  Off by default: nothing is allocated or launched.
        self._scan_args = None
        self._scan_sampled = False
        if range_scan is None:
            if (range_scene is not None or range_min != 0.0 or range_max != 10.0 or range_ground is not True or range_clamp
                    or range_see_drones or range_drone_range is not None):
                raise ValueError("range_scene / range_min / range_max / range_ground / range_clamp / range_see_drones / "
                                 "range_drone_range without range_scan=beams")
        else:
            from ..scanner import check_range, unit_beams
            beams = unit_beams(range_scan)
            check_range(range_min, range_max)
            if range_see_drones and dist is not None and dist.is_initialized() and dist.get_world_size() > 1:
                raise NotImplementedError("range_see_drones on a sharded fleet: the radii of the other ranks' drones would have to "
                                          "travel with their positions (dsim_depth_image_drones takes pos_all / radius_all)")
            if range_drone_range is not None and not range_see_drones:
                raise ValueError("range_drone_range without range_see_drones=True")
            if range_drone_range is not None and not float(range_drone_range) > 0.0:
                raise ValueError("range_drone_range must be positive")
            if range_scene is None and obstacle_watch is None and not range_see_drones and not range_ground:
                raise ValueError("range_scan needs a world to range against: range_scene=ObstacleSet (or obstacle_watch), "
                                 "range_ground=True or range_see_drones=True")
            self._scan_args = (beams, range_scene, float(range_min), float(range_max), bool(range_ground), bool(range_clamp),
                               bool(range_see_drones), range_drone_range)
        # corridor=dict(k, piece, sag=0.0, margin=None, ground=False): the planner's question, on demand.  corridor_clearance(rel)
        # gives, for k candidate segments per drone, the clearance of its bounding sphere (+ sag) swept along each
        # (dsim_corridor_clearance) against the obstacle_watch world where it stands now — the watch's device set or scenes, its
        # obstacle_offsets and obstacle_scene_id, so it sees obstacle_motion — and, with ground, the half-space z <= 0.  piece [m]:
        # the length one cell lookup serves; the shared set is made with the larger of the watch's reach and
        # corridor_reach(types, margin, sag, piece), and a segment of up to 32 pieces is served (corridor_unserved() counts the
        # others).  margin None: obstacle_margin.  It runs when asked, outside the launch: a captured sequence neither captures nor
        # refuses it, and it needs nothing of other ranks.  None by default: nothing is allocated or launched, and the set keeps
        # the reach it has without it.
        if corridor is not None:
            if not isinstance(corridor, dict) or "k" not in corridor or "piece" not in corridor:
                raise ValueError("corridor takes a dict(k=..., piece=..., sag=0.0, margin=None, ground=False)")
            unknown = set(corridor) - {"k", "piece", "sag", "margin", "ground"}
            if unknown:
                raise ValueError(f"corridor: unknown keys {sorted(unknown)}")
            if obstacle_watch is None:
                raise ValueError("corridor without obstacle_watch=ObstacleSet (or ObstacleScenes)")
            k, piece, sag = corridor["k"], corridor["piece"], corridor.get("sag", 0.0)
            margin = corridor.get("margin")
            if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= nat.CORRIDOR_MAX_K:
                raise ValueError(f"corridor: k must be a whole number of slots in 1 .. {nat.CORRIDOR_MAX_K}")
            if isinstance(piece, bool) or not np.isfinite(float(piece)) or not float(piece) >= 1e-3:
                raise ValueError("corridor: piece must be at least a millimetre")
            if isinstance(sag, bool) or not np.isfinite(float(sag)) or float(sag) < 0.0:
                raise ValueError("corridor: sag must be >= 0")
            margin = float(obstacle_margin) if margin is None else float(margin)
            if not (np.isfinite(margin) and margin > 0.0):
                raise ValueError("corridor: margin must be positive")
            self._corr_opts = dict(k=int(k), piece=float(piece), sag=float(sag), margin=margin, ground=bool(corridor.get("ground", False)))

    def _watch_setup(self, offsets) -> None:
        """At the end of __init__: the obstacle set first, because the camera shares its device set."""
        if self._drone_sweep:
            # where the previous query saw every drone (storage order), and how many drone x queries were point samples
            dev, n_pad = self.ctx.device, self.state.n_pad
            self._drone_prev = torch.zeros((3, n_pad), dtype=torch.float32, device=dev)
            self._drone_unswept = torch.zeros((1,), dtype=torch.int64, device=dev)
            self._drone_grid().clearance_prime(self._drone_prev)     # (the first _housekeeping ran before this tensor existed)
        if self._knn_k:
            # what the query behind every launch writes (storage order, fixed addresses)
            from ..downwash import Neighbors
            dev, n_pad, k = self.ctx.device, self.state.n_pad, self._knn_k
            f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
            self._knn_out = Neighbors(torch.full((k, n_pad), -1, dtype=torch.int32, device=dev), f32(k, n_pad), f32(k, 3, n_pad),
                                      f32(k, 3, n_pad) if self._knn_vel else None,
                                      torch.zeros((n_pad,), dtype=torch.int32, device=dev))
        self._obstacle_setup(offsets)
        self._vision_setup(offsets)
        self._scan_setup(offsets)
        self._gate_setup(offsets)
        self._sight_setup(offsets)
        self._filter_setup(offsets)
        self._corridor_setup(offsets)

    def _corridor_setup(self, offsets) -> None:
        """corridor=dict(...): the Corridor on the watch's device world, and the tensors every call reads (storage order, fixed
        addresses)."""
        if self._corr_opts is None:
            return
        from ..corridor import Corridor
        c = self._corr_opts
        dev, n_pad, k = self.ctx.device, self.state.n_pad, c["k"]
        self._corr = Corridor(self.ctx, self.state, self._obst, k, c["margin"], sag=c["sag"], ground=c["ground"], offsets=offsets,
                              scene_id=self._scene_ids if self._obst_placed else None, type_id=self._type_id)
        self._corr_rel = torch.zeros((k, 3, n_pad), dtype=torch.float32, device=dev)
        self._corr_index = torch.full((k, n_pad), -1, dtype=torch.int32, device=dev)

    def _filter_setup(self, offsets) -> None:
        """velocity_filter=dict(...): the VelocityFilter and the tensors every call reads and writes (storage order, fixed addresses)."""
        if self._filter_opts is None:
            return
        from ..avoid import Filtered, VelocityFilter
        dev, n_pad = self.ctx.device, self.state.n_pad
        self._filter = VelocityFilter(self.ctx, self.state, offsets=offsets, type_id=self._type_id, **self._filter_opts)
        self._filter_u = torch.zeros((3, n_pad), dtype=torch.float32, device=dev)
        self._filter_out = Filtered(torch.zeros((3, n_pad), dtype=torch.float32, device=dev),
                                    torch.zeros((n_pad,), dtype=torch.int32, device=dev))
        self._filter_wits = None      # the on-demand witnesses of a call before the first step
        self._filter_fresh = self._filter_sampled = False

    def _obstacle_setup(self, offsets) -> None:
        """obstacle_watch: the device set for reach = R_max + margin, the offsets in storage order and the tensors every
        per-step query writes (fixed addresses: a captured sequence holds them)."""
        if self._obst_set is None:
            if offsets is not None and self._vision_args is None and self._scan_args is None and self._gate_ap is None and not self._sight_on:
                raise ValueError("obstacle_offsets without obstacle_watch")
            return
        from .. import obstacles as obs
        if not isinstance(self._obst_set, (obs.ObstacleSet, obs.ObstacleScenes)):
            raise TypeError("obstacle_watch takes an ObstacleSet or an ObstacleScenes")
        self._obst_placed = isinstance(self._obst_set, obs.ObstacleScenes)
        if not self._obst_margin > 0.0:
            raise ValueError("obstacle_margin must be positive")
        dev, n_pad = self.ctx.device, self.state.n_pad
        self._obst_off = None
        if offsets is not None:
            offsets = np.asarray(offsets, dtype=np.float64)
            if offsets.shape != (self.NUM_DRONES, 3):
                raise ValueError(f"obstacle_offsets must be [{self.NUM_DRONES}, 3]")
            self._obst_off = self._soa3(offsets)
        reach = (obs.sweep_reach(self.ctx.types, self._obst_margin, self._obst_sag, self._obst_travel) if self._obst_sweep
                 else obs.watch_reach(self.ctx.types, self._obst_margin))
        if self._corr_opts is not None:              # (the corridor's pieces need their half cell: results of the watches do not depend on reach)
            c = self._corr_opts
            reach = max(reach, obs.corridor_reach(self.ctx.types, c["margin"], c["sag"], c["piece"]))
        self._obst = self._obst_set.to_device(self.ctx, reach)
        # the scene of every drone in storage order (a type-major fleet and a sharded rank's slice see their own ids)
        self._obst_ids = (obs.scene_ids_tensor(self._scene_ids, self.NUM_DRONES, n_pad, dev, self.order) if self._obst_placed
                          else None)
        self._obst_clr = torch.empty((n_pad,), dtype=torch.float32, device=dev)
        self._obst_near = torch.empty((n_pad,), dtype=torch.int32, device=dev)
        self._obst_on_demand = torch.zeros((1,), dtype=torch.int64, device=dev)    # what on-demand queries counted
        self._obst_sampled = False
        # the witness behind every launch (storage order, fixed address: a captured sequence holds it)
        self._obst_rel = torch.zeros((3, n_pad), dtype=torch.float32, device=dev) if self._obst_wit is not None else None
        m = self._obst_m
        if m:
            # the witnesses behind every launch, slot-major; the single answers are row 0 of them (the same fixed addresses)
            from ..obstacles import ObstacleWitnesses
            self._obst_wits = ObstacleWitnesses(torch.empty((m, n_pad), dtype=torch.float32, device=dev),
                                                torch.empty((m, n_pad), dtype=torch.int32, device=dev),
                                                torch.zeros((m, 3, n_pad), dtype=torch.float32, device=dev), None,
                                                torch.zeros((n_pad,), dtype=torch.int32, device=dev))
            self._obst_clr, self._obst_near, self._obst_rel = self._obst_wits.clearance[0], self._obst_wits.body[0], self._obst_wits.rel[0]
        if self._motion is not None:
            # the scene clock (fixed address: a captured sequence holds it) and the motion's device copy; the table to scene time 0
            self._scene_clock = torch.zeros((1,), dtype=torch.int64, device=dev)
            if self._wit_vel:
                # the twist table every move then writes, and the velocity behind every launch (storage order, fixed addresses)
                self._obst.enable_twist()
                self._obst_vel = torch.zeros((3, n_pad), dtype=torch.float32, device=dev)
                if m:
                    self._obst_wits = self._obst_wits._replace(vel=torch.zeros((m, 3, n_pad), dtype=torch.float32, device=dev))
                    self._obst_vel = self._obst_wits.vel[0]
            self._obst.set_motion(self._motion)
            self._obst.move(self._scene_clock, self._scene_dt())
        if self._obst_sweep:
            # where the previous query saw every drone (storage order, fixed address: a captured sequence holds it), and how many
            # drone x queries were point samples because they had no usable chord
            self._obst_prev = torch.zeros((3, n_pad), dtype=torch.float32, device=dev)
            self._obst_unswept = torch.zeros((1,), dtype=torch.int64, device=dev)
            self._watch_placed()

    def _vision_setup(self, offsets) -> None:
        """vision_attributes=True: the camera, its device set (shared with the obstacle watch when both look at the same
        ObstacleSet) and env.dep / env.seg."""
        if self._vision_args is None:
            return
        from ..camera import DepthCamera
        scene, drones, ground, see_drones, drone_range = self._vision_args
        shared = self._obst is not None and (scene is None or scene is self._obst_set)
        from ..obstacles import DeviceScenes, ObstacleScenes
        world = self._obst if shared else scene
        self._vision = DepthCamera(self.ctx, self.state, world, res=tuple(int(v) for v in self.IMG_RES),
                                   ground=ground, cameras=drones, offsets=offsets, type_id=self._type_id, drones=see_drones,
                                   drone_range=drone_range,
                                   scene_id=self._scene_ids if isinstance(world, (ObstacleScenes, DeviceScenes)) else None)
        self.dep, self.seg = self._vision.dep, self._vision.seg
        self.dep.fill_(1.0)                # nothing seen yet (BaseAviary.py:245 starts from ones too)
        self.seg.fill_(-1)

    def _scan_setup(self, offsets) -> None:
        """range_scan=beams: the scanner and its device set (shared with the obstacle watch when both look at the same world)."""
        if self._scan_args is None:
            return
        from ..obstacles import DeviceScenes, ObstacleScenes
        from ..scanner import RangeScanner
        beams, scene, t_min, t_max, ground, clamp, see_drones, drone_range = self._scan_args
        shared = self._obst is not None and (scene is None or scene is self._obst_set)
        world = self._obst if shared else scene
        self._scan = RangeScanner(self.ctx, self.state, world, beams, t_min=t_min, t_max=t_max, ground=ground, clamp=clamp,
                                  offsets=offsets, type_id=self._type_id, drones=see_drones, drone_range=drone_range,
                                  scene_id=self._scene_ids if isinstance(world, (ObstacleScenes, DeviceScenes)) else None)

    def _sight_setup(self, offsets) -> None:
        """neighbor_sight=True: the LineOfSight and its device set (shared with the obstacle watch when both look at the same world)."""
        if not self._sight_on:
            return
        scene = self._sight_scene
        shared = self._obst is not None and (scene is None or scene is self._obst_set)
        self._sight_offsets = offsets
        self._sight = self._sight_make(self._obst if shared else scene, self._knn_k)
        self._sight_demand = {}

    def _sight_make(self, world, k: int):
        from ..obstacles import DeviceScenes, ObstacleScenes
        from ..sight import LineOfSight
        # (one DroneTargets — one grid, one workspace, one outside count — serves the per-launch object and the on-demand ones)
        return LineOfSight(self.ctx, self.state, world, k, offsets=self._sight_offsets,
                           scene_id=self._scene_ids if isinstance(world, (ObstacleScenes, DeviceScenes)) else None,
                           drones=self._sight_drones, drone_box=self._sight_box, type_id=self._type_id if self._sight_drones else None,
                           targets=self._sight._targets if self._sight is not None else None)

    def _sight_query(self, sight, rel, index):
        """One query of ``sight`` on a record in storage order, on the env's stream."""
        if sight.drones and self._downwash is not None:
            self._downwash.invalidate_prebin()            # the drones' binning drops the ctx's grid bookkeeping
        return sight.query(rel, index)

    def _sight_caller(self, s):
        """A Sight in storage order in the caller's numbering on the drone axis (the drone axis only: a drone that blocks is
        already named in the caller's numbering, through the label table of the query)."""
        if self.order is None:
            return s
        from ..sight import Sight
        to = self.order.to_caller
        return Sight(*(to(t, 1) if t is not None else None for t in s))

    def _gate_setup(self, offsets) -> None:
        """gate_watch=Aperture: the device scenes (the obstacle watch's when the gates are its placements), ids and offsets in
        storage order, and the tensors every query reads and writes (fixed addresses: a captured sequence holds them)."""
        if self._gate_ap is None:
            return
        from .. import obstacles as obs
        dev, n_pad = self.ctx.device, self.state.n_pad
        self._gate_shared = self._obst is not None and self._obst_placed and (self._gate_scenes is None
                                                                             or self._gate_scenes is self._obst_set)
        if self._gate_shared:
            self._gate, self._gate_ids, self._gate_off = self._obst, self._obst_ids, self._obst_off
        else:
            # (the watch looks at placements only: the prototype's grid is made for the least reach the point watch would take)
            self._gate = self._gate_scenes.to_device(self.ctx, obs.watch_reach(self.ctx.types, 1.0))
            self._gate_ids = obs.scene_ids_tensor(self._scene_ids, self.NUM_DRONES, n_pad, dev, self.order)
            self._gate_off = None
            if offsets is not None:
                offsets = np.asarray(offsets, dtype=np.float64)
                if offsets.shape != (self.NUM_DRONES, 3):
                    raise ValueError(f"obstacle_offsets must be [{self.NUM_DRONES}, 3]")
                self._gate_off = self._soa3(offsets)
        i32 = lambda: torch.zeros((n_pad,), dtype=torch.int32, device=dev)
        self._gate_prev = torch.zeros((3, n_pad), dtype=torch.float32, device=dev)
        self._gate_due, self._gate_lap = i32(), i32()
        self._gate_time = torch.full((self._gate.G, n_pad), float("nan"), dtype=torch.float64, device=dev)
        self._gate_fwd, self._gate_back, self._gate_miss = i32(), i32(), i32()
        self._gate_clock = torch.zeros((1,), dtype=torch.int64, device=dev)      # queries so far: the whole part of a passage time
        self._gate_counts = torch.zeros((5,), dtype=torch.int64, device=dev)     # passes, wrong way, out of order, misses, unswept
        self._gate_sampled = False
        self._watch_placed()

    def _watch_gates(self, scratch: bool = False) -> None:
        """One dsim_gate_passage on the state the launch just left, on the env's stream (also under capture), then the clock moves
        on by one query.  ``scratch``: the eager call before a capture — a look ahead: prev and the course stay, events and counts go to copies."""
        from .. import obstacles as obs
        c = self._gate_counts
        if scratch:
            c = torch.zeros_like(c)
            obs.gate_passage(self.ctx, self.state, self._gate, self._gate_ids, self._gate_ap, self._gate_travel, self._gate_prev,
                             self._gate_due, self._gate_lap, self._gate_clock, self._gate_time,
                             torch.zeros_like(self._gate_fwd), None, None, self._gate_off, c[0:1], c[1:2], c[2:3], c[3:4], c[4:5],
                             wrap=self._gate_wrap, keep_prev=True)
            return
        obs.gate_passage(self.ctx, self.state, self._gate, self._gate_ids, self._gate_ap, self._gate_travel, self._gate_prev,
                         self._gate_due, self._gate_lap, self._gate_clock, self._gate_time, self._gate_fwd, self._gate_back,
                         self._gate_miss, self._gate_off, c[0:1], c[1:2], c[2:3], c[3:4], c[4:5], wrap=self._gate_wrap)
        nat.check(self.ctx.lib.dsim_counter_add(self.ctx.handle, self.ctx.stream_ptr(), self._gate_clock.data_ptr(), 1))
        self._gate_sampled = True

    def _watch_reset(self) -> None:
        """_housekeeping: the step counter is back at zero, and so is the last one the camera's cadence saw."""
        self._vision_seen = 0

    def _watch_placed(self) -> None:
        """_housekeeping placed every drone: the swept watch's chords start there (the first step is swept from the start)."""
        self._filter_fresh = False         # (the records behind the last launch describe a state that is gone)
        if self._obst is not None and self._obst_sweep:
            from .. import obstacles as obs
            obs.prime(self.ctx, self.state, self._obst, self._obst_prev)
        if self._drone_prev is not None:
            self._drone_grid().clearance_prime(self._drone_prev)
        if self._scene_clock is not None:
            # the world starts again: scene time 0
            self._scene_clock.zero_()
            self._obst.move(self._scene_clock, self._scene_dt())
        if self._gate is not None:
            # every course starts again: the chords from here, gate_start due, no lap, no passage time, the clock at zero
            from .. import obstacles as obs
            obs.gate_prime(self.ctx, self.state, self._gate_prev)
            self._gate_due.fill_(self._gate_start)
            self._gate_lap.zero_()
            self._gate_time.fill_(float("nan"))
            self._gate_clock.zero_()
            for t in (self._gate_fwd, self._gate_back, self._gate_miss):
                t.zero_()
            self._gate_sampled = False

    def _watch_close(self) -> None:
        if self._vision is not None:
            self._vision.close()
        if self._scan is not None:
            self._scan.close()
        if self._sight is not None:
            self._sight.close()
        if self._gate is not None and not self._gate_shared:
            self._gate.close()
        if self._corr is not None:
            self._corr.close()
        if self._obst is not None:
            self._obst.close()

    # ------------------------------------------------------------------ behind a step
    def _stepped(self, n_steps: int = 1) -> None:
        """The epilogue of every launch of ``n_steps`` Env.steps (step, step_fused and the adaptor envs' step, fresh or from a
        prepared plan): the counters move on, then the watches run on the state the launch just left and on the env's stream:
        one dsim_clearance with drone_watch=True, one dsim_obstacle_clearance with obstacle_watch, the camera when it is due."""
        self.step_counter += self.AGGR_PHY_STEPS * n_steps
        self._env_steps += n_steps
        if self._scene_clock is not None:
            self._scene_move(n_steps)          # (first: every watch below sees the world at the time of the state it looks at)
        if self._drone_watch:
            self.last_clearance = self._drone_query(self._drone_watch_margin, None, self._drone_sweep)
        if self._knn_k:
            self.last_neighbors = self._neighbor_query(self._knn_k, self._knn_radius, self._knn_vel, self._knn_out)
            if self._sight is not None:
                # (on the record the query just wrote, in storage order: the vectors last_neighbors reports, bit for bit)
                self.last_neighbor_sight = self._sight_caller(self._sight_query(self._sight, self._knn_out.rel_pos, self._knn_out.index))
        if self._obst is not None:
            self._watch_obstacles()
        if self._vision is not None:
            # due when a multiple of IMG_CAPTURE_FREQ lies in (the counter before the launch, the counter now]: for a launch of
            # one Env.step that is step_counter % IMG_CAPTURE_FREQ == 0 (BaseAviary.py:483)
            f = self.IMG_CAPTURE_FREQ
            due = self.step_counter // f > self._vision_seen // f
            self._vision_seen = self.step_counter
            if due:
                self._vision_capture()
        if self._scan is not None:
            self._scan_now()
        if self._gate is not None:
            self._watch_gates()
        self._filter_fresh = True

    def _scene_dt(self) -> float:
        """One Env.step in seconds: the unit of the scene clock."""
        return float(self.AGGR_PHY_STEPS) / float(self.SIM_FREQ)

    def _scene_move(self, n_steps: int) -> None:
        """The scene clock moves on by ``n_steps`` Env.steps, then the watch's table to that scene time, both on the env's stream
        (also under capture: the kernel reads the clock from the device)."""
        nat.check(self.ctx.lib.dsim_counter_add(self.ctx.handle, self.ctx.stream_ptr(), self._scene_clock.data_ptr(), int(n_steps)))
        self._obst.move(self._scene_clock, self._scene_dt())

    def _drone_grid(self):
        from ..downwash import Downwash
        if self._clearance is None:
            self._clearance = Downwash(self.ctx, self.state, self._type_id, None)
        return self._clearance

    def _drone_query(self, margin: float, pairs_out, swept: bool = False):
        """The point query of the current state, or (``swept``: the watch behind a launch of a drone_sweep=True env) the swept one
        from the state the previous swept query saw."""
        dw = self._drone_grid()
        if self._downwash is not None:
            self._downwash.invalidate_prebin()            # the clearance pass re-uses the ctx's grid bookkeeping
        if swept:
            clr, near = dw.clearance_sweep(margin, self._drone_sag, self._drone_travel, self._drone_prev, pairs_out=pairs_out,
                                           unswept_out=self._drone_unswept)
        else:
            clr, near = dw.clearance(margin, pairs_out=pairs_out)
        if self.order is not None:
            clr, near = self.order.to_caller(clr, 0), self.order.indices_to_caller(near, 0)
        return clr, near

    def _neighbor_query(self, k: int, radius: float, vel: bool, out):
        """One dsim_knn on the current state, on the env's stream and a grid of its own, in the caller's numbering on both axes:
        the drone axis of every member, and the indices the lists hold."""
        return self._neighbors_caller(self._neighbor_raw(k, radius, vel, out))

    def _neighbor_raw(self, k: int, radius: float, vel: bool, out):
        """... and the record as the query wrote it, in storage order on both axes."""
        from ..downwash import Downwash
        if self._knn is None:
            self._knn = Downwash(self.ctx, self.state, self._type_id, None)
        if self._downwash is not None:
            self._downwash.invalidate_prebin()            # the query's binning re-uses the ctx's grid bookkeeping
        return self._knn.nearest(radius, k, out=out, rel_vel=vel)

    def _neighbors_caller(self, nb):
        from ..downwash import Neighbors
        if self.order is None:
            return nb
        to = self.order.to_caller
        return Neighbors(self.order.indices_to_caller(nb.index, 1), to(nb.dist, 1), to(nb.rel_pos, 2),
                         to(nb.rel_vel, 2) if nb.rel_vel is not None else None, to(nb.count, 0))

    def _watch_obstacles(self) -> None:
        """One dsim_obstacle_clearance on the state the step just left, on the env's stream (also under capture); with
        obstacle_sweep=True one dsim_obstacle_sweep from the state the previous one saw."""
        from .. import obstacles as obs
        if self._obst_sweep:
            obs.sweep(self.ctx, self.state, self._obst, self._obst_margin, self._obst_sag, self._obst_prev, self._obst_clr,
                      self._obst_near, self._obst_off, self._type_id, None, self._obst_unswept)
            self._obst_sampled = True
            return
        if self._obst_m:
            w = self._obst_wits
            self._obst_query(self._obst_margin, w.clearance, w.body, None, w.rel, self._obst_wit, w.vel, self._obst_m, w.count)
        else:
            self._obst_query(self._obst_margin, self._obst_clr, self._obst_near, None, self._obst_rel, self._obst_wit, self._obst_vel)
        self._obst_sampled = True

    def _obst_query(self, margin, clr, near, contacts_out, rel=None, frame=None, vel=None, m=None, count=None) -> None:
        """The point query of the watch's world: dsim_obstacle_clearance, or dsim_obstacle_clearance_scenes on scenes; with
        ``rel`` the witness query in its place (dsim_obstacle_witness / _scenes: the same answers and the vector beside them);
        with ``vel`` too dsim_obstacle_witness_scenes_vel; with ``m`` dsim_obstacle_witnesses (_scenes) into slot-major tensors."""
        from .. import obstacles as obs
        obs.point_query(self.ctx, self.state, self._obst, self._obst_ids, margin, clr, near, rel, self._obst_off, self._type_id,
                        contacts_out, body_frame=frame == "body", vel=vel, m=m, count=count)

    def _scan_now(self):
        """One dsim_range_scan on the state the launch just left, on the env's stream (also under capture)."""
        if self._scan.drones and self._downwash is not None:
            self._downwash.invalidate_prebin()            # the drones' binning drops the ctx's grid bookkeeping
        self._scan.scan()
        self._scan_sampled = True

    def _vision_capture(self):
        if self._vision.drones and self._downwash is not None:
            self._downwash.invalidate_prebin()            # the drones' binning drops the ctx's grid bookkeeping
        return self._vision.capture()

    # ------------------------------------------------------------------ a captured sequence (capture_fused / FusedGraph)
    def _capture_prepare(self) -> None:
        """Before the capture: what cannot be part of a graph is refused, and each service's kernel runs once eagerly."""
        if self._drone_watch:
            raise NotImplementedError("graph capture with drone_watch: the watch re-measures its grid's box on the host from "
                                      "time to time, which a captured sequence cannot")
        if self._knn_k:
            raise NotImplementedError("graph capture with neighbor_obs: the query re-measures its grid's box on the host from "
                                      "time to time, which a captured sequence cannot")
        if self._scene_clock is not None:
            # (eager: the move's kernel is loaded before the capture starts; the clock stays, so the table is rewritten as it stands)
            self._obst.move(self._scene_clock, self._scene_dt())
        if self._obst is not None:
            # (eager, not an Env.step: the watch's kernel is loaded before the capture starts)
            if self._obst_m:
                self.obstacle_witnesses()
            elif self._obst_vel is not None:
                self.obstacle_witness_velocity()
            elif self._obst_wit is not None:
                self.obstacle_witness()
            else:
                self.obstacle_clearance()
            if self._obst_sweep:          # (and the swept one's: prev stays, the contacts it counts go where on-demand ones go)
                from .. import obstacles as obs
                obs.sweep(self.ctx, self.state, self._obst, self._obst_margin, self._obst_sag, self._obst_prev,
                          torch.empty_like(self._obst_clr), None, self._obst_off, self._type_id, self._obst_on_demand, None,
                          keep_prev=True)
        if self._vision is not None:
            if self.IMG_CAPTURE_FREQ != self.AGGR_PHY_STEPS:
                raise NotImplementedError(f"graph capture with vision_attributes: the images are due every "
                                          f"{self.IMG_CAPTURE_FREQ // self.AGGR_PHY_STEPS} Env.steps, and a captured sequence is captured "
                                          "at any length; only a cadence of 1 (IMG_CAPTURE_FREQ == AGGR_PHY_STEPS) is part of the graph")
            # (eager: the camera's kernel is loaded before the capture starts; with vision_see_drones this capture also measures the
            # box of the drones' grid and makes its workspace, which stand for the whole graph)
            if self._vision.drones:
                self._vision.refresh_drone_box()
            self._vision_capture()
        if self._scan is not None:
            # (eager: the scanner's kernel is loaded before the capture starts; with range_see_drones this scan also measures the box
            # of the drones' grid and makes its workspace, which stand for the whole graph.  Not an Env.step: what env.ranges shows
            # does not change kind, it is the current state's scan)
            if self._scan.drones:
                self._scan.refresh_drone_box()
            sampled = self._scan_sampled
            self._scan_now()
            self._scan_sampled = sampled
        if self._gate is not None:
            self._watch_gates(scratch=True)   # (eager: the watch's kernel is loaded before the capture starts; prev and the course stay)

    def _captured_step(self) -> None:
        """Behind every captured step, as in eager mode: the obstacle watch's query, the camera at its cadence of 1, the scan."""
        if self._scene_clock is not None:
            self._scene_move(1)
        if self._obst is not None:
            self._watch_obstacles()
        if self._vision is not None:
            self._vision_capture()
        if self._scan is not None:
            self._scan_now()
        if self._gate is not None:
            self._watch_gates()

    def _capture_keepalive(self):
        """After the capture: what the graph must keep alive.  The captured captures hold the camera's addresses, among them the
        workspace of the drones' grid: an eager capture that later re-measures the box and outgrows it allocates a new one."""
        keep = self._vision.graph_keepalive() if self._vision is not None else ()
        return keep + (self._scan.graph_keepalive() if self._scan is not None else ())

    def _replayed(self) -> None:
        """After a replay (the env's counters moved on already): the camera saw every step of it."""
        self._vision_seen = self.step_counter
        if self._scan is not None:
            self._scan_sampled = True
        if self._gate is not None:
            self._gate_sampled = True

    # ------------------------------------------------------------------ public surface
    @property
    def ranges(self):
        """[B, N] float32: what every beam of the ``range_scan`` fan read behind the last step, in the caller's numbering; None
        before the first step (and without range_scan)."""
        return self._scan.ranges if self._scan is not None and self._scan_sampled else None

    @property
    def range_hits(self):
        """[B, N] int32: what every beam hit behind the last step (body index, -1 nothing, -2 the plane, -3 - k drone k:
        RangeScanner.hit_drone); None before the first step."""
        return self._scan.hits if self._scan is not None and self._scan_sampled else None

    def range_scan(self):
        """(ranges, hits) [B, N] of the CURRENT state, scanned now on the env's stream (not counted as an Env.step)."""
        if self._scan is None:
            raise ValueError("range_scan() needs an env made with range_scan=beams")
        if self._scan.drones and self._downwash is not None:
            self._downwash.invalidate_prebin()
        self._scan.scan()
        return self._scan.ranges, self._scan.hits

    # ---- moving scenes
    def scene_time(self) -> float:
        """Seconds of scene time since reset(): Env.steps so far x one Env.step, read from the device clock (synchronises the
        stream).  The table behind the last launch stands at this time."""
        if self._scene_clock is None:
            raise ValueError("scene_time() needs an env made with obstacle_motion=SceneMotion")
        return int(self._scene_clock.item()) * self._scene_dt()

    def scene_placements(self) -> np.ndarray:
        """float32 [K, G, 12]: the watch's placements as the device holds them now (DeviceScenes.read(): R row-major then t, NaN in
        unused slots; waits for the stream)."""
        if self._scene_clock is None:
            raise ValueError("scene_placements() needs an env made with obstacle_motion=SceneMotion")
        return self._obst.read()

    # ---- the gate passage watch
    def _gate_need(self, what: str) -> None:
        if self._gate is None:
            raise ValueError(f"{what} needs an env made with gate_watch=Aperture")

    def _gate_to_caller(self, t, dim: int = 0):
        t = t[: self.NUM_DRONES] if dim == 0 else t[:, : self.NUM_DRONES]
        return self.order.to_caller(t, dim) if self.order is not None else t

    @property
    def gate_due(self):
        """[N] int32: the slot of its scene every drone has to pass next (the scene's count: finished), the caller's numbering."""
        self._gate_need("gate_due")
        return self._gate_to_caller(self._gate_due)

    @property
    def gate_laps(self):
        """[N] int32: how often every drone completed its scene's gates (``gate_laps=True``; else 0)."""
        self._gate_need("gate_laps")
        return self._gate_to_caller(self._gate_lap)

    @property
    def gate_pass_time(self):
        """[G, N] float64: when every drone last passed slot g IN ORDER, in queries (launches) since reset() — the number of the
        query's chord plus the fraction tau of it at which the plane was crossed; NaN: not passed."""
        self._gate_need("gate_pass_time")
        return self._gate_to_caller(self._gate_time, 1)

    @property
    def last_gate_events(self):
        """(fwd, back, miss) [N] int32 behind the last step, one bit per slot: crossed forward inside the aperture, backward inside
        it, forward outside it but inside the outer rectangle.  None before the first step."""
        self._gate_need("last_gate_events")
        if not self._gate_sampled:
            return None
        return tuple(self._gate_to_caller(t) for t in (self._gate_fwd, self._gate_back, self._gate_miss))

    def _gate_count(self, k: int, what: str) -> int:
        self._gate_need(what)
        return int(self._gate_counts[k].item())

    def gate_passes(self) -> int:
        """Gates passed in order so far, over the fleet (cumulative, also across reset(); synchronises the stream)."""
        return self._gate_count(0, "gate_passes()")

    def gate_wrong_way(self) -> int:
        """Backward crossings inside an aperture so far (cumulative; synchronises the stream)."""
        return self._gate_count(1, "gate_wrong_way()")

    def gate_out_of_order(self) -> int:
        """Forward crossings inside an aperture that did not advance a course: a gate that was not due (cumulative)."""
        return self._gate_count(2, "gate_out_of_order()")

    def gate_misses(self) -> int:
        """Drones x queries whose due gate was crossed forward outside its aperture but inside the outer rectangle (cumulative)."""
        return self._gate_count(3, "gate_misses()")

    def gate_unswept(self) -> int:
        """Drones x queries without a usable chord: longer than gate_travel, or a non-finite position on either end (cumulative).
        Such a chord is no passage, whatever it crossed."""
        return self._gate_count(4, "gate_unswept()")

    def drone_clearance(self, margin: float = 1.0):
        """Per-drone clearance of the CURRENT state between the vehicles' bounding spheres (dsim_clearance; no counterpart in
        the reference, whose Bullet world makes the vehicles collide instead): (clearance [N] float32, nearest [N] int32) in
        the caller's numbering — clearance[i] = min(margin, min_j |p_i - p_j| - R_i - R_j), nearest[i] = the drone that
        attains it, -1 when none is closer than ``margin``.  Negative clearance: the two spheres overlap."""
        if self._clr_on_demand is None:
            self._clr_on_demand = torch.zeros((1,), dtype=torch.int64, device=self.ctx.device)
        return self._drone_query(float(margin), self._clr_on_demand)

    def nearest_neighbors(self, k: Optional[int] = None, radius: Optional[float] = None):
        """The nearest-neighbour observation of the CURRENT state (dsim_knn), asked now on the env's stream: a ``Neighbors``
        record (index [k, N] int32, dist [k, N], rel_pos [k, 3, N], rel_vel [k, 3, N], count [N] int32) in the caller's
        numbering — slot t of drone i is its (t + 1)-th closest drone within ``radius``; unused slots hold -1 / +inf / 0, and
        count is exact whatever k.  ``k`` and ``radius`` default to the env's neighbor_obs and neighbor_radius, the radius
        further to a finite neighbourhood_radius.  env.last_neighbors is left as it is.  Single rank only."""
        if self._knn_sharded:
            raise NotImplementedError("nearest_neighbors() on a sharded fleet: the velocities of the other ranks' drones do not travel")
        if k is None:
            if not self._knn_k:
                raise ValueError("nearest_neighbors(): pass k, or make the env with neighbor_obs=k")
            k = self._knn_k
        if radius is None:
            radius = self._knn_radius if self._knn_k else float(self.NEIGHBOURHOOD_RADIUS)
        if not (np.isfinite(radius) and float(radius) > 0.0):
            raise ValueError("nearest_neighbors(): the radius must be finite and positive (pass radius, or make the env with "
                             "neighbor_radius or a finite neighbourhood_radius)")
        return self._neighbor_query(int(k), float(radius), True, None)

    def neighbor_sight(self, k: Optional[int] = None, radius: Optional[float] = None):
        """(Neighbors, Sight) of the CURRENT state, asked now on the env's stream: what nearest_neighbors(k, radius) returns, and
        for every slot of it whether the segment to that neighbour is clear of the ``neighbor_sight`` world (dsim_line_of_sight on
        that record: visible, blocker, frac [k, N]), both in the caller's numbering.  env.last_neighbors and
        env.last_neighbor_sight are left as they are.  The Sight's tensors are those of the on-demand query of this k: the next
        one writes them again."""
        if self._sight is None:
            raise ValueError("neighbor_sight() needs an env made with neighbor_sight=True")
        k = self._knn_k if k is None else int(k)
        radius = self._knn_radius if radius is None else float(radius)
        if not (np.isfinite(radius) and radius > 0.0):
            raise ValueError("neighbor_sight(): the radius must be finite and positive")
        nb = self._neighbor_raw(k, radius, True, None)
        if k not in self._sight_demand:
            self._sight_demand[k] = self._sight_make(self._sight.set, k)
        if nb.rel_pos is None:
            raise ValueError("the record has no rel_pos")
        return self._neighbors_caller(nb), self._sight_caller(self._sight_query(self._sight_demand[k], nb.rel_pos, nb.index))

    def drone_contacts(self) -> int:
        """Pairs of drones x Env.steps so far whose bounding spheres (DroneType.collision_sphere) overlapped behind a step
        of a ``drone_watch=True`` env (cumulative over this env's context; synchronises the stream).  The reference's
        Bullet world lets the vehicles' collision shapes act on each other; here contact between drones is not modelled,
        and a non-zero count means part of the flight lies outside the domain in which trajectories are comparable with
        the reference.  One-sided: 0 certifies that no two vehicles touched; overlapping spheres need not be touching
        shapes.  That 0 is about the sampled states, one per launch; with ``drone_sweep=True`` the count is of spheres moved along
        the chords between two sampled states, and with drone_sweep_sag >= obstacles.sweep_sag(a_max, time between two queries) and
        drone_unswept() == 0 it certifies the states in between as well.  On-demand drone_clearance() calls are not Env.steps and
        are left out."""
        seen = self.ctx.query(nat.QUERY_DRONE_CONTACTS)
        return seen - (int(self._clr_on_demand.item()) if self._clr_on_demand is not None else 0)

    def drone_unswept(self) -> int:
        """Drones x queries so far of a ``drone_sweep=True`` env that were point samples instead of chords: a chord longer than
        drone_sweep_travel (a teleport, or a launch of more Env.steps than the travel was sized for) or a non-finite position on
        either end (cumulative; synchronises the stream).  0 for a flight: every counted state was reached along a tested chord."""
        if not self._drone_sweep:
            raise ValueError("drone_unswept() needs an env made with drone_watch=True, drone_sweep=True")
        return int(self._drone_unswept.item()) if self._drone_unswept is not None else 0

    @property
    def last_obstacle_clearance(self):
        """(clearance [N] float32, nearest body [N] int32) behind the last step of an ``obstacle_watch`` env, in the
        caller's numbering; None before the first step."""
        if self._obst is None or not self._obst_sampled:
            return None
        return self._obst_to_caller(self._obst_clr, self._obst_near)

    def _obst_to_caller(self, clr, near):
        clr, near = clr[: self.NUM_DRONES], near[: self.NUM_DRONES]
        if self.order is not None:
            clr, near = self.order.to_caller(clr, 0), self.order.to_caller(near, 0)
        return clr, near

    def obstacle_contacts(self) -> int:
        """Drones x sampled Env.steps so far whose bounding sphere (DroneType.collision_sphere) overlapped a triangle of the
        ``obstacle_watch`` set (cumulative over this env's context; synchronises the stream).  The reference's Bullet world
        makes a vehicle collide with the static bodies loaded into it; here they act on nothing, and a non-zero count means
        part of the flight lies outside the domain in which trajectories are comparable with the reference.  One-sided:
        0 certifies that no bounding sphere touched a triangle at the sampled states; an overlapping sphere need not be a
        touching shape.  A step_fused launch with n_steps > 1 is sampled once, at its end.  With ``obstacle_sweep=True`` the
        count is of spheres swept along the chord between two sampled states, and 0 certifies the states in between as well
        (obstacle_sweep_sag covers how far the path leaves the chord; rotation needs no cover: the sphere bounds it).  On-demand
        obstacle_clearance() calls are not Env.steps and are left out."""
        seen = self.ctx.query(nat.QUERY_OBSTACLE_CONTACTS)
        return seen - (int(self._obst_on_demand.item()) if self._obst is not None else 0)

    def obstacle_unswept(self) -> int:
        """Drones x queries so far of an ``obstacle_sweep=True`` env that were point samples instead of chords: a chord of more
        than 32 pieces (a teleport) or a non-finite position on either end (cumulative; synchronises the stream).  0 for
        a flight: every counted state was reached along a tested chord."""
        if self._obst is None or not self._obst_sweep:
            raise ValueError("obstacle_unswept() needs an env made with obstacle_sweep=True")
        return int(self._obst_unswept.item())

    def obstacle_clearance(self, margin: Optional[float] = None):
        """Per-drone clearance of the CURRENT state to the ``obstacle_watch`` set (dsim_obstacle_clearance): (clearance [N]
        float32, nearest [N] int32) in the caller's numbering — clearance[i] = min(margin, min_t dist(p_i - offset_i,
        triangle t) - R_i), nearest[i] = the body of the triangle that attains it, -1 when none is closer than ``margin``
        (default: the env's obstacle_margin, which is also the largest the device set serves).  Not counted as an Env.step."""
        if self._obst is None:
            raise ValueError("obstacle_clearance() needs an env made with obstacle_watch=ObstacleSet")
        return self._obst_now(margin)

    def _obst_now(self, margin, frame=None, velocity=False):
        """The on-demand point query of the current state into tensors of its own, in the caller's numbering; with ``frame`` the
        witness query, and ``rel`` behind the two; with ``velocity`` the witness's velocity behind the three.  Its contacts are
        counted apart (_obst_on_demand)."""
        margin = self._obst_margin if margin is None else float(margin)
        dev, n_pad = self.ctx.device, self.state.n_pad
        clr = torch.empty((n_pad,), dtype=torch.float32, device=dev)
        near = torch.empty((n_pad,), dtype=torch.int32, device=dev)
        rel = torch.zeros((3, n_pad), dtype=torch.float32, device=dev) if frame is not None else None
        vel = torch.zeros((3, n_pad), dtype=torch.float32, device=dev) if velocity else None
        self._obst_query(margin, clr, near, self._obst_on_demand, rel, frame, vel)
        out = self._obst_to_caller(clr, near)
        if rel is not None:
            out = out + (self._rel_to_caller(rel),)
        return out if vel is None else out + (self._rel_to_caller(vel),)

    @property
    def last_obstacle_witness(self):
        """[3, N] float32 behind the last step of an ``obstacle_witness`` env, in the caller's numbering: the vector from every
        drone's query point p_i - offset_i to the closest point of its world, in world axes ("world") or the drone's body axes
        ("body"); zeros where last_obstacle_clearance says (margin, -1).  The unit direction is rel / (clearance + R_i), the
        caller's to guard where the distance vanishes.  None before the first step."""
        if self._obst_rel is None or not self._obst_sampled:
            return None
        return self._rel_to_caller(self._obst_rel)

    def _rel_to_caller(self, rel):
        rel = rel[:, : self.NUM_DRONES]
        return self.order.to_caller(rel, 1) if self.order is not None else rel

    def obstacle_witness(self, margin: Optional[float] = None, frame: Optional[str] = None):
        """(clearance [N] float32, nearest [N] int32, rel [3, N] float32) of the CURRENT state, in the caller's numbering
        (dsim_obstacle_witness / _scenes): what obstacle_clearance() returns and the vector to the closest point of the
        ``obstacle_watch`` world.  ``frame``: "world" or "body" (default: the env's obstacle_witness, else "world").  Not counted as
        an Env.step: the contacts it sees go where obstacle_clearance()'s go."""
        if self._obst is None:
            raise ValueError("obstacle_witness() needs an env made with obstacle_watch=ObstacleSet")
        frame = (self._obst_wit or "world") if frame is None else frame
        if frame not in ("world", "body"):
            raise ValueError(f"frame must be 'world' or 'body', got {frame!r}")
        return self._obst_now(margin, frame)

    @property
    def last_obstacle_witness_velocity(self):
        """[3, N] float32 behind the last step of an ``obstacle_witness_velocity`` env, in the caller's numbering: the velocity of
        the point last_obstacle_witness leads to, as a material point of the moving placement that holds it (t' + w x r at the
        launch's scene time), in the witness's axes; zeros where there is no witness and on a static placement.  None before the
        first step."""
        if self._obst_vel is None or not self._obst_sampled:
            return None
        return self._rel_to_caller(self._obst_vel)

    def obstacle_witness_velocity(self, margin: Optional[float] = None, frame: Optional[str] = None):
        """(clearance [N] float32, nearest [N] int32, rel [3, N] float32, vel [3, N] float32) of the CURRENT state, in the caller's
        numbering (dsim_obstacle_witness_scenes_vel): what obstacle_witness() returns and the velocity of the closest point,
        from the twist table as the last launch left it.  Not counted as an Env.step: the contacts it sees go where
        obstacle_clearance()'s go."""
        if self._obst_vel is None:
            raise ValueError("obstacle_witness_velocity() needs an env made with obstacle_witness_velocity=True")
        frame = self._obst_wit if frame is None else frame
        if frame not in ("world", "body"):
            raise ValueError(f"frame must be 'world' or 'body', got {frame!r}")
        return self._obst_now(margin, frame, velocity=True)

    @property
    def last_obstacle_witnesses(self):
        """The :class:`~dronesim_amd.obstacles.ObstacleWitnesses` behind the last step of an ``obstacle_witnesses=m`` env, in the
        caller's numbering: ``clearance`` / ``body`` [m, N], ``rel`` [m, 3, N] (the env's witness axes), ``vel`` [m, 3, N] with
        ``obstacle_witness_velocity`` else None, ``count`` [N] — per drone the m closest bodies within the margin, ascending;
        (margin, -1, zeros) in an unfilled slot; ``count == m`` may hide further bodies.  Slot 0 is last_obstacle_clearance /
        last_obstacle_witness / last_obstacle_witness_velocity.  None before the first step."""
        if self._obst_wits is None or not self._obst_sampled:
            return None
        return self._wits_to_caller(self._obst_wits)

    def _wits_to_caller(self, w):
        n = self.NUM_DRONES
        to = (lambda t: self.order.to_caller(t[..., :n], -1)) if self.order is not None else (lambda t: t[..., :n])
        return type(w)(to(w.clearance), to(w.body), to(w.rel), to(w.vel) if w.vel is not None else None, to(w.count))

    def obstacle_witnesses(self, margin: Optional[float] = None, frame: Optional[str] = None, m: Optional[int] = None):
        """The :class:`~dronesim_amd.obstacles.ObstacleWitnesses` of the CURRENT state, in the caller's numbering
        (dsim_obstacle_witnesses / _scenes): per drone the ``m`` (default: the env's obstacle_witnesses, else 1) closest bodies of
        the ``obstacle_watch`` world within ``margin``; ``vel`` on an ``obstacle_witness_velocity`` env, from the twist table as
        the last launch left it.  Not counted as an Env.step: the contacts it sees go where obstacle_clearance()'s go."""
        if self._obst is None:
            raise ValueError("obstacle_witnesses() needs an env made with obstacle_watch=ObstacleSet")
        frame = (self._obst_wit or "world") if frame is None else frame
        if frame not in ("world", "body"):
            raise ValueError(f"frame must be 'world' or 'body', got {frame!r}")
        m = (self._obst_m or 1) if m is None else m
        if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 1 <= int(m) <= nat.WITNESSES_MAX:
            raise ValueError(f"m must be an int in 1..{nat.WITNESSES_MAX}, got {m!r}")
        from ..obstacles import ObstacleWitnesses
        margin = self._obst_margin if margin is None else float(margin)
        dev, n_pad, m = self.ctx.device, self.state.n_pad, int(m)
        w = ObstacleWitnesses(torch.empty((m, n_pad), dtype=torch.float32, device=dev), torch.empty((m, n_pad), dtype=torch.int32, device=dev),
                              torch.zeros((m, 3, n_pad), dtype=torch.float32, device=dev),
                              torch.zeros((m, 3, n_pad), dtype=torch.float32, device=dev) if self._obst_vel is not None else None,
                              torch.zeros((n_pad,), dtype=torch.int32, device=dev))
        self._obst_query(margin, w.clearance, w.body, self._obst_on_demand, w.rel, frame, w.vel, m, w.count)
        return self._wits_to_caller(w)

    # ---- the velocity safety filter
    def filter_velocity(self, u):
        """[3, N] float32 in the caller's numbering: the wished velocity ``u`` [3, N] (world axes, m/s) changed as little as the
        control-barrier rows of every drone allow (dsim_velocity_filter; the rows and the drop rule are in
        include/dronesim_amd.h), on the records the env keeps behind the last launch — last_neighbors and
        last_obstacle_witnesses as the queries wrote them, in storage order.  Before the first step (and after a reset) the
        records are asked for on demand, which leaves last_* alone.  The answer lives in the env's own tensor: the next call
        writes it again.  There is no speed cap: step_velocity clamps the speed fraction at 1, which can undo a row."""
        if self._filter is None:
            raise ValueError("filter_velocity() needs an env made with velocity_filter=dict(alpha=...)")
        n = self.NUM_DRONES
        u = torch.as_tensor(u, dtype=torch.float32, device=self.ctx.device)
        if tuple(u.shape) != (3, n):
            raise ValueError(f"u must be [3, {n}]")
        self._filter_u[:, :n].copy_(self.order.to_storage(u, 1) if self.order is not None else u)
        nb = wit = None
        if self._knn_k:
            nb = self._knn_out if self._filter_fresh else self._neighbor_raw(self._knn_k, self._knn_radius, True, None)
        if self._obst_m:
            wit = self._obst_wits
            if not self._filter_fresh:
                from ..obstacles import ObstacleWitnesses
                if self._filter_wits is None:
                    dev, n_pad, m = self.ctx.device, self.state.n_pad, self._obst_m
                    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
                    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
                    self._filter_wits = ObstacleWitnesses(f32(m, n_pad), i32(m, n_pad), f32(m, 3, n_pad),
                                                          f32(m, 3, n_pad) if self._obst_vel is not None else None, i32(n_pad))
                wit = self._filter_wits
                self._obst_query(self._obst_margin, wit.clearance, wit.body, self._obst_on_demand, wit.rel, "world", wit.vel,
                                 self._obst_m, wit.count)
        out = self._filter.apply(self._filter_u, nb, wit, out=self._filter_out)
        self._filter_sampled = True
        return self.order.to_caller(out.vel, 1) if self.order is not None else out.vel

    @property
    def last_filter_dropped(self):
        """[N] int32 in the caller's numbering: the rows the last filter_velocity() could not keep, one bit per row — bit 0 the
        floor, 1 + s obstacle slot s, 9 + t neighbour slot t; None before the first call."""
        if self._filter is None or not self._filter_sampled:
            return None
        d = self._filter_out.dropped[: self.NUM_DRONES]
        return self.order.to_caller(d, 0) if self.order is not None else d

    def filter_counts(self):
        """(drones x calls whose velocity the filter changed, drones x calls with a dropped row), cumulative (synchronises the stream)."""
        if self._filter is None:
            raise ValueError("filter_counts() needs an env made with velocity_filter=dict(alpha=...)")
        return self._filter.counters()

    # ---- corridor clearance
    def corridor_clearance(self, rel, index=None):
        """CorridorClearance(clearance [k, N] float32, body [k, N] int32) in the caller's numbering: for slot t of drone i the
        clearance of its bounding sphere (+ sag) swept from p_i - offset_i along ``rel[t, :, i]`` ([k, 3, N], world axes, m)
        against the ``obstacle_watch`` world as it stands now and, with ground, the half-space z <= 0 (dsim_corridor_clearance;
        include/dronesim_amd.h), cut at the corridor's margin; ``body`` the body that attains it (-2 the ground, -1 none within
        the margin).  ``index`` [k, N] ints or None: a slot whose index is negative is not evaluated.  A slot that is not
        evaluated (also: a non-finite rel or position) or not served (longer than 32 pieces: corridor_unserved()) reads -inf / -1
        — never "free".  The answer lives in the env's own tensors: the next call writes them again.  Not counted as an
        Env.step, and no contact counter moves."""
        if self._corr is None:
            raise ValueError("corridor_clearance() needs an env made with corridor=dict(k=..., piece=...)")
        n, k, dev = self.NUM_DRONES, self._corr.k, self.ctx.device
        rel = torch.as_tensor(rel, dtype=torch.float32, device=dev)
        if tuple(rel.shape) != (k, 3, n):
            raise ValueError(f"rel must be [{k}, 3, {n}]")
        self._corr_rel[:, :, :n].copy_(self.order.to_storage(rel, 2) if self.order is not None else rel)
        if index is not None:
            index = torch.as_tensor(index, device=dev)
            if tuple(index.shape) != (k, n) or index.dtype.is_floating_point or index.dtype == torch.bool:
                raise ValueError(f"index must be [{k}, {n}] ints")
            index = index.clamp(min=-1, max=2 ** 31 - 1).to(torch.int32)
            self._corr_index[:, :n].copy_(self.order.to_storage(index, 1) if self.order is not None else index)
        out = self._corr.query(self._corr_rel, self._corr_index if index is not None else None)
        if self.order is None:
            return out
        from ..corridor import CorridorClearance
        return CorridorClearance(*(self.order.to_caller(t, 1) for t in out))

    def corridor_unserved(self) -> int:
        """Slots x corridor_clearance() calls so far whose segment needed more than 32 pieces (longer than the Corridor's
        max_length; synchronises the stream): they read -inf."""
        if self._corr is None:
            raise ValueError("corridor_unserved() needs an env made with corridor=dict(k=..., piece=...)")
        return self._corr.unserved()

    def scene_twists(self) -> np.ndarray:
        """float32 [K, G, 6]: (t', w) of the watch's placements as the device holds them now, the last launch's scene time; zeros
        in static slots, NaN in unused ones (waits for the stream)."""
        if self._obst_vel is None:
            raise ValueError("scene_twists() needs an env made with obstacle_witness_velocity=True")
        tw = self._obst.twist.cpu().numpy()
        out = np.concatenate([tw[..., 0:3], tw[..., 4:7]], -1)
        out[~self._motion.used] = np.nan
        return out

    def drone_images(self):
        """(dep, seg) of the CURRENT state, captured now on the env's stream into env.dep / env.seg (BaseAviary._getDroneImages
        for every camera drone at once): float32 depth-buffer values and int32 body indices [n, H, W]."""
        if self._vision is None:
            raise ValueError("drone_images() needs an env made with vision_attributes=True")
        return self._vision_capture()
