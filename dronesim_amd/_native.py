"""ctypes binding of libdronesim_amd.so (the C-ABI in include/dronesim_amd.h).

There is no CPU fallback: if the shared library is missing or does not load the
import fails loudly, and ``Context`` fails when no HIP device is present.
"""
from __future__ import annotations

import ctypes
import os

from .params import TypeParamsC

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdronesim_amd.so")

# every symbol include/dronesim_amd.h declares
EXPORTS = (
    "dsim_abi_version", "dsim_strerror", "dsim_create", "dsim_destroy", "dsim_reset", "dsim_step",
    "dsim_physics", "dsim_control", "dsim_control2", "dsim_step_adaptor", "dsim_traj_sample", "dsim_materialize",
    "dsim_counter_add", "dsim_reserve", "dsim_observe", "dsim_observe_soa", "dsim_query", "dsim_downwash",
    "dsim_downwash_workspace", "dsim_downwash_prebin_ok", "dsim_downwash_reset", "dsim_adjacency", "dsim_wls_fallback", "dsim_fleet_bounds",
    "dsim_halo_pack", "dsim_downwash_workspace_halo", "dsim_dev_alloc", "dsim_dev_free", "dsim_noise_draw",
    "dsim_downwash_keep_workspace", "dsim_downwash_keep_ok", "dsim_downwash_keep_stats",
    "dsim_clearance", "dsim_clearance_workspace", "dsim_abi_minor",
    "dsim_obstacle_grid_plan", "dsim_obstacle_grid_build", "dsim_obstacles_create", "dsim_obstacles_destroy", "dsim_obstacle_clearance",
    "dsim_obstacle_ray_grid_plan", "dsim_obstacle_ray_grid_build", "dsim_obstacles_enable_rays", "dsim_depth_image",
    "dsim_depth_image_drones", "dsim_depth_image_drones_workspace",
    "dsim_trajgen", "dsim_trajgen_workspace", "dsim_traj_sample_bank",
    "dsim_obstacle_sweep",
    "dsim_scenes_create", "dsim_scenes_destroy", "dsim_obstacle_clearance_scenes", "dsim_depth_image_scenes",
    "dsim_clearance_sweep", "dsim_clearance_sweep_workspace",
    "dsim_range_scan",
    "dsim_gate_passage",
    "dsim_knn", "dsim_knn_workspace",
    "dsim_obstacle_witness", "dsim_obstacle_witness_scenes",
    "dsim_line_of_sight",
    "dsim_scenes_motion_set", "dsim_scenes_move", "dsim_scenes_read",
    "dsim_scenes_move_twist", "dsim_obstacle_witness_scenes_vel",
    "dsim_obstacle_witnesses", "dsim_obstacle_witnesses_scenes",
    "dsim_velocity_filter",
    "dsim_line_of_sight_drones",
    "dsim_corridor_clearance",
)

ABI_VERSION = 11
ABI_MINOR = 1            # DSIM_ABI_MINOR: dsim_type_params ends with collision_sphere; dsim_clearance
MAX_PEERS = 8
HALO_HDR = 8           # header floats of a halo message (DSIM_HALO_HDR)
DW_ALL, DW_LOCAL, DW_HALO_BIN, DW_HALO_QUERY = 0, 1, 2, 3
DW_KEEP_OFF, DW_KEEP_BUILD, DW_KEEP_REUSE = 0, 1, 2      # dsim_downwash_args.keep
NF_QUAD, NF_HEXA, NT = 24, 26, 10
OPT_DRAG, OPT_GROUND, OPT_BCAST_TGT, OPT_CHAINED = 1, 2, 4, 8
OPT_STREAM_ON, OPT_STREAM_OFF = 16, 32      # tuning knobs (results do not depend on them)
# option bits of measured-and-rejected kernel forms (tools/variants/ up to round 5, in the git history): reserved, ignored by the library
VAR_GENERIC, VAR_MIXED_V1, VAR_MIXED_RING, VAR_MIXED_V3, VAR_RUNS_SEPARATE = 64, 128, 256, 512, 1 << 13
TUNING_MASK = OPT_STREAM_ON | OPT_STREAM_OFF | VAR_GENERIC | VAR_MIXED_V1 | VAR_MIXED_RING | VAR_MIXED_V3 | VAR_RUNS_SEPARATE
OPT_PLANE = 1 << 10        # ground-plane contact (product-defined model, oracle/dsim_oracle.c:orc_plane_contact)
OPT_DEFER_FALLBACK = 1 << 11   # the caller launches dsim_wls_fallback itself (scheduling only)
OPT_CALLER_IO = 1 << 14    # dsim_physics / dsim_control2: action, rows, command, errors indexed by drone_id[i] (the caller's numbering)
OPT_ACTION_ROWS = 1 << 15  # dsim_step_adaptor: the action row-major [n][4]
OPT_DYN = 1 << 16          # Physics.DYN: BaseAviary._dynamics instead of the Bullet step (StepArgs.dyn_rpy_rates required)
OPT_DYN_BODY_RATES = 1 << 17   # ... with ang_v = R(quat) rpy_rates instead of the reference's placeholder (-1, -1, -1)
# rotor noise: which Box-Muller lattice a launch draws on (changes results).  Neither bit: the fine one (16 + 16 bits per pair) for a launch
# of ONE physics sub-step, the coarse one (8 + 8 bits) for a launch of several; the bits force one at any count (include/dronesim_amd.h)
OPT_NOISE_FINE = 1 << 18
OPT_NOISE_COARSE = 1 << 19
# the caller asserts that the target groups of StepArgs.tgt_const_mask (bit 0 pos, 1 vel, 2 acc, 3 yaw) hold StepArgs.tgt_const for every
# drone; the library may skip reading them (results do not depend on it; include/dronesim_amd.h)
OPT_TGT_CONST = 1 << 20
OPT_MEM_DERIVED = 1 << 21
TGT_CONST_POS_PER_DRONE = 0xE   # the mask the kernels honour: pos per drone, vel / acc / yaw constant
# StepArgs.tgt_period (no option bit, 0 = none): the caller asserts that every target field of drone i equals that of drone
# i mod tgt_period; the library may read the first period only (results do not depend on it; include/dronesim_amd.h)
ADAPT_VELOCITY, ADAPT_RPYT = 0, 1
QUERY_WLS_FALLBACKS, QUERY_WLS_FAILURES, QUERY_GROUND_CONTACTS, QUERY_HALO_OVERFLOW = 0, 1, 2, 3
QUERY_DW_REUSES, QUERY_DW_MOVERS = 4, 5
QUERY_DRONE_CONTACTS = 6     # pairs of drones x dsim_clearance calls whose bounding spheres overlapped
QUERY_OBSTACLE_CONTACTS = 7  # drones x dsim_obstacle_clearance calls whose bounding sphere overlapped a triangle of the set


CAM_METRIC, CAM_GROUND = 1, 2    # dsim_camera_params.flags
SEG_GROUND = -2                  # DSIM_SEG_GROUND: the plane z = 0 in a segmentation image


class CameraParams(ctypes.Structure):
    """dsim_camera_params (dsim_depth_image)."""
    _fields_ = [
        ("width", ctypes.c_int32),
        ("height", ctypes.c_int32),
        ("fov_deg", ctypes.c_float),
        ("aspect", ctypes.c_float),
        ("far", ctypes.c_float),
        ("flags", ctypes.c_uint32),
    ]


def seg_drone(k: int) -> int:
    """DSIM_SEG_DRONE(k): drone k in a segmentation image (its own inverse)."""
    return -3 - k


class CameraDrones(ctypes.Structure):
    """dsim_camera_drones (dsim_depth_image_drones)."""
    _fields_ = [
        ("grid", ctypes.c_void_p),
        ("radius_all", ctypes.c_void_p),
        ("label", ctypes.c_void_p),
        ("range", ctypes.c_float),
        ("outside_out", ctypes.c_void_p),
    ]


SCAN_GROUND, SCAN_CLAMP = 1, 2   # dsim_scan_args.flags


class ScanArgs(ctypes.Structure):
    """dsim_scan_args (dsim_range_scan)."""
    _fields_ = [
        ("beams", ctypes.c_void_p),
        ("n_beams", ctypes.c_int32),
        ("t_min", ctypes.c_float),
        ("t_max", ctypes.c_float),
        ("flags", ctypes.c_uint32),
        ("offset", ctypes.c_void_p),
        ("type_id", ctypes.c_void_p),
        ("scenes", ctypes.c_void_p),
        ("scene_id", ctypes.c_void_p),
        ("drones", ctypes.c_void_p),
        ("range_out", ctypes.c_void_p),
        ("hit_out", ctypes.c_void_p),
    ]


SIGHT_GROUND = 1                 # dsim_sight_args.flags
SIGHT_MAX_K = 32                 # dsim_sight_args.k: 1 .. 32


class SightArgs(ctypes.Structure):
    """dsim_sight_args (dsim_line_of_sight)."""
    _fields_ = [
        ("rel", ctypes.c_void_p),
        ("index", ctypes.c_void_p),
        ("k", ctypes.c_int32),
        ("flags", ctypes.c_uint32),
        ("offset", ctypes.c_void_p),
        ("scenes", ctypes.c_void_p),
        ("scene_id", ctypes.c_void_p),
        ("visible_out", ctypes.c_void_p),
        ("blocker_out", ctypes.c_void_p),
        ("frac_out", ctypes.c_void_p),
    ]


TRAJGEN_GIVEN, TRAJGEN_TMIN, TRAJGEN_OPTIMIZE = 0, 1, 2     # dsim_trajgen_args.mode
TRAJGEN_LMAX = 9                                              # DSIM_TRAJGEN_LMAX: waypoints per course
TRAJGEN_BAD_COUNT, TRAJGEN_BAD_WAYPOINT, TRAJGEN_BAD_SEGMENT, TRAJGEN_BAD_TIME, TRAJGEN_BAD_CONDITION = 1, 2, 3, 4, 5    # status of a course


class TrajBank(ctypes.Structure):
    """dsim_traj_bank: K courses, course-minor (dsim_trajgen, dsim_traj_sample_bank)."""
    _fields_ = [
        ("K", ctypes.c_int64),
        ("K_pad", ctypes.c_int64),
        ("L_max", ctypes.c_int32),
        ("_pad", ctypes.c_int32),
        ("coeffs", ctypes.c_void_p),
        ("ts", ctypes.c_void_p),
        ("n_seg", ctypes.c_void_p),
    ]


class TrajGenArgs(ctypes.Structure):
    """dsim_trajgen_args."""
    _fields_ = [
        ("wp", ctypes.c_void_p),
        ("n_wp", ctypes.c_void_p),
        ("max_vel", ctypes.c_double),
        ("gamma", ctypes.c_double),
        ("mode", ctypes.c_int32),
        ("max_evals", ctypes.c_int32),
        ("cost", ctypes.c_void_p),
        ("evals", ctypes.c_void_p),
        ("status", ctypes.c_void_p),
        ("seg_times", ctypes.c_void_p),
        ("workspace", ctypes.c_void_p),
        ("workspace_len", ctypes.c_int64),
    ]


class ObstacleGrid(ctypes.Structure):
    """dsim_obstacle_grid: the uniform 3-D grid around a triangle soup (dsim_obstacle_grid_plan)."""
    _fields_ = [
        ("origin", ctypes.c_float * 3),
        ("cell", ctypes.c_float),
        ("nx", ctypes.c_int32),
        ("ny", ctypes.c_int32),
        ("nz", ctypes.c_int32),
        ("reach", ctypes.c_float),
        ("list_len", ctypes.c_int64),
        ("lo", ctypes.c_float * 3),
        ("hi", ctypes.c_float * 3),
    ]


SWEEP_KEEP_PREV, SWEEP_PRIME = 1, 2     # dsim_sweep_args.flags


CORRIDOR_GROUND = 1              # dsim_corridor_args.flags
CORRIDOR_MAX_K = 32              # dsim_corridor_args.k: 1 .. 32
CORRIDOR_MAX_PIECES = 32         # a slot that needs more pieces is unserved


class CorridorArgs(ctypes.Structure):
    """dsim_corridor_args (dsim_corridor_clearance)."""
    _fields_ = [
        ("rel", ctypes.c_void_p),
        ("index", ctypes.c_void_p),
        ("k", ctypes.c_int32),
        ("flags", ctypes.c_uint32),
        ("offset", ctypes.c_void_p),
        ("type_id", ctypes.c_void_p),
        ("scenes", ctypes.c_void_p),
        ("scene_id", ctypes.c_void_p),
        ("margin", ctypes.c_float),
        ("sag", ctypes.c_float),
        ("clearance_out", ctypes.c_void_p),
        ("body_out", ctypes.c_void_p),
        ("unserved_out", ctypes.c_void_p),
    ]


class SweepArgs(ctypes.Structure):
    """dsim_sweep_args (dsim_obstacle_sweep)."""
    _fields_ = [
        ("offset", ctypes.c_void_p),
        ("type_id", ctypes.c_void_p),
        ("margin", ctypes.c_float),
        ("sag", ctypes.c_float),
        ("prev", ctypes.c_void_p),
        ("flags", ctypes.c_int32),
        ("clearance_out", ctypes.c_void_p),
        ("nearest_out", ctypes.c_void_p),
        ("contacts_out", ctypes.c_void_p),
        ("unswept_out", ctypes.c_void_p),
    ]


WITNESS_BODY_FRAME = 1                  # dsim_witness_args.flags


class WitnessArgs(ctypes.Structure):
    """dsim_witness_args (dsim_obstacle_witness, dsim_obstacle_witness_scenes)."""
    _fields_ = [
        ("offset", ctypes.c_void_p),
        ("type_id", ctypes.c_void_p),
        ("margin", ctypes.c_float),
        ("flags", ctypes.c_int32),
        ("clearance_out", ctypes.c_void_p),
        ("nearest_out", ctypes.c_void_p),
        ("rel_out", ctypes.c_void_p),
        ("triangle_out", ctypes.c_void_p),
        ("contacts_out", ctypes.c_void_p),
    ]


WITNESSES_MAX = 8                       # DSIM_WITNESSES_MAX: slots per drone of dsim_obstacle_witnesses


class WitnessesArgs(ctypes.Structure):
    """dsim_witnesses_args (dsim_obstacle_witnesses, dsim_obstacle_witnesses_scenes)."""
    _fields_ = [
        ("offset", ctypes.c_void_p),
        ("type_id", ctypes.c_void_p),
        ("margin", ctypes.c_float),
        ("m", ctypes.c_int32),
        ("flags", ctypes.c_int32),
        ("clearance_out", ctypes.c_void_p),
        ("body_out", ctypes.c_void_p),
        ("rel_out", ctypes.c_void_p),
        ("triangle_out", ctypes.c_void_p),
        ("count_out", ctypes.c_void_p),
        ("contacts_out", ctypes.c_void_p),
        ("twist", ctypes.c_void_p),
        ("vel_out", ctypes.c_void_p),
    ]


APERTURE_RECT, APERTURE_ELLIPSE = 0, 1      # dsim_aperture.shape
GATE_WRAP = 4                                # dsim_gate_args.flags, beside SWEEP_KEEP_PREV and SWEEP_PRIME


class ApertureC(ctypes.Structure):
    """dsim_aperture (dsim_gate_passage)."""
    _fields_ = [
        ("center", ctypes.c_float * 3),
        ("normal", ctypes.c_float * 3),
        ("u", ctypes.c_float * 3),
        ("half", ctypes.c_float * 2),
        ("outer", ctypes.c_float * 2),
        ("shape", ctypes.c_int32),
    ]


class GateArgs(ctypes.Structure):
    """dsim_gate_args (dsim_gate_passage)."""
    _fields_ = [
        ("aperture", ApertureC),
        ("travel", ctypes.c_float),
        ("flags", ctypes.c_int32),
        ("offset", ctypes.c_void_p),
        ("prev", ctypes.c_void_p),
        ("due", ctypes.c_void_p),
        ("laps", ctypes.c_void_p),
        ("clock", ctypes.c_void_p),
        ("pass_time", ctypes.c_void_p),
        ("fwd_out", ctypes.c_void_p),
        ("back_out", ctypes.c_void_p),
        ("miss_out", ctypes.c_void_p),
        ("passes_out", ctypes.c_void_p),
        ("wrong_way_out", ctypes.c_void_p),
        ("out_of_order_out", ctypes.c_void_p),
        ("misses_out", ctypes.c_void_p),
        ("unswept_out", ctypes.c_void_p),
    ]


class SceneMotionC(ctypes.Structure):
    """dsim_scene_motion (dsim_scenes_motion_set): one placement's motion record, 64 bytes."""
    _fields_ = [
        ("vel", ctypes.c_float * 3),
        ("amp", ctypes.c_float * 3),
        ("omega", ctypes.c_float),
        ("phase", ctypes.c_float),
        ("axis", ctypes.c_float * 3),
        ("rate", ctypes.c_float),
        ("swing", ctypes.c_float),
        ("pad_", ctypes.c_float * 3),
    ]


class ClearanceSweepArgs(ctypes.Structure):
    """dsim_clearance_sweep_args (dsim_clearance_sweep); flags as dsim_sweep_args'."""
    _fields_ = [
        ("prev", ctypes.c_void_p),
        ("margin", ctypes.c_float),
        ("sag", ctypes.c_float),
        ("travel", ctypes.c_float),
        ("flags", ctypes.c_int32),
        ("clearance_out", ctypes.c_void_p),
        ("nearest_out", ctypes.c_void_p),
        ("pairs_out", ctypes.c_void_p),
        ("unswept_out", ctypes.c_void_p),
    ]


KNN_MAX_K = 16            # dsim_knn_args.k: 1 .. 16


class KnnArgs(ctypes.Structure):
    """dsim_knn_args (dsim_knn): the k nearest drones within a radius, sorted, with their relative state."""
    _fields_ = [
        ("grid", ctypes.c_void_p),          # const dsim_downwash_args*
        ("radius", ctypes.c_float),
        ("k", ctypes.c_int32),
        ("flags", ctypes.c_int32),
        ("index_out", ctypes.c_void_p),
        ("dist_out", ctypes.c_void_p),
        ("rel_pos_out", ctypes.c_void_p),
        ("rel_vel_out", ctypes.c_void_p),
        ("count_out", ctypes.c_void_p),
    ]


FILTER_FLOOR_BIT, FILTER_OBSTACLE_BIT, FILTER_NEIGHBOR_BIT, FILTER_ROWS = 0, 1, 9, 25      # DSIM_FILTER_*: the bits of dropped_out


class FilterArgs(ctypes.Structure):
    """dsim_filter_args (dsim_velocity_filter): the wished velocity, the barrier's constants and the records the rows are built from."""
    _fields_ = [
        ("u", ctypes.c_void_p),
        ("offset", ctypes.c_void_p),
        ("type_id", ctypes.c_void_p),
        ("alpha", ctypes.c_float),
        ("share", ctypes.c_float),
        ("buffer_drone", ctypes.c_float),
        ("buffer_obstacle", ctypes.c_float),
        ("floor", ctypes.c_float),
        ("has_floor", ctypes.c_int32),
        ("k", ctypes.c_int32),
        ("m", ctypes.c_int32),
        ("nb_index", ctypes.c_void_p),
        ("nb_dist", ctypes.c_void_p),
        ("nb_rel_pos", ctypes.c_void_p),
        ("nb_rel_vel", ctypes.c_void_p),
        ("wit_clearance", ctypes.c_void_p),
        ("wit_body", ctypes.c_void_p),
        ("wit_rel", ctypes.c_void_p),
        ("wit_vel", ctypes.c_void_p),
        ("v_out", ctypes.c_void_p),
        ("dropped_out", ctypes.c_void_p),
        ("counters", ctypes.c_void_p),
    ]


class View(ctypes.Structure):
    _fields_ = [
        ("base", ctypes.c_void_p),
        ("n_pad", ctypes.c_int64),
        ("block", ctypes.c_int64),
        ("field_stride", ctypes.c_int64),
        ("block_stride", ctypes.c_int64),
        ("n_fields", ctypes.c_int32),
        ("_pad", ctypes.c_int32),
    ]


class StepArgs(ctypes.Structure):
    _fields_ = [
        ("phys_substeps", ctypes.c_int32),
        ("dt_phys", ctypes.c_float),
        ("dt_ctrl", ctypes.c_float),
        ("options", ctypes.c_uint32),
        ("noise_seed", ctypes.c_uint64),
        ("step_index", ctypes.c_uint64),
        ("noise_replay", ctypes.c_void_p),
        ("type_id", ctypes.c_void_p),
        ("action", ctypes.c_void_p),
        ("wp_table", ctypes.c_void_p),
        ("wp_counter", ctypes.c_void_p),
        ("wp_offset", ctypes.c_void_p),
        ("n_wp", ctypes.c_int32),
        ("n_steps", ctypes.c_int32),
        ("ext_force", ctypes.c_void_p),
        ("step_index_dev", ctypes.c_void_p),
        ("runs", ctypes.c_void_p),
        ("n_runs", ctypes.c_int32),
        ("obs_width", ctypes.c_int32),
        ("obs_out", ctypes.c_void_p),
        ("bin_next", ctypes.c_void_p),
        ("drone_id", ctypes.c_void_p),
        ("dyn_rpy_rates", ctypes.c_void_p),
        ("tgt_const_mask", ctypes.c_uint32),
        ("tgt_const", ctypes.c_float * 10),
        ("tgt_period", ctypes.c_int64),
    ]


class TypeRun(ctypes.Structure):
    _fields_ = [("first", ctypes.c_int64), ("count", ctypes.c_int64), ("type", ctypes.c_int32), ("_pad", ctypes.c_int32)]


class DownwashArgs(ctypes.Structure):
    _fields_ = [
        ("pos_all", ctypes.c_void_p),
        ("m", ctypes.c_int64),
        ("m_pad", ctypes.c_int64),
        ("xmin", ctypes.c_float),
        ("ymin", ctypes.c_float),
        ("cell", ctypes.c_float),
        ("nx", ctypes.c_int32),
        ("ny", ctypes.c_int32),
        ("workspace", ctypes.c_void_p),
        ("workspace_len", ctypes.c_int64),
        ("type_id", ctypes.c_void_p),
        ("local_offset", ctypes.c_int64),
        ("prebinned", ctypes.c_int32),
        ("phase", ctypes.c_int32),
        ("halo", ctypes.c_void_p),
        ("pairs_evaluated", ctypes.c_void_p),
        ("keep", ctypes.c_int32),
        ("keep_age", ctypes.c_int32),
        ("keep_skin", ctypes.c_float),
        ("keep_ws", ctypes.c_void_p),
        ("keep_ws_len", ctypes.c_int64),
    ]


class HaloPlan(ctypes.Structure):
    _fields_ = [
        ("world", ctypes.c_int32),
        ("rank", ctypes.c_int32),
        ("cap", ctypes.c_int64),
        ("send", ctypes.c_void_p),
        ("recv", ctypes.c_void_p),
        ("scratch", ctypes.c_void_p),
        ("send_cap", ctypes.c_int32 * MAX_PEERS),
        ("recv_cap", ctypes.c_int32 * MAX_PEERS),
        ("reach", ctypes.c_float * MAX_PEERS),
    ]


class DsimError(RuntimeError):
    pass


_lib = None


def load(path: str = None) -> ctypes.CDLL:
    """Load the HIP extension; raises if it has not been built (``__graft_entry__.build()``).  ``path``: a
    differently-tuned build of the same ABI (A/B runs); must be given on the first call."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()'). dronesim_amd has no CPU fallback.")
    # torch first: its wheel bundles the HIP runtime; loading ours afterwards binds to that same
    # libamdhip64 instead of pulling a second runtime into the process
    import torch  # noqa: F401
    lib = ctypes.CDLL(path)
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    lib.dsim_abi_version.restype = ctypes.c_int
    lib.dsim_strerror.restype = ctypes.c_char_p
    lib.dsim_strerror.argtypes = [ctypes.c_int]
    lib.dsim_create.argtypes = [ctypes.POINTER(vp), ctypes.c_int, ctypes.POINTER(TypeParamsC), ctypes.c_int]
    lib.dsim_destroy.argtypes = [vp]
    lib.dsim_reset.argtypes = [vp, vp, i64, View, vp, vp, vp, vp, vp]
    lib.dsim_step.argtypes = [vp, vp, i64, View, View, ctypes.POINTER(StepArgs)]
    lib.dsim_physics.argtypes = [vp, vp, i64, View, vp, ctypes.POINTER(StepArgs)]  # (.., last_action_out, args)
    lib.dsim_control.argtypes = [vp, vp, i64, View, View, ctypes.POINTER(StepArgs), vp, vp]
    lib.dsim_control2.argtypes = [vp, vp, i64, View, View, ctypes.POINTER(StepArgs), vp, vp, vp]
    lib.dsim_downwash_prebin_ok.argtypes = [i64, i32, i32]
    lib.dsim_downwash_reset.argtypes = [ctypes.c_void_p]
    lib.dsim_step_adaptor.argtypes = [vp, vp, i64, View, vp, i32, vp, ctypes.POINTER(StepArgs)]
    lib.dsim_traj_sample.argtypes = [vp, vp, i64, vp, vp, i32, vp, ctypes.c_double, vp, vp, View]
    lib.dsim_materialize.argtypes = [vp, vp, i64, View]
    lib.dsim_counter_add.argtypes = [vp, vp, vp, ctypes.c_uint64]
    lib.dsim_reserve.argtypes = [vp, vp, i64]
    lib.dsim_observe.argtypes = [vp, vp, i64, View, vp, vp, i32]
    lib.dsim_observe_soa.argtypes = [vp, vp, i64, View, vp, vp, i32]
    lib.dsim_query.argtypes = [vp, vp, i32, ctypes.POINTER(ctypes.c_int64)]
    lib.dsim_downwash_workspace.restype = ctypes.c_int64
    lib.dsim_downwash_workspace.argtypes = [i64, i32, i32]
    lib.dsim_downwash.argtypes = [vp, vp, i64, View, ctypes.POINTER(DownwashArgs), vp]
    lib.dsim_adjacency.argtypes = [vp, vp, i64, View, ctypes.POINTER(DownwashArgs), ctypes.c_float, vp, vp, i32]
    lib.dsim_wls_fallback.argtypes = [vp, vp, i64, View, vp, vp]
    lib.dsim_fleet_bounds.argtypes = [vp, vp, i64, View, vp]
    lib.dsim_halo_pack.argtypes = [vp, vp, i64, View, ctypes.POINTER(HaloPlan)]
    lib.dsim_dev_alloc.argtypes = [vp, i64, ctypes.POINTER(vp)]
    lib.dsim_dev_free.argtypes = [vp, vp]
    lib.dsim_noise_draw.argtypes = [vp, vp, i64, i64, i32, ctypes.c_uint64, ctypes.c_uint64, i32, ctypes.c_uint32, vp, vp]
    lib.dsim_downwash_workspace_halo.restype = ctypes.c_int64
    lib.dsim_downwash_workspace_halo.argtypes = [i64, i64, i32, i32]
    lib.dsim_downwash_keep_workspace.restype = ctypes.c_int64
    lib.dsim_downwash_keep_workspace.argtypes = [i64, i32, i32]
    lib.dsim_downwash_keep_ok.argtypes = [i64, i32, i32, ctypes.c_float, ctypes.c_float]
    lib.dsim_downwash_keep_stats.argtypes = [vp] + [ctypes.POINTER(ctypes.c_int64)] * 4
    lib.dsim_clearance_workspace.restype = ctypes.c_int64
    lib.dsim_clearance_workspace.argtypes = [i64, i32, i32]
    lib.dsim_clearance.argtypes = [vp, vp, i64, View, ctypes.POINTER(DownwashArgs), vp, ctypes.c_float, vp, vp, vp]
    lib.dsim_abi_minor.restype = ctypes.c_int
    lib.dsim_obstacle_grid_plan.argtypes = [vp, i64, ctypes.c_float, ctypes.POINTER(ObstacleGrid)]
    lib.dsim_obstacle_grid_build.argtypes = [vp, i64, ctypes.POINTER(ObstacleGrid), vp, vp]
    lib.dsim_obstacles_create.argtypes = [vp, vp, vp, i64, ctypes.c_float, ctypes.POINTER(vp)]
    lib.dsim_obstacles_destroy.argtypes = [vp, vp]
    lib.dsim_obstacle_clearance.argtypes = [vp, vp, i64, View, vp, vp, vp, ctypes.c_float, vp, vp, vp]
    lib.dsim_obstacle_sweep.argtypes = [vp, vp, i64, View, vp, ctypes.POINTER(SweepArgs)]
    lib.dsim_clearance_sweep_workspace.restype = ctypes.c_int64
    lib.dsim_clearance_sweep_workspace.argtypes = [i64, i32, i32]
    lib.dsim_clearance_sweep.argtypes = [vp, vp, i64, View, ctypes.POINTER(DownwashArgs), ctypes.POINTER(ClearanceSweepArgs)]
    lib.dsim_obstacle_ray_grid_plan.argtypes = [vp, i64, ctypes.POINTER(ObstacleGrid)]
    lib.dsim_obstacle_ray_grid_build.argtypes = [vp, i64, ctypes.POINTER(ObstacleGrid), vp, vp]
    lib.dsim_obstacles_enable_rays.argtypes = [vp, vp]
    lib.dsim_depth_image.argtypes = [vp, vp, View, vp, ctypes.POINTER(CameraParams), i64, vp, vp, vp, vp, vp]
    lib.dsim_depth_image_drones_workspace.restype = ctypes.c_int64
    lib.dsim_depth_image_drones_workspace.argtypes = [i64, i32, i32]
    lib.dsim_depth_image_drones.argtypes = [vp, vp, View, vp, ctypes.POINTER(CameraParams), i64, vp, vp, vp, ctypes.POINTER(CameraDrones), vp, vp]
    lib.dsim_scenes_create.argtypes = [vp, vp, vp, vp, i64, i32, ctypes.POINTER(vp)]
    lib.dsim_scenes_destroy.argtypes = [vp, vp]
    lib.dsim_obstacle_clearance_scenes.argtypes = [vp, vp, i64, View, vp, vp, vp, vp, ctypes.c_float, vp, vp, vp]
    lib.dsim_depth_image_scenes.argtypes = [vp, vp, View, vp, vp, ctypes.POINTER(CameraParams), i64, vp, vp, vp, vp, vp]
    lib.dsim_scenes_motion_set.argtypes = [vp, vp, vp]
    lib.dsim_scenes_move.argtypes = [vp, vp, vp, vp, ctypes.c_double, ctypes.c_double]
    lib.dsim_scenes_read.argtypes = [vp, vp, vp, vp]
    lib.dsim_scenes_move_twist.argtypes = [vp, vp, vp, vp, ctypes.c_double, ctypes.c_double, vp]
    lib.dsim_obstacle_witness.argtypes = [vp, vp, i64, View, vp, ctypes.POINTER(WitnessArgs)]
    lib.dsim_obstacle_witness_scenes.argtypes = [vp, vp, i64, View, vp, vp, ctypes.POINTER(WitnessArgs)]
    lib.dsim_obstacle_witness_scenes_vel.argtypes = [vp, vp, i64, View, vp, vp, ctypes.POINTER(WitnessArgs), vp, vp]
    lib.dsim_obstacle_witnesses.argtypes = [vp, vp, i64, View, vp, ctypes.POINTER(WitnessesArgs)]
    lib.dsim_obstacle_witnesses_scenes.argtypes = [vp, vp, i64, View, vp, vp, ctypes.POINTER(WitnessesArgs)]
    lib.dsim_range_scan.argtypes = [vp, vp, i64, View, vp, ctypes.POINTER(ScanArgs)]
    lib.dsim_line_of_sight.argtypes = [vp, vp, i64, View, vp, ctypes.POINTER(SightArgs)]
    lib.dsim_line_of_sight_drones.argtypes = [vp, vp, i64, View, vp, ctypes.POINTER(SightArgs), vp, ctypes.POINTER(CameraDrones)]
    lib.dsim_corridor_clearance.argtypes = [vp, vp, i64, View, vp, ctypes.POINTER(CorridorArgs)]
    lib.dsim_gate_passage.argtypes = [vp, vp, i64, View, vp, vp, ctypes.POINTER(GateArgs)]
    lib.dsim_knn_workspace.restype = ctypes.c_int64
    lib.dsim_knn_workspace.argtypes = [i64, i32, i32]
    lib.dsim_knn.argtypes = [vp, vp, i64, View, ctypes.POINTER(KnnArgs)]
    lib.dsim_velocity_filter.argtypes = [vp, vp, i64, View, ctypes.POINTER(FilterArgs)]
    lib.dsim_trajgen_workspace.restype = ctypes.c_int64
    lib.dsim_trajgen_workspace.argtypes = [i64, i32]
    lib.dsim_trajgen.argtypes = [vp, vp, ctypes.POINTER(TrajBank), ctypes.POINTER(TrajGenArgs)]
    lib.dsim_traj_sample_bank.argtypes = [vp, vp, i64, ctypes.POINTER(TrajBank), vp, vp, ctypes.c_double, vp, vp, View]
    if lib.dsim_abi_version() != ABI_VERSION or lib.dsim_abi_minor() != ABI_MINOR:
        raise ImportError(f"libdronesim_amd.so ABI {lib.dsim_abi_version()}.{lib.dsim_abi_minor()} != binding {ABI_VERSION}.{ABI_MINOR}")
    _lib = lib
    return lib


def check(code: int) -> None:
    if code != 0:
        raise DsimError(f"dsim error {code}: {load().dsim_strerror(code).decode()}")
