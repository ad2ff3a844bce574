/* dronesim_amd.h — C-ABI of the MI355X-native fleet dynamics + INDI control step.
 *
 * The reference (enac-drones/dronesim, pure Python) has no FFI: its boundary on
 * this path is two Python call surfaces,
 *     gym.Env      reset()/step(action)      dronesim/envs/BaseAviary.py:406-555
 *     BaseControl  computeControl(...)       dronesim/control/BaseControl.py:107-149
 *                                            dronesim/control/INDIControl.py:154-227
 * so the entry points below are what a ctypes binding on the reference side
 * would bind to replace the per-drone Python loops behind those two surfaces
 * (INTEGRATION.md shows that binding).  Each entry point cites the reference
 * code it replaces.
 *
 * Conventions (same as the reference): quaternions xyzw (w at index 3,
 * dronesim/utils/math.py:6,25,47); world frame z-up; angular velocity stored in
 * WORLD frame (BaseAviary.py:730); PWM commands in [pwm_min, pwm_max].
 *
 * Memory: every state / target / action buffer is CALLER-OWNED DEVICE memory
 * (e.g. a torch-ROCm tensor's data_ptr()).  The library allocates nothing per
 * call, never frees caller memory and never synchronises the device; work is
 * stream-ordered on the caller's hipStream_t (passed as void*).  A dsim_ctx owns
 * only the per-type constant table (device copy), a few diagnostic counters and, for
 * fleets with the morphing hexa, the queue of deferred WLS fallbacks (grown when a
 * larger fleet is first seen).  One ctx per device; a ctx may be used from one host
 * thread at a time; the calling thread's current HIP device must be the ctx's device
 * (dsim_create makes it so) and the stream must belong to it.
 *
 * Errors: int return, 0 = OK, negative = library error (DSIM_E_*), positive =
 * hipError_t.  No exceptions or aborts cross the ABI.  There is NO CPU fallback:
 * without a HIP device dsim_create fails.
 */
#ifndef DRONESIM_AMD_H
#define DRONESIM_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSIM_ABI_VERSION 11
#define DSIM_ABI_MINOR 1   /* 1: dsim_type_params ends with collision_sphere (callers built against minor 0 must be rebuilt: the
                              type table's stride grew); dsim_clearance, DSIM_Q_DRONE_CONTACTS.
                              Added since, without a new number because a caller built against 11.1 never sees them (new functions,
                              a new struct, a new enum value; nothing that existed changed size, layout or meaning): the
                              static-obstacle watch, dsim_obstacle_grid_plan / _build, dsim_obstacles_create / _destroy,
                              dsim_obstacle_clearance, dsim_obstacle_grid, DSIM_Q_OBSTACLE_CONTACTS; the depth camera,
                              dsim_obstacle_ray_grid_plan / _build, dsim_obstacles_enable_rays, dsim_depth_image, dsim_camera_params,
                              DSIM_CAM_*, DSIM_SEG_GROUND; the other drones in the camera's images, dsim_depth_image_drones,
                              dsim_depth_image_drones_workspace, dsim_camera_drones, DSIM_SEG_DRONE; the trajectory bank,
                              dsim_trajgen, dsim_trajgen_workspace, dsim_traj_sample_bank, dsim_traj_bank, dsim_trajgen_args,
                              DSIM_TRAJGEN_* (DSIM_TRAJGEN_BAD_CONDITION among them); the swept obstacle watch, dsim_obstacle_sweep, dsim_sweep_args, DSIM_SWEEP_*; obstacle
                              scenes, dsim_scenes_create / _destroy, dsim_obstacle_clearance_scenes, dsim_depth_image_scenes; the
                              swept drone-drone watch, dsim_clearance_sweep, dsim_clearance_sweep_workspace,
                              dsim_clearance_sweep_args; the range scanner, dsim_range_scan, dsim_scan_args, DSIM_SCAN_*; the
                              gate passage watch, dsim_gate_passage, dsim_gate_args, dsim_aperture, DSIM_APERTURE_*, DSIM_GATE_WRAP; the
                              nearest-neighbour observation, dsim_knn, dsim_knn_workspace, dsim_knn_args; the obstacle witness,
                              dsim_obstacle_witness, dsim_obstacle_witness_scenes, dsim_witness_args, DSIM_WITNESS_BODY_FRAME; line
                              of sight, dsim_line_of_sight, dsim_sight_args, DSIM_SIGHT_GROUND; moving scenes,
                              dsim_scenes_motion_set, dsim_scenes_move, dsim_scenes_read, dsim_scene_motion; the velocity of the
                              witness on moving scenes, dsim_scenes_move_twist, dsim_obstacle_witness_scenes_vel; obstacle witnesses,
                              dsim_obstacle_witnesses, dsim_obstacle_witnesses_scenes, dsim_witnesses_args, DSIM_WITNESSES_MAX; the
                              velocity safety filter, dsim_velocity_filter, dsim_filter_args, DSIM_FILTER_*; line of sight
                              among the drones, dsim_line_of_sight_drones; corridor clearance, dsim_corridor_clearance,
                              dsim_corridor_args, DSIM_CORRIDOR_GROUND */
#define DSIM_MAX_ACT 6     /* actuators per vehicle (quad 4, morphing hexa 6) */
#define DSIM_MAX_TYPES 8

/* ---- state layout ---------------------------------------------------------
 * Fleet state is ONE fp32 device array in "blocked SoA":
 *     addr(field f, drone i) = base + (i / block) * block_stride
 *                                   + f * field_stride + (i % block)
 * Plain SoA [F][n_pad] is block = n_pad, field_stride = n_pad; the wave-tiled
 * form [n_pad/64][F][64] is block = 64, field_stride = 64, block_stride = F*64.
 * n_pad must be a multiple of 64 (padding lanes are computed and ignored).
 *
 * Field order (DSIM_F_*): the 13 rigid-body floats the reference reads back
 * from Bullet (BaseAviary.py:718-732) followed by the controller memory the
 * reference keeps on each INDIControl instance (INDIControl.py:109-146).      */
enum {
  DSIM_F_POS = 0,        /* 3  world position                                   */
  DSIM_F_QUAT = 3,       /* 4  xyzw                                            */
  DSIM_F_VEL = 7,        /* 3  world linear velocity                           */
  DSIM_F_ANGVEL = 10,    /* 3  world angular velocity                          */
  DSIM_F_LAST_VEL = 13,  /* 3  INDIControl.last_vel   (INDIControl.py:130,291) */
  DSIM_F_LAST_RATES = 16,/* 3  INDIControl.last_rates (INDIControl.py:125,442) */
  DSIM_F_LAST_THRUST = 19,/*1  INDIControl.last_thrust(INDIControl.py:127,455) */
  DSIM_F_CMD = 20,       /* n_act  INDIControl.cmd == the action fed to step() */
  DSIM_NF_QUAD = 24,     /* fields for a 4-actuator fleet                      */
  DSIM_NF_HEXA = 26      /* fields for a 6-actuator (or mixed) fleet           */
};

/* Per-step targets, same blocked-SoA addressing, 10 fields:
 * target_pos3, target_vel3, target_acc3, target_yaw (only target_rpy[2] is read
 * by the reference, INDIControl.py:341; target_rpy_rates is ignored, :404-410) */
enum { DSIM_T_POS = 0, DSIM_T_VEL = 3, DSIM_T_ACC = 6, DSIM_T_YAW = 9, DSIM_NT = 10 };

typedef struct dsim_view {
  float*  base;          /* device pointer                                      */
  int64_t n_pad;         /* padded drone count, multiple of 64                  */
  int64_t block;         /* drones per block (n_pad for plain SoA, or 64)       */
  int64_t field_stride;  /* floats between consecutive fields inside a block    */
  int64_t block_stride;  /* floats between consecutive blocks                   */
  int32_t n_fields;      /* DSIM_NF_QUAD / DSIM_NF_HEXA / DSIM_NT               */
  int32_t _pad;
} dsim_view;

/* ---- per-type constants (host side, fp64; converted to fp32 on upload) -----
 * Filled by the host from the vehicle URDF exactly as the reference does
 * (BaseAviary._parseURDFParameters, BaseAviary.py:2041-2140;
 *  INDIControl._parseURDFControlParameters, INDIControl.py:55-106).            */
enum {
  DSIM_KIND_QUAD = 0,          /* quad physics (BaseAviary.py:1477-1543) + the quad INDI law (INDIControl.py)                    */
  DSIM_KIND_HEXA6DOF = 1,      /* morphing-hexa physics (BaseAviary.py:1389-1457) + the 6-DOF INDI law with WLS allocation
                                  (INDIControl_6DOF.py): hexa_6DOF.urdf                                                        */
  DSIM_KIND_HEXA_QUADLAW = 2   /* morphing-hexa physics + the QUAD law on six actuators — G1 is 4 x 6, alloc = pinv(G1/0.05)
                                  is 6 x 4, every one of the six commands is incremented and clipped (INDIControl.py:457-487
                                  with actuator_nr = 6): hexa_6DOF_simple.urdf:25-34, examples/fly_hexa_6DOF_simple.py:18   */
};

typedef struct dsim_type_params {
  int32_t kind;                       /* DSIM_KIND_*                                        */
  int32_t n_act;                      /* 4 | 6   (indi actuator_nr); 6 for both hexa kinds   */
  double  mass;                       /* total rigid-body mass used by the integrator       */
  double  inertia[3];                 /* principal moments (URDF ixx,iyy,izz)               */
  double  kf, km;                     /* thrust / drag-torque coefficients                  */
  double  pwm2rpm_scale[DSIM_MAX_ACT];
  double  pwm2rpm_const[DSIM_MAX_ACT];
  double  pwm_min[DSIM_MAX_ACT], pwm_max[DSIM_MAX_ACT];
  double  rotor_pos[DSIM_MAX_ACT][3]; /* point of force application, body frame (link inertial origin) */
  double  rotor_axis[DSIM_MAX_ACT][3];/* thrust direction, body frame ((0,0,1) for quads)   */
  double  rotor_spin[DSIM_MAX_ACT];   /* sign of km*rpm^2 in the yaw torque (BaseAviary.py:1527: -,+,-,+) */
  double  G1[DSIM_MAX_ACT][DSIM_MAX_ACT];    /* control effectiveness, [n_out][n_act]       */
  double  alloc[DSIM_MAX_ACT][DSIM_MAX_ACT]; /* quad: pinv(G1/0.05) [n_act][n_out] (INDIControl.py:459);
                                                hexa: M1 of the WLS first iteration, u_opt = M1 v + M4 u0 */
  double  alloc2[DSIM_MAX_ACT][DSIM_MAX_ACT];/* hexa: M4 (see DESIGN.md "WLS allocation"); quad: unused  */
  double  kp_pos, kd_pos;             /* indi_guidance_gains                                */
  double  att_gain[3], rate_gain[3];  /* indi_att_gains att / rate                          */
  double  gravity;                    /* 9.8 (BaseAviary.py:182,673)                        */
  double  lin_damping, ang_damping;   /* Bullet multibody defaults 0.04f                    */
  double  max_coord_vel;              /* Bullet multibody default 100                       */
  double  drag_coeff[3];              /* BaseAviary._drag coefficients (formula P6)         */
  double  gnd_eff_coeff, prop_radius, gnd_eff_h_clip;   /* formula P7                       */
  double  dw_coeff[3];                /* formula P8                                         */
  double  max_speed_kmh;              /* URDF max_speed_kmh (VelocityAviary speed limit)    */
  /* bounding cylinder of the vehicle's collision shapes about its body z axis (URDF <collision>; robobee: the
   * 0.15 m x 0.1 m cylinder, robobee.urdf:72-77): radius, and extent below the centre of mass.  The reference loads
   * plane.urdf with collisions on (BaseAviary.py:680).  DSIM_OPT_PLANE enforces that plane on this cylinder (general
   * kernels); without the option the flight kernels do not model it, and every drone-step that ends with this
   * cylinder reaching z <= 0 is counted instead (DSIM_Q_GROUND_CONTACTS), so that a caller knows when a flight has
   * left the domain in which results are comparable.  0 = no watch and no contact for this type.  */
  double  collision_radius, collision_below;
  double  contact_friction;           /* DSIM_OPT_PLANE: Coulomb coefficient against the plane (PyBullet combines by product:
                                         plane.urdf's lateral_friction 1.0 x the vehicle's default 0.5)                 */
  /* Body-frame vector from the centre of mass the physics integrates to the point whose position and velocity the state
   * block holds — what p.getBasePositionAndOrientation / getBaseVelocity report (BaseAviary.py:726-732): the BASE
   * link's centre of mass.  Zero for the single-body quads; the morphing hexa is flown as the rigid composite of its 19
   * links, whose centre of mass lies 11 mm below the base link's (hexa_6DOF.urdf).  mass, inertia, rotor_pos and the
   * collision cylinder are about the integrated centre of mass. */
  double  base_offset[3];
  /* Physics.DYN (BaseAviary._dynamics, BaseAviary.py:1767-1828: the reference's own explicit rigid-body model, four-rotor
   * types only): the URDF's `arm` attribute L (BaseAviary.py:2058; robobee / tello 0.0635 — NOT the rotor links' lever arms
   * the PYB force map uses) and which of the two mixers of :1794-1803 turns the rotor forces into roll / pitch torques. */
  double  arm;
  int32_t dyn_mixer;                  /* DSIM_DYN_MIXER_X: (f0+f1-f2-f3, -f0+f1+f2-f3) L/sqrt 2 (DroneModel.CF2X, :1794-1800);
                                         DSIM_DYN_MIXER_PLUS: (f1-f3, -f0+f2) L (CF2P / HB, :1801-1803)                    */
  int32_t _pad_dyn;
  /* Bounding sphere of the vehicle's collision shapes: the radius, about the integrated centre of mass, of the smallest sphere
   * the builder can certify to contain every <collision> shape of every link in the URDF rest pose (and the lower rim of the
   * bounding cylinder above, which carries the contact points of DSIM_OPT_PLANE).  The reference flies in a Bullet world where
   * the vehicles' collision shapes act on each other (BaseAviary.py:681-694 loads every vehicle with collisions on); this
   * library integrates every drone alone, and every pair of drones whose spheres overlap is counted instead
   * (dsim_clearance, DSIM_Q_DRONE_CONTACTS), so that a caller knows when a flight has left the domain in which results are
   * comparable.  The test is one-sided in the useful direction: where no two spheres overlap, Bullet's narrow phase would
   * have found no drone-drone contact either; an overlap of spheres need not be one of shapes.  0 = the type takes no part in
   * the watch.  (At the END of the struct: DSIM_ABI_MINOR 1 appended it.) */
  double  collision_sphere;
} dsim_type_params;
enum { DSIM_DYN_MIXER_X = 0, DSIM_DYN_MIXER_PLUS = 1 };

/* ---- step options ---------------------------------------------------------- */
enum {
  DSIM_OPT_DRAG        = 1u << 0,   /* add formula P6 (BaseAviary.py:1705-1732)            */
  DSIM_OPT_GROUND      = 1u << 1,   /* add formula P7 (BaseAviary.py:1648-1699)            */
  DSIM_OPT_BCAST_TGT   = 1u << 2,   /* targets view holds ONE drone's targets, broadcast   */
  DSIM_OPT_CHAINED     = 1u << 3,   /* dsim_step only.  The caller asserts that the stored controller memory is
                                       the one the previous dsim_step / dsim_control left on the SAME rigid state,
                                       i.e. last_vel == vel and last_rates == R(quat)^T ang_vel.  Both are then
                                       recomputed from the rigid state instead of being read, and are NOT written
                                       back (6 of the 24 fields: 184 instead of 232 bytes of traffic per
                                       drone-step).  The six fields are stale until dsim_materialize is called. */
  /* -- tuning knobs (results do not depend on them; the library reads no environment variables) --------------- */
  DSIM_OPT_STREAM_ON   = 1u << 4,   /* force nontemporal (streaming) loads/stores of the state; default: on when one
                                       step's traffic exceeds what the 256 MB Infinity Cache keeps between steps   */
  DSIM_OPT_STREAM_OFF  = 1u << 5,   /* force the default cache policy                                              */
  /* (bits 6-9, 12, 13: A/B knobs of measured-and-rejected kernel forms; honoured only by a library built with
   * tools/variants/ in the git history up to round 5 — the library ignores them)                              */
  /* -- physics (changes results) ------------------------------------------------------------------------------------ */
  DSIM_OPT_PLANE       = 1u << 10,  /* ground plane z = 0 with contact and friction, as the reference's world has
                                       (BaseAviary.py:680 loads plane.urdf, collisions on).  A PRODUCT-DEFINED contact
                                       model (eight body-fixed rim points of the vehicle's collision cylinder, 24
                                       sequential-impulse sweeps, ERP 0.2, restitution 0, Coulomb friction): Bullet's own
                                       contact pipeline cannot be restated or pinned here.  Served
                                       by the k_step_plane / k_physics_plane / k_adaptor kernels; every airframe kind;
                                       not combined with DSIM_OPT_CHAINED.                                            */
  /* -- numbering of the per-drone arrays beside the state (dsim_physics, dsim_control2) -------------------------------------
   * A host class may STORE a heterogeneous fleet type-major (runs) behind its caller's numbering (dsim_step_args.drone_id).
   * With this bit the per-drone arrays those two entry points take and return besides the state and target views — the
   * action, obs_out, cmd_out, pos_e_out, yaw_e_out — are indexed by the CALLER's drone number drone_id[i] instead of the
   * storage slot i: Env.step() returns its observation rows and computeControl() its triple in the caller's order with no
   * second pass over them (BaseAviary.py:547-555, INDIControl.py:227), and the command goes from the one to the other as
   * it is.  last_action_out stays in storage order (it is the env's own memory, read back by dsim_observe).  Needs
   * drone_id and a fleet that the run kernels serve (runs given or one type; no noise replay, no drag / ground / plane
   * option): DSIM_E_UNSUPPORTED otherwise.  The first call with a NEW set of runs builds a small table the ctx keeps: it
   * waits for the device and may allocate, so it must not sit inside a stream capture (every later call with the same
   * runs may).                                                                                                        */
  DSIM_OPT_CALLER_IO   = 1u << 14,
  /* dsim_physics / dsim_step_adaptor: `action` is row-major [n][4] — one 4-vector per drone, as Env.step is handed it
   * (CtrlAviary.py:258-263, VelocityAviary.py:221-264, RPYTAviary.py:181-193) — instead of field-major [4][n_pad]; 16-byte
   * aligned.  Served by the one-launch forms (homogeneous quad fleet in whole tiles, no physics option, no downwash inputs):
   * DSIM_E_UNSUPPORTED otherwise.                                                                                        */
  DSIM_OPT_ACTION_ROWS = 1u << 15,
  /* -- Physics.DYN (changes results) -----------------------------------------------------------------------------------
   * dsim_physics / dsim_step integrate with the reference's OWN explicit model instead of the restated Bullet step:
   * BaseAviary._dynamics (BaseAviary.py:1767-1828; dispatch :525-527, no p.stepSimulation :541-543), per physics sub-step
   *     rpm = pwm2rpm_scale * clipped action + pwm2rpm_const   (the fork's PWM -> RPM map, BaseAviary.py:1487-1490; the
   *                                                              function's argument is documented as RPMs, :1770-1775)
   *     rpy = getEulerFromQuaternion(quat)                      (:513-520 / :547 refresh self.rpy from the engine, :729)
   *     thrust = sum kf rpm^2 along body z (R from quat, :1786-1790);  force_world = R thrust - (0, 0, G M)
   *     torques = mixer(forces; L) , z = -t0 + t1 - t2 + t3 (t = km rpm^2);  torques -= rpy_rates x (J rpy_rates)
   *     vel += dt force_world / M;  rpy_rates += dt J^-1 torques;  pos += dt vel;  rpy += dt rpy_rates
   *     quat = getQuaternionFromEuler(rpy)                      (:1814-1819)
   * There is no rotor noise in this model (noise_seed / noise_replay are ignored) and no damping.  Four-rotor types only
   * (both mixers read forces[0..3]): DSIM_E_UNSUPPORTED for a table with a six-actuator type, and with the drag / ground /
   * plane options, ext_force, waypoint tables, n_steps > 1, DSIM_OPT_CHAINED, _CALLER_IO, _ACTION_ROWS, bin_next.
   * The model's own state `rpy_rates` (BaseAviary.py:670-671, 1828: an env attribute beside pos / quat / vel) lives in
   * dsim_step_args.dyn_rpy_rates, REQUIRED with this bit.  The angular-velocity fields of the state block hold what
   * p.getBaseVelocity reports after the step: the reference stores the placeholder (-1, -1, -1) there ("ang_vel not computed
   * by DYN", :1821-1826), so that is what observations show and what a controller reads — bit for bit the reference's
   * behaviour, and the reason its INDI controller cannot close a loop on Physics.DYN.                                      */
  DSIM_OPT_DYN         = 1u << 16,
  /* With DSIM_OPT_DYN: a PRODUCT-DEFINED deviation that makes the mode flyable.  The angular-velocity fields receive
   * R(quat_new) rpy_rates_new instead of the placeholder — the world-frame image of the rates, which the model's own torque
   * equation treats as body rates (rpy_rates x J rpy_rates, :1805).  Off = the reference's (-1, -1, -1).                  */
  DSIM_OPT_DYN_BODY_RATES = 1u << 17,
  /* -- rotor noise (changes results) -------------------------------------------------------------------------------------
   * WHICH of the two lattices the rotor-noise normals are drawn on (see dsim_step_args.noise_seed).  A function of the launch
   * arguments alone, never of the kernel that happens to serve the launch:
   *   neither bit   phys_substeps == 1: the FINE lattice; phys_substeps > 1: the COARSE one
   *   _NOISE_FINE   the fine lattice at any sub-step count: 16 + 16 bits per Box-Muller pair, one Threefry block per quad sub-step
   *                 (two per hexa sub-step), radius and direction evaluated.  Free on launches of one sub-step (bound by HBM);
   *                 a launch of several sub-steps on it leaves the looped fast kernels for the general ones
   *   _NOISE_COARSE the coarse lattice at any count: 8 + 8 bits per pair, one block per TWO quad sub-steps (one per hexa
   *                 sub-step), radius and direction from 256-entry tables in the kernels that loop over sub-steps (bound by
   *                 vector issue).  A caller that splits one Env.step of several sub-steps into single-sub-step launches
   *                 (the per-sub-step neighbour downwash) passes the bit of the lattice its unsplit step would draw
   * Both bits: DSIM_E_ARG.                                                                                                */
  DSIM_OPT_NOISE_FINE  = 1u << 18,
  DSIM_OPT_NOISE_COARSE = 1u << 19,
  /* -- traffic (results do not depend on it) -------------------------------------------------------------------------- */
  DSIM_OPT_TGT_CONST   = 1u << 20,  /* The caller asserts that, for every drone, the target fields of the groups set in
                                       dsim_step_args.tgt_const_mask (bit 0 pos, 1 vel, 2 acc, 3 yaw) hold exactly the
                                       values of dsim_step_args.tgt_const (pos3 vel3 acc3 yaw, bit for bit).  The library
                                       MAY take those fields from the arguments instead of reading the targets view, and
                                       may ignore the hint; the view must hold the values either way.  Honoured, with the
                                       mask exactly 0xE (pos per drone, vel / acc / yaw constant), by the whole-tile quad
                                       kernels of dsim_step (plain targets: no waypoint table, n_steps 1, no explicit
                                       action) and of dsim_control2: 7 of the 10 target floats are not read, 28 bytes less
                                       per drone-step (232 -> 204, chained 184 -> 156, control 212 -> 184).  Every other
                                       kernel and mask reads the view as without the bit.  A target view that repeats
                                       with a period is described by dsim_step_args.tgt_period (no option bit).         */
  DSIM_OPT_MEM_DERIVED = 1u << 21,  /* dsim_step only.  The caller asserts that in the stored block last_vel == vel and
                                       last_rates == R(quat)^T ang_vel bit for bit, as the previous dsim_step / dsim_control
                                       on this rigid state left them (the assertion of DSIM_OPT_CHAINED).  The library MAY
                                       then recompute the six fields instead of reading them, and may ignore the hint; it
                                       WRITES them as without the bit, so the block is current after every launch and
                                       nothing needs dsim_materialize.  Honoured by the whole-tile kernels of one physics
                                       sub-step with plain targets and no explicit action: the quad ones where
                                       DSIM_OPT_TGT_CONST is honoured too (192 -> 168 bytes per drone-step with a period)
                                       and the morphing-hexa ones (248 -> 224).  Every other kernel reads the fields (the
                                       quad kernels that read all ten target fields would lose a wave per SIMD).  With DSIM_OPT_CHAINED the bit is redundant
                                       and ignored.  Not valid behind dsim_physics or a host write of the rigid state.   */
  /* -- scheduling (results do not depend on it) ---------------------------------------------------------------------- */
  DSIM_OPT_DEFER_FALLBACK = 1u << 11 /* dsim_step / dsim_control2 of a table with a morphing hexa do NOT launch the deferred
                                       WLS fallback pass behind the step; the caller launches dsim_wls_fallback itself —
                                       on any stream ordered behind this call — before the commands are next read
                                       (INDIControl_6DOF.py:600-631 finishes the allocation inside computeControl; here its
                                       rare active-set tail may overlap the next Env.step's neighbour query).            */
};

/* A run of consecutive drones of one type (type-major storage of a heterogeneous fleet). */
typedef struct dsim_type_run {
  int64_t first;            /* first drone of the run (any index: the launch starts at the 256-drone tile that
                               holds it and the lanes in front of `first` retire)                        */
  int64_t count;            /* drones in the run                                                        */
  int32_t type;             /* index into the ctx type table                                            */
  int32_t _pad;
} dsim_type_run;

typedef struct dsim_step_args {
  int32_t  phys_substeps;   /* AGGR_PHY_STEPS: Bullet sub-steps per Env.step (BaseAviary.py:510) */
  float    dt_phys;         /* 1/SIM_FREQ  (BaseAviary.py:675)                                   */
  float    dt_ctrl;         /* control_timestep handed to computeControl (fly_INDI.py:231)       */
  uint32_t options;         /* DSIM_OPT_*                                                        */
  uint64_t noise_seed;      /* 0 = rotor noise off; else counter-based noise, N(0, .01) on the rotor forces and N(0, .001) on
                               the rotor moments per sub-step (BaseAviary.py:1518-1525, 1429-1432).  The reference draws
                               np.random.normal from the unseeded global generator; here the stream is PRODUCT-DEFINED:
                               Threefry4x32-12 keyed by the seed, counter = (drone, block), Box-Muller pairs on a LATTICE of
                               cell centres (u = (k + 1/2) / K: no draw is exactly 0) —
                                 fine      16 + 16 bits per pair: 2^32 distinct pairs, |n| <= 4.855 sigma (mass 1.2e-6 beyond),
                                           kurtosis 2.9998, Kolmogorov distance from the normal distribution below what 1e7 draws
                                           resolve.  The lattice of every launch of ONE sub-step (BASELINE's metric) and of
                                           DSIM_OPT_NOISE_FINE;
                                 coarse    8 + 8 bits per pair: 256 radii x 256 directions = 65 536 distinct pairs, |n| <= 3.535
                                           sigma (the reference's tails are unbounded: mass 4.1e-4 beyond 3.535 sigma; 2.75e-3 instead of 2.70e-3 beyond 3), variance
                                           exactly sigma^2 (the radius is rescaled), kurtosis 2.977 instead of 3, no atoms,
                                           Kolmogorov distance 1.4e-3 from the normal distribution.  The lattice of launches of
                                           SEVERAL sub-steps (the examples' five: kernels bound by vector issue) and of
                                           DSIM_OPT_NOISE_COARSE.
                               WHAT is drawn: a quad's eight normals per sub-step, one per rotor force and rotor moment as the
                               reference draws them (BaseAviary.py:1518-1521).  The six-actuator kinds draw SIX: the reference's twelve
                               per-rotor normals (:1429-1430) enter the rigid composite only through the body wrench they add up
                               to, a Gaussian 6-vector; the stream draws that vector (W = L z, L the Cholesky factor of its
                               covariance, computed from the type's rotor geometry by dsim_create) — the same distribution of the
                               wrench, hence of the flight, from half the bits (tests/test_noise_distribution.py:
                               test_hexa_wrench_noise_has_the_covariance_of_the_per_rotor_noise).  Per-rotor normals remain an
                               input: noise_replay.
                               tests/test_noise_distribution.py measures both lattices against N(0, 1) (Kolmogorov distance, moments,
                               tail mass, the absence of exact zeros) over 1e7 draws; dsim_noise_draw hands out the normals.   */
  uint64_t step_index;      /* env-step counter, mixed into the noise counter                    */
  const float* noise_replay;/* nullable; [phys_substeps][2*n_act][n_pad] recorded normals (tests)*/
  const uint8_t* type_id;   /* nullable; per-drone index into the ctx type table (mixed fleets)  */
  const float* action;      /* nullable; SoA [n_act][n_pad].  dsim_step: action for the physics part
                               instead of the stored cmd (first iteration of the example loop: the
                               initial action 0.4, fly_INDI.py:214, while INDIControl.cmd starts at 0).
                               dsim_physics: the action of Env.step(action); NULL = stored cmd.      */
  /* -- waypoint-table targets (examples/fly_INDI_TrajectoryTrack.py:178-189, 242-256) ------------
   * wp_table non-NULL: the targets view is ignored; drone i tracks row wp_counter[i] of the table
   * (row-major [n_wp][10] = pos3 vel3 acc3 yaw, device memory, read-only; 1200 rows = 48 KB for the
   * example) plus its own position offset, and after every control evaluation the counter advances
   * by one and wraps to 0 after n_wp-1, as the example does.                                        */
  const float* wp_table;
  int32_t*     wp_counter;  /* [n_pad] device, in-out                                              */
  const float* wp_offset;   /* nullable; SoA [3][n_pad] added to the table's target position       */
  int32_t      n_wp;
  /* -- multi-step launches -------------------------------------------------------------------------
   * n_steps > 1: dsim_step runs that many consecutive [Env.step + computeControl] iterations in ONE
   * launch with the state held in registers (step_index, step_index+1, ...); targets stay fixed
   * unless they come from the waypoint table.  0 is treated as 1.                                   */
  int32_t      n_steps;
  /* -- external body-frame force --------------------------------------------------------------------
   * nullable; SoA [3][n_pad]: extra force applied at the COM in the LINK frame every sub-step, e.g.
   * the neighbour downwash of dsim_downwash (BaseAviary.py:1755-1762 applies it to link 4 = COM).   */
  const float* ext_force;
  /* -- graph replay -----------------------------------------------------------------------------------
   * nullable device pointer; the effective env-step counter is step_index + *step_index_dev.  Lets a
   * captured hipGraph of [dsim_step, dsim_counter_add] pairs be replayed without repeating the noise
   * stream (kernel arguments are frozen at capture time, device memory is not).                        */
  const uint64_t* step_index_dev;
  /* -- type-major storage ------------------------------------------------------------------------------
   * nullable HOST array: the fleet is stored as n_runs runs of one type each (type_id[], still required by
   * the other entry points, must agree).  dsim_step then launches the single-type kernel of each run's kind
   * over that run — the mixed-fleet kernel, which has to hold every law and re-sort each tile by type, is
   * not needed.  Drones outside every run are not stepped.                                              */
  const dsim_type_run* runs;
  int32_t n_runs;
  /* -- fused observation (dsim_physics only) -----------------------------------------------------------------------
   * obs_out nullable: the rows of dsim_observe (BaseAviary._getDroneStateVector, BaseAviary.py:764-790) of the state
   * AFTER the step with the applied (clipped) action echoed, written by the same launch: what Env.step() returns
   * (BaseAviary.py:547-555).  Row-major [n][obs_width], obs_width = 16 + n_act of the ctx.                           */
  int32_t obs_width;
  float*  obs_out;
  /* -- neighbour grid for the NEXT Env.step (dsim_step only) --------------------------------------------------------
   * nullable: the grid description of the next dsim_downwash call.  The step kernel then appends the NEW position of
   * every local drone to its cell's bucket while the position is still in registers (or, when that call will re-use kept
   * candidate lists — its keep field says DSIM_DW_KEEP_REUSE —, refreshes the drone's bucket entry in place), and that
   * dsim_downwash call (same workspace and shape, args->prebinned = 1) skips the binning launch for the local drones.  Honoured on the
   * bucket form of the grid only (dsim_downwash_prebin_ok() != 0); otherwise ignored.                                */
  const struct dsim_downwash_args* bin_next;
  /* -- storage order --------------------------------------------------------------------------------------------------
   * nullable device array [n_pad]: the index of storage slot i in the CALLER's numbering.  Drones are independent, so a
   * host class may store a heterogeneous fleet type-major (runs) whatever order its caller uses; the rotor-noise
   * counter is then keyed by drone_id[i] instead of i, so that a drone draws the same noise wherever it is stored.   */
  const int32_t* drone_id;
  /* -- Physics.DYN ------------------------------------------------------------------------------------------------------
   * device SoA [3][n_pad], in-out; required with DSIM_OPT_DYN, ignored otherwise: BaseAviary.rpy_rates (BaseAviary.py:670-671
   * zeroed by _housekeeping, :1785 read, :1828 written by _dynamics).  Caller-owned like every other per-drone array.  */
  float* dyn_rpy_rates;
  /* -- constant target groups (DSIM_OPT_TGT_CONST; zeroed arguments: no hint) ---------------------------------------------- */
  uint32_t tgt_const_mask;  /* bit 0 pos, 1 vel, 2 acc, 3 yaw: the groups whose fields hold tgt_const for every drone      */
  float    tgt_const[10];   /* pos3 vel3 acc3 yaw; the entries of the groups outside the mask are ignored                 */
  /* -- periodic targets (traffic only: results do not depend on it; zeroed arguments: no hint) ----------------------------
   * 0: no hint.  Otherwise the caller asserts that, for every drone i < n_pad, every field of the targets view holds the
   * value (bit for bit) the same field holds for drone i mod tgt_period: env replicas that share a task, or a constant group
   * (a period of 1 taken up to a whole tile).  The library MAY then read the targets of the first period only, and may ignore
   * the hint; the whole view must hold the values either way.  Honoured on a per-drone view (no DSIM_OPT_BCAST_TGT) without a
   * waypoint table, when tgt_period is a multiple of 256 and of the view's block (no condition for plain SoA), divides n_pad
   * and is below it; otherwise ignored, never an error.  The kernels that honour it are the whole-tile quad kernels of
   * dsim_step with plain targets (n_steps 1, no explicit action), with or without DSIM_OPT_TGT_CONST: 12 (with it) or 40
   * (without it) bytes per drone-step less read from HBM, the first period staying in L2.  Every other kernel — the hexa,
   * mixed, run and general kernels, dsim_control2, dsim_physics — reads the whole view.                                 */
  int64_t  tgt_period;
} dsim_step_args;

typedef struct dsim_ctx dsim_ctx;

/* library / build info */
int         dsim_abi_version(void);
int         dsim_abi_minor(void);
const char* dsim_strerror(int code);

/* ctx: uploads the type table to `device`.  Replaces the per-instance parsing in
 * BaseAviary.__init__ (BaseAviary.py:200-235) + INDIControl.__init__ (:34-52).   */
int dsim_create(dsim_ctx** out, int device, const dsim_type_params* types, int n_types);
int dsim_destroy(dsim_ctx* ctx);

/* Plain device allocations straight from the driver (hipMalloc / hipFree on the ctx's device), outside any caching
 * allocator of the host framework.  (No counterpart in the reference.)  For host classes that choose WHERE a fleet-sized
 * array lies by trial (dronesim_amd/placement.py): candidates that are not kept go back to the driver at once, and no
 * framework-wide cache has to be emptied to walk through device memory.  The caller owns what it allocates; dsim_dev_free
 * takes ctx == NULL too (a block may outlive the ctx it was allocated through: dsim_destroy frees nothing of the caller's). */
int dsim_dev_alloc(dsim_ctx* ctx, int64_t bytes, void** out);
int dsim_dev_free(dsim_ctx* ctx, void* ptr);

/* reset(): BaseAviary._housekeeping (BaseAviary.py:640-714) + INDIControl.reset
 * (INDIControl.py:109-146).  init_* are device SoA [3][n_pad]; init_vel and
 * init_cmd nullable (zeros / controller reset value).  Writes every field.       */
int dsim_reset(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state,
               const float* init_pos, const float* init_rpy, const float* init_vel,
               const float* init_cmd, const uint8_t* type_id);

/* One fused Env.step() + computeControl() for every drone:
 *   physics x phys_substeps with the stored cmd  (BaseAviary.py:510-545, 1477-1543 | 1389-1457,
 *                                                  p.stepSimulation :542)
 *   then the INDI law on the fresh state          (INDIControl.py:154-227)
 * i.e. the body of the example loop (examples/fly_INDI.py:223-239).             */
int dsim_step(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, dsim_view targets,
              const dsim_step_args* args);

/* Pre-allocates what the ctx owns for fleets of up to n_pad drones (today: the deferred-WLS-fallback queue of
 * tables that hold a morphing hexa; a no-op otherwise), so that no later call allocates or synchronises — which
 * hipGraph capture of dsim_step requires. */
int dsim_reserve(dsim_ctx* ctx, void* stream, int64_t n_pad);

/* *counter += inc on the stream (a one-thread kernel; the companion of step_index_dev). */
int dsim_counter_add(dsim_ctx* ctx, void* stream, uint64_t* counter, uint64_t inc);

/* Rewrites last_vel / last_rates from the rigid state (ends a DSIM_OPT_CHAINED sequence). */
int dsim_materialize(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state);

/* Env.step() only: physics sub-steps with args->action (clipped in-kernel as
 * CtrlAviary._preprocessAction does, CtrlAviary.py:258-263; NULL = stored cmd).
 * The clipped action is written to last_action_out (SoA [n_act][n_pad], nullable):
 * the env's last_clipped_action (BaseAviary.py:545).  The controller memory
 * (state cmd fields) is NOT touched: env and controller are separate objects in
 * the reference.                                                              */
int dsim_physics(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state,
                 float* last_action_out, const dsim_step_args* args);

/* Env.step() of the reference's two alternate action adaptors, which run (part of) the INDI law
 * INSIDE _preprocessAction and then the physics:  control on the current state first, then
 * phys_substeps with the new command.  action: SoA [4][n_pad].
 *   DSIM_ADAPT_VELOCITY  VelocityAviary._preprocessAction (VelocityAviary.py:221-264): action =
 *       (vx, vy, vz, speed fraction); full INDI with target_pos = current position, target yaw =
 *       current yaw, target_vel = SPEED_LIMIT |a3| unit(a0..2)
 *   DSIM_ADAPT_RPYT      RPYTAviary._preprocessAction (RPYTAviary.py:181-193): action = (p, q, r
 *       body-rate set-points, thrust) fed to _INDIRateControl only
 * dt_ctrl of args is the control_timestep (AGGR_PHY_STEPS * TIMESTEP).  Quad types only.
 * last_action_out (nullable, SoA [4][n_pad]) receives the applied command (last_clipped_action).
 * args->obs_out (nullable, [n][20], obs_width = 20): Env.step's return value, the rows of _computeObs for the NEW state
 * (BaseAviary.py:547-555, 780-790) — written by the same launch for a homogeneous fleet in whole tiles (which also takes the
 * action row-major, DSIM_OPT_ACTION_ROWS), by the observation kernel behind the step otherwise. */
enum { DSIM_ADAPT_VELOCITY = 0, DSIM_ADAPT_RPYT = 1 };
int dsim_step_adaptor(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const float* action,
                      int32_t mode, float* last_action_out, const dsim_step_args* args);

/* computeControl() only (INDIControl.py:154-227 / INDIControl_6DOF.py:259-336):
 * reads the rigid fields, updates the controller-memory fields and cmd.
 * pos_e_out [3][n_pad] and yaw_e_out [n_pad] nullable.                           */
int dsim_control(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, dsim_view targets,
                 const dsim_step_args* args, float* pos_e_out, float* yaw_e_out);
/* The same, and the new command is also written to cmd_out (nullable, SoA [n_act][n_pad]): the first return value of
 * computeControl as a plain array, in the layout Env.step's action (dsim_step_args.action) takes — the command goes
 * from the controller to the next Env.step without a copy. */
int dsim_control2(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, dsim_view targets,
                  const dsim_step_args* args, float* pos_e_out, float* yaw_e_out, float* cmd_out);

/* _getDroneStateVector (BaseAviary.py:764-790): writes the reference's 20/22-wide
 * observation rows [pos3 quat4 rpy3 vel3 ang_v3 last_action] as row-major
 * [n][obs_width] fp32, obs_width = 16 + n_act.  last_action: SoA [n_act][n_pad]
 * (the env's last_clipped_action); NULL = the stored cmd.                        */
int dsim_observe(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const float* last_action,
                 float* obs_out, int32_t obs_width);

/* Trajectory sampler on device: trajGenerator.get_des_state(t) (dronesim/utils/trajGen.py:108-126,
 * polyder trajutils.py:13-21) per drone, including the stateful yaw-from-velocity rule
 * (trajGen.py:128-143), written into a targets view that dsim_step / dsim_control then consume.
 * coeffs: device, row-major [n_seg*10][3] fp64 (trajGenerator.coeffs); ts: device [n_seg+1] fp64.
 * t: device [n_pad] fp64 in-out, each drone's own trajectory time; advanced by dt_advance after
 * sampling (the example samples at 1/control_freq).  yaw_state: device SoA [3][n_pad] fp64 in-out
 * (yaw, heading_x, heading_y), zero-initialised like trajGenerator; fp64 because the rule integrates
 * acos() of nearly parallel unit headings, whose error is sqrt(eps) per step.  offset: nullable fp32
 * SoA [3][n_pad] added to the sampled position.  Polynomials (degree 9, t up to ~7 s) in fp64.
 * At zero horizontal velocity the reference's heading is 0/0 and its yaw NaN from that sample on
 * (np.sign of a NaN cross product): so is this one's — yaw_state[0] and the yaw target become NaN and stay. */
int dsim_traj_sample(dsim_ctx* ctx, void* stream, int64_t n, const double* coeffs, const double* ts,
                     int32_t n_seg, double* t, double dt_advance, double* yaw_state, const float* offset,
                     dsim_view targets_out);

/* ---- trajectory bank: a course per drone --------------------------------------------------------------------------
 * K min-snap courses side by side in caller-owned device memory, all fp64, course-minor ("K_pad apart") so that lanes
 * with neighbouring courses read neighbouring words:
 *     coeffs[((seg * 10 + j) * 3 + d) * K_pad + k]    seg < L_max - 1, j < 10 ascending powers, d < 3
 *     ts[seg * K_pad + k]                             seg < L_max: the reference's TS, cumulative, ts[0] = 0
 *     n_seg[k]                                        int32, 1 .. L_max - 1; 0 marks a course that could not be made
 * K_pad: a multiple of 64, >= K.  2 <= L_max <= DSIM_TRAJGEN_LMAX (n_seg <= 8).  Entries of segments past a course's own
 * n_seg hold NaN.  Bytes: 240 (L_max - 1) + 8 L_max + 4 per course, 2 236 at L_max = 9.                                 */
#define DSIM_TRAJGEN_LMAX 9
typedef struct dsim_traj_bank {
  int64_t  K, K_pad;
  int32_t  L_max;
  int32_t  _pad;
  double*  coeffs;
  double*  ts;
  int32_t* n_seg;
} dsim_traj_bank;

/* trajGenerator.__init__ (dronesim/utils/trajGen.py:13-106, trajutils.py:13-36) for K courses in one launch: one lane per
 * course.  Course k: n_wp[k] waypoints wp[(l * 3 + d) * K_pad + k] (2 <= n_wp[k] <= L_max), one max_vel and gamma for all.
 *   Tmin_i = |wp[i+1] - wp[i]| / max_vel (trajGen.py:33-34); segment times T by mode:
 *     DSIM_TRAJGEN_GIVEN     bank->ts holds the cumulative times on entry and is left as it is;
 *     DSIM_TRAJGEN_TMIN      T = Tmin;
 *     DSIM_TRAJGEN_OPTIMIZE  minimises J(T) = trace(P^T Q P) + gamma sum(T) subject to T >= Tmin (trajGen.py:27-40).
 *   coeffs = MinimizeSnap(T) (trajGen.py:45-106): order 10, positions at both ends of every segment, derivatives 1-4
 *   continuous, at rest at both ends, the 4 (L - 2) interior derivatives free and chosen to minimise the cost; L = 2 has none.
 * The reference inverts the dense 10 n_seg-square constraint matrix.  Here a segment's cost is the quadratic form of its
 * scaled end values in ONE constant 10 x 10 matrix M over T^7, held as its 6 x 10 factor F (M = F^T F; tables, exact
 * rationals rounded once), and the interior derivatives solve a least-squares problem with a block-bidiagonal matrix of
 * 6 x 4 blocks: one sweep along the course in registers, by Householder reflections, gives J (that is an evaluation of the
 * search: about a thousand flops per segment), a second sweep back gives the coefficients.  Each segment is solved for
 * p(t) - wp[seg], which costs the same.  No difference of nearly equal numbers is formed, so a short leg beside a long one
 * keeps its digits up to a ratio of about 1 000 in their times; beyond that the course is refused, see below.
 * The reference searches T with scipy's COBYLA; this search is a greedy multiplicative pattern search, deterministic and
 * derivative-free: from x = Tmin and step = 0.5, sweep i and try y_i = max(Tmin_i, x_i (1 + step)), then
 * max(Tmin_i, x_i / (1 + step)) (a y_i equal to x_i is skipped); J(y) < J(x) is accepted at once and the sweep moves to
 * i + 1; a sweep that accepted nothing halves step; it ends at step <= 1e-4 or after max_evals evaluations of J (>= 1; the
 * first is J(Tmin), so max_evals = 1 returns Tmin).  It reaches the reference's J to parts in 1e9 on the fixture courses
 * (tests/README_trajgen.md); T itself agrees to about 1e-3, the minimum is flat.
 * Out: bank->coeffs, ->ts (not in GIVEN), ->n_seg; cost[k] = trace(P^T Q P) without the gamma term (trajGenerator.cost);
 * evals[k] = evaluations of J the search spent (0 in GIVEN / TMIN); status[k] = 0, or DSIM_TRAJGEN_BAD_* for a course that
 * cannot be made — n_wp[k] out of [2, L_max], a non-finite waypoint, a zero-length segment (the reference's matrix is singular
 * there), in GIVEN a time step that is not positive and finite, or (DSIM_TRAJGEN_BAD_CONDITION) segment times at which
 * the solve cannot keep the published accuracy (tests/README_trajgen.md) — whose coeffs, ts, seg_times and cost are NaN
 * and n_seg 0.  DSIM_TRAJGEN_BAD_CONDITION is reported where a pivot of the carried triangular factor is more than
 * 2^14 times smaller than its column was and a later segment goes on from it (a leg whose time is about 1 000 times
 * shorter than those around it; measured error of the course 0.2 eps (ratio)^2), where T^9 or T^-9 of a segment is no
 * normal fp64 number (T outside about 1e-33 .. 1e33 s), and where a coefficient or the cost comes out not finite; it is
 * judged at the times the course is made for, and evals[k] still counts what the search spent.  The other courses of the
 * launch are not affected.  cost, evals, status: [K_pad].  seg_times (nullable) receives the segment times
 * the coefficients were made for, NaN past n_seg and for such a course: T >= Tmin holds for them exactly.
 * workspace: dsim_trajgen_workspace(K_pad, L_max) fp64 entries (38 (L_max - 2) K_pad: what the sweep back needs of the
 * sweep along), the call's until it has run; may be NULL at L_max = 2.  Stream-ordered, allocates and synchronises nothing.
 * DSIM_E_ARG, nothing enqueued: a null pointer, K < 1, K_pad < K or no multiple of 64, L_max outside [2, DSIM_TRAJGEN_LMAX],
 * max_vel / gamma not finite or max_vel <= 0, gamma <= 0 in DSIM_TRAJGEN_OPTIMIZE (J has no minimum then; GIVEN and TMIN
 * do not read gamma), an unknown mode, max_evals < 1, a workspace too small.                                            */
enum { DSIM_TRAJGEN_GIVEN = 0, DSIM_TRAJGEN_TMIN = 1, DSIM_TRAJGEN_OPTIMIZE = 2 };
enum { DSIM_TRAJGEN_BAD_COUNT = 1, DSIM_TRAJGEN_BAD_WAYPOINT = 2, DSIM_TRAJGEN_BAD_SEGMENT = 3, DSIM_TRAJGEN_BAD_TIME = 4,
       DSIM_TRAJGEN_BAD_CONDITION = 5 };
typedef struct dsim_trajgen_args {
  const double*  wp;
  const int32_t* n_wp;
  double   max_vel, gamma;
  int32_t  mode;
  int32_t  max_evals;       /* the search's cap on evaluations of J (2000 is ample: the fixture courses take 14 .. 539) */
  double*  cost;
  int32_t* evals;
  int32_t* status;
  double*  seg_times;       /* nullable [L_max - 1][K_pad]: T itself, seg_times[seg * K_pad + k] (differences of ts lose its last bits) */
  double*  workspace;
  int64_t  workspace_len;
} dsim_trajgen_args;
int64_t dsim_trajgen_workspace(int64_t K_pad, int32_t L_max);
int dsim_trajgen(dsim_ctx* ctx, void* stream, const dsim_traj_bank* bank, const dsim_trajgen_args* args);

/* dsim_traj_sample with a course per drone: drone i samples course traj_id[i] of the bank (traj_id: device int32 [n_pad];
 * NULL = the identity, which needs bank->K >= n).  Everything else — t, dt_advance, yaw_state, offset, the clamp past the
 * end, the segment search, fp64 polynomials, the stateful yaw rule and its NaN at zero horizontal velocity — is
 * dsim_traj_sample's, statement by statement: with one course the two calls write the same bits.
 * A drone whose traj_id is outside [0, K), or whose course has n_seg outside [1, L_max - 1], gets NaN in all ten target
 * fields and in its yaw_state; a course with NaN ts gives NaN targets through the arithmetic.  Nothing is read out of bounds.
 * Bytes: a drone reads the 30 fp64 coefficients of its segment per sample, 240 B, besides its 8 B of t, 24 B of
 * yaw_state and up to 8 L_max of ts — more than the 168 B per drone of the fused step itself.  With K = n that comes from HBM,
 * uncoalesced only in that neighbouring drones may sit in different segments; with courses shared among drones it is served
 * from L2. */
int dsim_traj_sample_bank(dsim_ctx* ctx, void* stream, int64_t n, const dsim_traj_bank* bank, const int32_t* traj_id,
                          double* t, double dt_advance, double* yaw_state, const float* offset, dsim_view targets_out);

/* The same rows as dsim_observe, written field-major: SoA [obs_width][n_pad] (coalesced), the slab a
 * device-side Logger appends per step (dronesim/utils/Logger.py:117-139 stores exactly this vector). */
int dsim_observe_soa(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const float* last_action,
                     float* obs_out, int32_t obs_width);

/* Neighbour downwash, formula P8 (BaseAviary._downwash, BaseAviary.py:1736-1763; dead code in the
 * fork, intended semantics): for every local drone i and every drone j of the WORLD above it
 * (dz > 0) within dxy < 10 m,  Fz -= DW1 (PROP_RADIUS/(4 dz))^2 exp(-0.5 (dxy / (DW2 dz + DW3))^2)
 * with the receiving drone's coefficients, along its body z axis.
 * pos_all: SoA [3][m_pad] positions of ALL drones of the world (on several GPUs: the all-gather of
 * every rank's positions); the library bins them into a uniform xy grid (cell >= 10 m; drones outside
 * the box are clamped to the border cells, which keeps every pair within 10 m in adjacent cells) and
 * each local drone scans its 3x3 cells: O(n * neighbours) instead of the reference's O(n m).  Receivers
 * are processed in grid order (a wave's lanes sit in the same or neighbouring cells, so their scans
 * read the same sorted entries).
 * force_out: SoA [3][n_pad], x and y written as 0 (feed it to dsim_step_args.ext_force).
 * workspace: caller-owned device int32 buffer of at least dsim_downwash_workspace(m, nx, ny) entries. */
struct dsim_halo_plan;
typedef struct dsim_downwash_args {
  const float* pos_all;     /* SoA [3][m_pad] positions of every drone of the world, or NULL: the world is this
                               fleet alone (m = n, local_offset = 0) and positions are read from the state block */
  int64_t  m, m_pad;
  float    xmin, ymin, cell;
  int32_t  nx, ny;
  int32_t* workspace;
  int64_t  workspace_len;
  const uint8_t* type_id;   /* nullable; types of the LOCAL drones */
  int64_t  local_offset;    /* index inside pos_all of local drone 0 (the rank's shard begin); the local
                               drones' entries of pos_all must equal their state positions               */
  int32_t  prebinned;       /* 1: the previous dsim_step was given this grid as bin_next and has already binned the
                               local drones (see dsim_step_args.bin_next); only the other entries of pos_all are
                               binned by this call.  The library falls back to a full binning pass when its own
                               record of the last prebinning does not match (another grid, or the positions were
                               moved since by a call that did not re-bin them).                              */
  int32_t  phase;           /* DSIM_DW_*: with a halo plan the call can be split so that the exchange overlaps the local
                               part of the query (see dsim_halo_plan)                                        */
  const struct dsim_halo_plan* halo;   /* nullable: the rest of the world is what the neighbouring ranks sent (pos_all must
                               be NULL, local_offset 0, m = n + the sum of the plan's recv_cap); bucket form only */
  uint64_t* pairs_evaluated; /* nullable device counter, diagnostics only (results do not depend on it): += the number of
                               (receiver, candidate) pairs whose term the query's loops evaluate in this call — the unit of
                               the query's vector-pipe roofline (bench.py, config 5).  Bucket form only; one atomic per
                               receiver group when given, one scalar test when not                                        */
  /* -- kept candidate lists (no counterpart in the reference, whose loop is O(N^2) per drone) ---------------------------------
   * A fleet moves centimetres per Env.step, so WHICH candidates the receivers of a cell have to look at changes slowly.
   * DSIM_DW_KEEP_BUILD: the query also writes, per cell, the list it worked out (receivers in height order, candidates in
   * height-band order), with its reach and band tests widened by 2 keep_skin.  DSIM_DW_KEEP_REUSE: the query reads the lists of
   * the last BUILD call on this grid and the CURRENT positions and goes straight to the pair loops; nothing is binned — a
   * dsim_step that is given this block as bin_next refreshes every drone's position in the grid's buckets IN PLACE instead (no
   * atomic round trip for a bucket slot); a call that finds no such step in front of it refreshes them itself.  EXACT for any motion: every pair is still tested against the cut-off and the height order on current positions;
   * a drone that has moved further than keep_skin from where it was at the BUILD leaves the lists for the overflow list, which
   * every receiver scans, and is served where it is now.  How often to BUILD is the caller's choice (performance only: the
   * more drones have left the skin, the longer the overflow scan).  Honoured where dsim_downwash_keep_ok() != 0 (the world is
   * this fleet alone: pos_all = NULL, no halo plan; bucket form at a density that takes the banded query; cells of
   * 5 m + keep_skin or more — two rings of cells cover the widened reach — and below 10 m), otherwise ignored; a REUSE without usable
   * lists (none made yet, another grid or fleet size) is answered as a BUILD.  keep_ws: caller-owned,
   * dsim_downwash_keep_workspace(n_pad, nx, ny) int32 entries, owned by the library between a BUILD and the last REUSE. */
  int32_t  keep;            /* DSIM_DW_KEEP_* */
  int32_t  keep_age;        /* REUSE: how many REUSE calls the lists have served, this one included (1, 2, ...; the dsim_step that is
                               given this block as bin_next refreshes for that call).  The skin moves with the fleet — displacements are
                               measured against the mean drift of a sample of it, predicted from the two refreshes before —, and the
                               age says which of the ring of sums a refresh fills.  Performance only: a wrong age makes the prediction
                               worse, never the result (the query reads the drift its refresh used from device memory).             */
  float    keep_skin;       /* metres, > 0 */
  int32_t* keep_ws;
  int64_t  keep_ws_len;
} dsim_downwash_args;
enum { DSIM_DW_KEEP_OFF = 0, DSIM_DW_KEEP_BUILD = 1, DSIM_DW_KEEP_REUSE = 2 };
int64_t dsim_downwash_keep_workspace(int64_t n_pad, int32_t nx, int32_t ny);
/* How the lists are holding up, WITHOUT synchronising anything: *queries = the REUSE calls enqueued so far; *outside_skin = the
 * length of the overflow list that REUSE call number *of_query (1-based; 0: none has finished) found — the drones that had left the
 * skin, which every later call until the next BUILD will find too, and more; *half_way = the drones the refresh in front of that
 * call found further than HALF the skin from where they were when the lists were made (the warning: a fleet in coordinated motion
 * leaves any skin together, and a REUSE call whose overflow list holds the fleet costs a hundred plain ones).  The device writes
 * the three into host memory when that query starts; a caller that paces its BUILDs by them (dronesim_amd/downwash.py) reads values
 * a query or two old, which is what such pacing needs.  -1: no feedback memory. */
int     dsim_downwash_keep_stats(dsim_ctx* ctx, int64_t* outside_skin, int64_t* half_way, int64_t* of_query, int64_t* queries);
int     dsim_downwash_keep_ok(int64_t m, int32_t nx, int32_t ny, float cell, float keep_skin);
int64_t dsim_downwash_workspace(int64_t m, int32_t nx, int32_t ny);

/* ---- halo exchange of a spatially sharded fleet (BASELINE config 5: slabs along x, one rank per GPU) -----------------
 * The reference's downwash loop runs over the whole world (BaseAviary.py:1736-1763); a sharded fleet needs, per rank,
 * the positions of the other ranks' drones that can be within the 10 m cut-off of one of its own.  The library does the
 * device side of that exchange — selecting and packing the boundary drones, binning what arrived — and the caller moves
 * the packed buffers between ranks (RCCL send/recv; the library itself has no communicator).  Per Env.step, with no
 * host synchronisation anywhere:
 *     dsim_halo_pack -> [send/recv of the caller, on the collective library's stream] ............ wait for it
 *                    -> dsim_downwash(DSIM_DW_LOCAL) (beside the wire) -> dsim_downwash(DSIM_DW_HALO_BIN)
 *                    -> dsim_downwash(DSIM_DW_HALO_QUERY) -> dsim_step(bin_next)
 * or, with a transport that has no latency to hide, pack -> wire -> dsim_downwash(DSIM_DW_ALL) -> dsim_step.
 * A message is a HEADER (DSIM_HALO_HDR floats: the number of positions that follow, and the sender's xy bounding box at
 * the time of sending) followed by xyz triples.  dsim_halo_pack selects, for every peer, the local drones inside that
 * peer's box — read from the header of the LAST message that peer sent, in device memory — grown by reach[p]; with a
 * message every step the box is one Env.step old, so reach = cut-off + (max coordinate velocity) x dt_env is exact for ANY
 * motion the integrator allows (Bullet clamps every coordinate velocity to 100 m/s, P4).  Message sizes are fixed on
 * the host (send_cap / recv_cap, re-made rarely from counts read back); the count travels in the header, and a
 * selection that does not fit is dropped AND counted (DSIM_Q_HALO_OVERFLOW: 0 certifies that nothing was missed).      */
#define DSIM_MAX_PEERS 8
#define DSIM_HALO_HDR 8      /* floats: [0] count (int32 bits)  [1..4] xmin ymin xmax ymax of the sender  [5] max |coordinate
                                velocity| of the sender (diagnostic)  [6..7] reserved                                    */
enum {
  DSIM_DW_ALL = 0,          /* one grid, one query: local drones and whatever pos_all / the halo plan hold               */
  DSIM_DW_LOCAL = 1,        /* bin (unless pre-binned) and query the LOCAL drones only; force_out is written              */
  DSIM_DW_HALO_BIN = 2,     /* bin the plan's received positions into the halo grid (touches nothing else)                 */
  DSIM_DW_HALO_QUERY = 3    /* local receivers against the halo grid; force_out += (after LOCAL and HALO_BIN)             */
};
typedef struct dsim_halo_plan {
  int32_t world, rank;
  int64_t cap;              /* positions a peer's buffer can hold; buffer p begins at float (DSIM_HALO_HDR + 3 cap) p      */
  float*  send;             /* device [world][DSIM_HALO_HDR + 3 cap]: dsim_halo_pack writes header + triples for peer p    */
  const float* recv;        /* device, same shape: the last message of peer p (its header is read by the NEXT pack)       */
  int32_t* scratch;         /* device int32[32], zero-initialised by the caller once, owned by the plan's pack calls       */
  int32_t send_cap[DSIM_MAX_PEERS];   /* host: positions in the message to peer p (0: no message to p)                    */
  int32_t recv_cap[DSIM_MAX_PEERS];   /* host: positions in the message from peer p                                       */
  float   reach[DSIM_MAX_PEERS];      /* host: selection margin around peer p's last known box, >= the cut-off             */
} dsim_halo_plan;
/* out5 (device float[5]): xmin, ymin, xmax, ymax of the n local drones and their largest |coordinate velocity|. */
int dsim_fleet_bounds(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, float* out5);
/* One launch: for every peer p != rank, send[p] = header + the positions of the local drones inside p's last known box
 * grown by reach[p] (at most send_cap[p] of them; the header carries the number SELECTED, so the receiver sees an
 * overflow too), and this rank's own box in every header. */
int dsim_halo_pack(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_halo_plan* plan);
/* workspace (int32 entries) of a split-phase downwash: the local grid of n drones + the halo grid of up to h drones */
int64_t dsim_downwash_workspace_halo(int64_t n, int64_t h, int32_t nx, int32_t ny);

/* The deferred WLS fallback pass of a table with a morphing hexa (wls_alloc.py:222-350 for the drones whose first
 * iteration left the box), as its own call: what dsim_step / dsim_control2 launch behind themselves unless
 * DSIM_OPT_DEFER_FALLBACK is set.  cmd_out nullable (SoA [n_act][n_pad], as dsim_control2). */
int dsim_wls_fallback(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const uint8_t* type_id, float* cmd_out);
/* != 0 when a grid of this shape takes the bucket form (one binning pass, cell-centred LDS-tiled query), which is
 * the form dsim_step_args.bin_next can fill. */
int dsim_downwash_prebin_ok(int64_t m, int32_t nx, int32_t ny);
int dsim_downwash(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_downwash_args* args,
                  float* force_out);
/* Forgets the ctx's bookkeeping of the neighbour grid (which of the two count buffers is current, whether a step has
 * filled one ahead): the next dsim_downwash clears both and bins everything itself.  Host-side only, nothing is launched.
 * For callers that replay a captured sequence of dsim_downwash / dsim_step calls (hipGraph): captured behind this call, the
 * sequence starts from no assumption about the buffers, and called again after a replay, so does whatever follows. */
int dsim_downwash_reset(dsim_ctx* ctx);

/* Neighbourhood adjacency at fleet scale (BaseAviary._getAdjacencyMatrix, BaseAviary.py:901-921: drones
 * i != j are neighbours when |pos_i - pos_j| < neighbourhood_radius).  The reference returns the dense
 * O(N^2) matrix row in every observation; here the same uniform grid as the downwash gives, per local
 * drone, the neighbour count and (optionally) up to max_k neighbour indices into pos_all in ascending
 * grid order: the cell index cy * nx + cx of the listed neighbours never decreases along a list, and a
 * list cut at max_k holds the neighbours of the lowest cells; the order inside one cell is unspecified
 * (count_out [n_pad], exact whatever max_k; list_out [max_k][n_pad] nullable, unused slots -1).
 * args->cell must be >= radius (DSIM_E_ARG otherwise, nothing is written); pos_all / workspace /
 * local_offset as for dsim_downwash (type_id is ignored). */
int dsim_adjacency(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_downwash_args* args,
                   float radius, int32_t* count_out, int32_t* list_out, int32_t max_k);

/* Drone-drone contact watch: per-drone clearance between the bounding spheres of the vehicles (dsim_type_params.collision_sphere)
 * on the same uniform grid.  No counterpart in the reference, whose Bullet world lets the vehicles' collision shapes act on each
 * other; this library models no such contact and reports where it would have mattered.  For local drone i, over every other
 * drone j of the world,
 *     c_ij = |p_i - p_j| - R_i - R_j   (3-D),      clearance_out[i] = min(margin, min_j c_ij)       [n_pad]
 *     nearest_out[i] = the j that attains the minimum, as an index into the world (pos_all), -1 when no c_ij < margin
 *                      (nullable; [n_pad])
 * A drone with R = 0 neither receives nor is seen: clearance = margin, nearest = -1.  Every unordered pair with c_ij < 0 is
 * counted once per world, by the rank that owns the lower world index (i local, j > i + local_offset): into the cumulative
 * counter DSIM_Q_DRONE_CONTACTS and, when pairs_out is given, *pairs_out += the count (a device counter).  One-sided like the
 * ground watch: a count of 0 certifies that Bullet's narrow phase would have found no drone-drone contact; a pair that is
 * counted has overlapping SPHERES, which the shapes inside them need not.
 * R of a local drone comes from the type table (args->type_id with more than one type).  With args->pos_all the radius of every
 * world entry — the remote drones' too — is radius_all [m_pad] (device; the local entries must agree with the table), and
 * without pos_all radius_all must be NULL.  args->cell must be >= 2 R_max + margin (R_max over the type table, and the caller
 * vouches for it over radius_all): every pair with c_ij < margin is then less than one cell apart in x and in y, so its two
 * drones lie in the same or adjacent cells — also when one of them is clamped into a border cell from outside the box, because
 * clamping never moves two cell indices further apart.  The grid takes the counting-sort form; workspace: at least
 * dsim_clearance_workspace(m, nx, ny) int32 entries.  A halo plan: DSIM_E_UNSUPPORTED.  margin > 0. */
int64_t dsim_clearance_workspace(int64_t m, int32_t nx, int32_t ny);
int dsim_clearance(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_downwash_args* grid,
                   const float* radius_all, float margin,
                   float* clearance_out, int32_t* nearest_out, uint64_t* pairs_out);

/* Nearest-neighbour observation: per local drone the k closest drones within `radius`, sorted, with their relative state.  The
 * reference puts the dense N x N row of _getAdjacencyMatrix into every observation; dsim_adjacency's list is cut in grid order and
 * carries no distance.  This is what a decentralised controller asks: who is nearest, where, and how it moves relative to me.
 * For local drone i the neighbours are the world entries j != i with d_ij = |p_j - p_i| < radius (3-D, strict, as the adjacency):
 *     count_out[i]        = their number, exact whatever k (as dsim_adjacency's)
 *     slots t = 0 .. min(k, count) - 1: the neighbours of least distance, ascending by the key (d^2, j) — d^2 as fp32 computes it
 *                           from the fp32 differences, an exact tie going to the lower world index —
 *     index_out[t][i]     = j, an index into the world (pos_all, or this fleet);     -1 in unused slots
 *     dist_out[t][i]      = d_ij [m];                                               +inf in unused slots
 *     rel_pos_out[t][:][i] = p_j - p_i;                                              0 in unused slots
 *     rel_vel_out[t][:][i] = v_j - v_i (DSIM_F_VEL, world frame);                    0 in unused slots
 * Deterministic from run to run.  A local drone whose position is not finite gets count 0 and empty slots; a candidate whose
 * position is not finite is nobody's neighbour (the comparison fails).  Entries i >= n are not written.  Stream-ordered, allocates
 * nothing, never synchronises; all outputs are written with plain vector stores.
 * The drones are binned per call on the counting-sort grid of `grid`, as dsim_adjacency bins them (pos_all / local_offset /
 * workspace as there; type_id is ignored).  grid->cell must be >= radius: every pair closer than the radius is then less than one
 * cell apart in x and in y, so its drones lie in the same or adjacent cells — also when one of them is clamped into a border cell
 * from outside the box, because clamping never moves two cell indices further apart.  Workspace: at least
 * dsim_knn_workspace(m, nx, ny) int32 entries.  The relative velocity is gathered from the state block by world index, so it needs
 * the world to be this fleet: rel_vel_out must be NULL with grid->pos_all.
 * DSIM_E_ARG, nothing enqueued: a null ctx, args, grid or index_out; k outside 1 .. 16; a radius that is not finite or not > 0; an
 * unknown flag; grid->cell < radius; a workspace that is too short; rel_vel_out together with grid->pos_all; and what dsim_adjacency
 * refuses of the grid and of n.  A halo plan: DSIM_E_UNSUPPORTED. */
typedef struct dsim_knn_args {
  const dsim_downwash_args* grid;  /* xy grid, counting-sort form, as for dsim_adjacency; cell >= radius; a halo plan: DSIM_E_UNSUPPORTED */
  float radius;                    /* > 0, finite: only drones with |p_j - p_i| < radius are neighbours */
  int32_t k;                       /* 1 .. 16 */
  int32_t flags;                   /* 0 (unknown bits: DSIM_E_ARG) */
  int32_t* index_out;              /* [k][n_pad] world index, -1 in unused slots; required */
  float*   dist_out;               /* [k][n_pad] metres, +inf in unused slots; nullable */
  float*   rel_pos_out;            /* [k][3][n_pad] p_j - p_i, 0 in unused slots; nullable */
  float*   rel_vel_out;            /* [k][3][n_pad] v_j - v_i, 0 in unused slots; nullable; must be NULL with grid->pos_all */
  int32_t* count_out;              /* [n_pad] number of drones within radius; nullable */
} dsim_knn_args;
int64_t dsim_knn_workspace(int64_t m, int32_t nx, int32_t ny);
int dsim_knn(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_knn_args* args);

/* Static-obstacle watch: per-drone clearance to world triangle meshes.  The third thing a Bullet world does to a vehicle besides
 * the ground plane and the other vehicles is collide it with the static bodies loaded into the world (p.loadURDF of a gate, a
 * wall; a body marked concave="yes" collides against its triangles).  This library models no such contact and reports where it
 * would have mattered, in the drone watch's terms:
 *   - The watch is one-sided.  A count of 0 certifies that, at the sampled states, no vehicle's bounding sphere
 *     (dsim_type_params.collision_sphere) touched a triangle, and hence that Bullet's narrow phase had nothing to report at
 *     those states.
 *   - A counted drone has an overlapping SPHERE, which its shapes need not.
 *   - The watch samples the end of an Env.step, as the other two watches do.
 *   - A meshed solid is its surface.  A sphere wholly inside a closed body is not seen, but it crossed the surface on the way in.
 *
 * An obstacle set is a soup of triangles in fp32 (tri [n_tri][9]: vertices a, b, c), each carrying the index of the BODY it belongs
 * to; it is static for its lifetime.  Around it lies a uniform 3-D grid over the soup's bounding box grown by `reach`; the list of
 * a cell holds every triangle whose distance to any point of that cell can be below `reach` (and may hold more: over-inclusion is
 * allowed, omission is not).  The cell of a point q is (clamp(floor((q - origin) / cell), 0, n - 1)) per axis, index
 * (cz * ny + cy) * nx + cx; the lists carry a slack of a hundredth of a cell, so a point within fp32 rounding of a cell face may be
 * looked up in either cell.  A point outside the grown box [lo, hi] has no triangle within `reach`.
 *
 * The two grid functions are host-only: no ctx, no device, callable on a machine without a GPU.
 *   dsim_obstacle_grid_plan   chooses the grid (the cell edge starts at reach / 2 and is doubled until there are at most 2^18 cells,
 *                             4096 along an axis, and 2^26 list entries) and counts the lists: *out is complete, list_len included.
 *   dsim_obstacle_grid_build  fills cell_start [cells + 1] (cells = nx ny nz; cell_start[cells] = list_len) and cell_tri [list_len]
 *                             (triangle indices, ascending inside a cell) for the grid `g` the plan returned for the same soup.
 * DSIM_E_ARG, with nothing written: n_tri < 1 or > 65536, a null pointer, reach <= 0 or not finite, a non-finite coordinate, a
 * triangle with area below 1e-12 m^2, a grid that needs more than 2^18 cells at any list budget, or (build) a `g` that is not the
 * plan of this soup. */
typedef struct dsim_obstacle_grid {
  float   origin[3];      /* corner of cell (0, 0, 0) = lo                                                      */
  float   cell;           /* cell edge [m]                                                                      */
  int32_t nx, ny, nz;
  float   reach;          /* what the lists were made for                                                       */
  int64_t list_len;       /* entries of cell_tri                                                                */
  float   lo[3], hi[3];   /* the soup's bounding box grown by reach                                             */
} dsim_obstacle_grid;
int dsim_obstacle_grid_plan(const float* tri, int64_t n_tri, float reach, dsim_obstacle_grid* out);
int dsim_obstacle_grid_build(const float* tri, int64_t n_tri, const dsim_obstacle_grid* g, int32_t* cell_start, int32_t* cell_tri);

/* The device set, owned by the library: dsim_obstacles_create plans and builds the grid on the host, prepares one 64-byte record
 * per triangle (a, ab, ac, the unit normal, the three dot products of the region test, the body index), allocates, uploads and
 * SYNCHRONISES.  It must not sit inside a stream capture (like the run table of DSIM_OPT_CALLER_IO, it is made before capture
 * starts); neither must dsim_obstacles_destroy, which waits for the work that may still read the set.  tri_host [n_tri][9] and
 * body_host [n_tri] (>= 0; NULL: every triangle is body 0) are host memory, read during the call only.  Errors as the grid plan's. */
typedef struct dsim_obstacles dsim_obstacles;
int dsim_obstacles_create(dsim_ctx* ctx, const float* tri_host, const int32_t* body_host, int64_t n_tri, float reach,
                          dsim_obstacles** out);
int dsim_obstacles_destroy(dsim_ctx* ctx, dsim_obstacles* set);

/* The query: stream-ordered, allocates nothing, never synchronises (it may be captured).  For drone i of `state`,
 *     q_i = p_i - offset_i       offset: SoA [3][n_pad] (device) or NULL = 0.  The set lives in the frame of the drone's TASK, which
 *                                is what dsim_step_args.wp_offset means for waypoint tables: every replica has its own gate.
 *     R_i = collision_sphere of its type (type_id [n_pad], required with more than one type)
 *     c_i = min_t dist(q_i, triangle t) - R_i       exact Euclidean point-triangle distance (face, edge and vertex regions)
 *     clearance_out[i] = min(margin, c_i)                                                                  [n_pad]
 *     nearest_out[i]   = the BODY index of the triangle that attains the minimum, -1 when c_i >= margin      [n_pad], nullable
 *                        (not the triangle: a closest point on a shared edge belongs to two triangles)
 * A type with R = 0 takes no part: its drones get clearance = margin, nearest = -1 and are never counted.  Every drone with
 * c_i < 0 adds one to the cumulative counter DSIM_Q_OBSTACLE_CONTACTS and, when contacts_out is given, to *contacts_out (a device
 * counter); one atomic per wave and counter at most.  DSIM_E_ARG, nothing written: a null ctx / set / clearance_out, margin <= 0,
 * or R_max + margin > reach of the set (R_max over the type table), because a cell list then no longer holds every triangle
 * that matters.  A wave none of whose drones lies in the grown box reads its positions and nothing else. */
int dsim_obstacle_clearance(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_obstacles* set,
                            const float* offset, const uint8_t* type_id, float margin,
                            float* clearance_out, int32_t* nearest_out, uint64_t* contacts_out);

/* The swept query: the clearance along the CHORD from the position the previous call saw to the current one, as a swept sphere.
 * dsim_obstacle_clearance certifies the sampled states only; between two samples a vehicle a few m/s fast crosses a bar 0.14 m
 * thick unseen.  Stream-ordered, allocates nothing, never synchronises (it may be captured).  For drone i of `state`,
 *     q1 = p_i - offset_i, q0 = prev_i - offset_i        prev: SoA [3][n_pad] (device), WORLD frame like p, owned by the caller
 *     Rs = collision_sphere of its type + sag            sag >= 0 [m]: how far the flown path may leave its chord; a path whose
 *                                                        acceleration is bounded by a_max leaves it by at most a_max T^2 / 8 over T
 *     c_i = min_t dist(segment q0 q1, triangle t) - Rs   exact segment-triangle distance, 0 where the chord pierces a triangle
 *     clearance_out[i] = min(margin, c_i);  nearest_out[i] = the BODY that attains the minimum, -1 when c_i >= margin
 * Every drone with c_i < 0 adds one to DSIM_Q_OBSTACLE_CONTACTS and to *contacts_out, as in the point query: the same quantity,
 * measured better.  A type with collision_sphere = 0 takes no part (margin, -1, never counted), whatever the sag.  Then, unless
 * DSIM_SWEEP_KEEP_PREV is set, prev_i := p_i for every drone i < n (also those of R = 0 and those outside the box): a captured
 * and replayed call carries its own history.
 *
 * A chord is cut into K = ceil(|q1 - q0| / (2 half)) equal pieces, half = reach - (R_max + sag + margin), each looked up in the
 * cell of its own midpoint: a triangle within Rs + margin of a piece is within reach of that midpoint, so the minimum over the
 * pieces is the chord's and does not depend on K (half is taken 2^-10 shorter when K is chosen).  A piece whose midpoint lies
 * outside the grown box reads no list.  A drone is UNSWEPT when K > 32 (a teleport: the caller's own reset) or when prev_i or p_i
 * has a non-finite component: it is a point sample at q1, bit for bit what dsim_obstacle_clearance gives for the radius Rs, and
 * adds one to *unswept_out (types with R = 0 are not counted).  A non-finite p_i gives (margin, -1) and leaves itself in prev.
 *
 * DSIM_SWEEP_PRIME: prev_i := p_i for i < n and nothing else; offset, type_id, margin, sag, the outputs and the counters are not
 * looked at.  DSIM_E_ARG, nothing written: a null ctx / set / args / prev, n <= 0 or > n_pad, an unknown flag or both flags; and
 * unless PRIME: more than one type without type_id, a null clearance_out, margin <= 0, sag < 0, either not finite, or half < reach / 1024
 * (make the set with reach >= R_max + sag + margin + half the chord length one lookup should serve). */
enum { DSIM_SWEEP_KEEP_PREV = 1,   /* do not write prev (on-demand queries, the eager call before a capture) */
       DSIM_SWEEP_PRIME     = 2 }; /* prev := current position and nothing else: no outputs, no counters    */
typedef struct dsim_sweep_args {
  const float*   offset;        /* SoA [3][n_pad] or NULL, as dsim_obstacle_clearance                      */
  const uint8_t* type_id;       /* [n_pad]; required with more than one type                               */
  float          margin;        /* > 0                                                                      */
  float          sag;           /* >= 0 [m]: added to every radius                                          */
  float*         prev;          /* SoA [3][n_pad], WORLD frame, in-out; required                            */
  int32_t        flags;
  float*         clearance_out; /* [n_pad]; required unless PRIME                                           */
  int32_t*       nearest_out;   /* [n_pad], nullable                                                        */
  uint64_t*      contacts_out;  /* device counter, nullable                                                 */
  uint64_t*      unswept_out;   /* device counter, nullable                                                 */
} dsim_sweep_args;
int dsim_obstacle_sweep(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_obstacles* set,
                        const dsim_sweep_args* args);

/* The swept drone-drone query: dsim_clearance along the CHORDS from the positions the previous call saw to the current ones.
 * dsim_clearance certifies the sampled states only; two vehicles that close at a few m/s, or any fleet sampled once per several
 * Env.steps, pass through each other between two samples.  Stream-ordered, allocates nothing, never synchronises.  Each drone is
 * a sphere of radius R + sag that moves linearly from p0 = prev to p1 = its current position, both drones of a pair at the same
 * parameter s in [0, 1]:
 *     d0 = p0_j - p0_i,  d1 = p1_j - p1_i,  Delta = d1 - d0
 *     s* = clamp(-d0.Delta / Delta.Delta, 0, 1)            (0 where Delta.Delta = 0)
 *     dist^2 = min(|d0|^2, |d1|^2, |d0 + s* Delta|^2)       never above the point query's distance at either end
 *     c_ij = sqrt(dist^2) - (R_i + sag) - (R_j + sag)
 *     clearance_out[i] = min(margin, min_j c_ij);  nearest_out[i] = the j that attains it, -1 when no c_ij < margin
 * sag >= 0 [m]: how far a flown path may leave the interpolation AT EQUAL TIMES; with |a| <= a_max over the time T between two
 * calls that is a_max T^2 / 8 per drone, hence 2 sag per pair.  A type with collision_sphere = 0 takes no part (margin, -1, never
 * counted), whatever the sag.  Every unordered pair with c_ij < 0 is counted once per call, by the lower index, into
 * DSIM_Q_DRONE_CONTACTS and *pairs_out, as in dsim_clearance: the same quantity, measured better.  Then, unless
 * DSIM_SWEEP_KEEP_PREV is set, prev_i := p_i for every i < n.
 *
 * The drones are binned at their CURRENT positions on the counting-sort grid of `grid`, as dsim_clearance bins them.  grid->cell
 * must be >= 2 (R_max + sag) + margin + 2 travel: a pair with c_ij < margin has |d1| <= |d(s*)| + |Delta| < 2 (R_max + sag) +
 * margin + 2 travel as long as no chord is longer than `travel`, so its current positions lie in the same or adjacent cells
 * (clamping into a border cell is monotone).  The library enforces the bound: a drone whose chord is longer than travel (by a
 * comparison 2^-20 on the safe side), or whose prev_i or p_i has a non-finite component, is UNSWEPT — p0 := p1, a point sample —
 * and adds one to *unswept_out when its R > 0.  Workspace: at least dsim_clearance_sweep_workspace(m, nx, ny) int32 entries (the
 * clearance layout and one 16-byte aligned float4 [m]).
 *
 * DSIM_SWEEP_PRIME: prev_i := p_i for i < n and nothing else; grid (may be NULL), margin, sag, travel, the outputs and the
 * counters are not looked at.  Refused with nothing enqueued: a NULL args or prev, an unknown flag or both flags (DSIM_E_ARG);
 * grid->pos_all or a halo plan (DSIM_E_UNSUPPORTED: a sharded world would need prev for every world entry); and DSIM_E_ARG for a
 * NULL ctx, n <= 0 or > n_pad, and unless PRIME: a NULL grid or clearance_out, margin <= 0, sag < 0, travel <= 0, any of them not
 * finite, more than one type without grid->type_id, the cell rule, a workspace that is too short, and what dsim_clearance refuses
 * of the grid. */
typedef struct dsim_clearance_sweep_args {
  float*    prev;           /* [3][n_pad] SoA, world frame; updated to the current positions unless KEEP_PREV */
  float     margin, sag, travel;
  int32_t   flags;
  float*    clearance_out;  /* [n_pad] */
  int32_t*  nearest_out;    /* nullable [n_pad] */
  uint64_t* pairs_out;      /* nullable device counter */
  uint64_t* unswept_out;    /* nullable device counter */
} dsim_clearance_sweep_args;
int64_t dsim_clearance_sweep_workspace(int64_t m, int32_t nx, int32_t ny);
int dsim_clearance_sweep(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_downwash_args* grid,
                         const dsim_clearance_sweep_args* args);

/* Depth camera: per-drone depth and segmentation images of the obstacle set.  The reference's envs keep, with
 * vision_attributes=True, an rgb / depth / segmentation image per drone from p.getCameraImage (BaseAviary._getDroneImages,
 * BaseAviary.py:794-853).  Depth and segmentation of the STATIC world are geometry and are reproduced here by casting one ray
 * per pixel against the set; two deviations from Bullet's renderer: the other drones are not drawn (dsim_depth_image_drones below
 * draws them, as spheres), and there is no RGB.
 *
 * Camera of drone i (line by line what _getDroneImages hands to computeViewMatrix / computeProjectionMatrixFOV), in the frame
 * p = p_i - offset_i of the drone's task, with L = dsim_type_params.arm of its type:
 *     eye = p + (0, 0, L)     target = p + R(quat_i) (1000, 0, 0)     up = (0, 0, 1)     near = L
 *     f = normalize(target - eye)     s = normalize(f x up)     u = s x f     th = tan(fov / 2)
 *     d(r, c) = f + ((c + 1/2) / W 2 - 1) th aspect s + (1 - (r + 1/2) / H 2) th u        row r from the top, column c
 * d is not normalised, so the ray parameter t of a hit IS its eye-space depth.  A pixel takes the nearest hit with
 * near <= t <= far over both faces of every triangle; DSIM_CAM_GROUND adds the plane z = 0 of the task frame (the reference always
 * loads plane.urdf) as an analytic ray-plane hit, also for rays that never enter the set's box, reported as body DSIM_SEG_GROUND.
 *     depth_out[cam][r][c]  the depth-buffer value PyBullet returns, far (t - near) / (t (far - near)), 1.0 where nothing is hit;
 *                           with DSIM_CAM_METRIC t itself in metres, +inf where nothing is hit
 *     seg_out[cam][r][c]    the BODY index of the hit triangle, -1 for none, DSIM_SEG_GROUND for the plane; nullable
 * A camera whose drone state (or offset) is not finite, whose cam_index entry is outside [0, n_pad), or whose basis is degenerate
 * (|f x up|^2 < 1e-12: a vehicle pitched to the vertical, where Bullet's view matrix is NaN) has no defined image: it gets the
 * no-hit value and -1 everywhere; nothing faults and the call returns DSIM_OK.
 *
 * The ray grid.  The watch grid lists a triangle in every cell within `reach` of it — at a gate's size every cell lists every
 * triangle — so rays walk a SECOND grid of the same set: reach = 0 in dsim_obstacle_grid, a triangle listed only in the cells
 * its bounding box touches (plus the hundredth-of-a-cell slack), box = the set's own grown by that slack, cell edge from
 * bounding-box diagonal / (2 cbrt(n_tri)), doubled until the caps of the watch grid hold.  dsim_obstacle_ray_grid_plan / _build
 * are its host-only half (as dsim_obstacle_grid_plan / _build); dsim_obstacles_enable_rays plans, builds and uploads it for a
 * device set, SYNCHRONISES (not inside a capture) and returns DSIM_OK at once when the set already has it.
 *
 * dsim_depth_image: stream-ordered, allocates nothing, never synchronises (it may be captured); the outputs are the caller's,
 * float32 / int32 [n_cam][height][width].  cam_index: int32 [n_cam] (device), drone indices in STORAGE order, NULL = drones
 * 0 .. n_cam - 1 (n_cam <= n_pad then).  offset and type_id as in dsim_obstacle_clearance.  DSIM_E_ARG, nothing written: a
 * null ctx / set / params / depth_out, a set without rays enabled, width or height outside 1 .. 1024, fov_deg outside (0, 180),
 * aspect <= 0, far <= 0 or not finite, n_cam < 1, type_id missing with several types, any type with
 * arm <= 0.  One lane per pixel; a wave is an 8 x 8 pixel tile of one camera. */
enum { DSIM_CAM_METRIC = 1u << 0, DSIM_CAM_GROUND = 1u << 1 };
#define DSIM_SEG_GROUND (-2)
typedef struct dsim_camera_params {
  int32_t  width, height;  /* 1 .. 1024 each (the reference: IMG_RES = [64, 48])                                  */
  float    fov_deg;        /* vertical field of view (the reference: 60)                                          */
  float    aspect;         /* scales the horizontal extent (the reference passes 1.0 at 64 x 48)                  */
  float    far;            /* far plane [m] (the reference: 1000); near is the arm of the drone's type            */
  uint32_t flags;          /* DSIM_CAM_*                                                                          */
} dsim_camera_params;
int dsim_obstacle_ray_grid_plan(const float* tri, int64_t n_tri, dsim_obstacle_grid* out);
int dsim_obstacle_ray_grid_build(const float* tri, int64_t n_tri, const dsim_obstacle_grid* g, int32_t* cell_start, int32_t* cell_tri);
int dsim_obstacles_enable_rays(dsim_ctx* ctx, dsim_obstacles* set);
int dsim_depth_image(dsim_ctx* ctx, void* stream, dsim_view state, const dsim_obstacles* set,
                     const dsim_camera_params* params, int64_t n_cam, const int32_t* cam_index,
                     const float* offset, const uint8_t* type_id, float* depth_out, int32_t* seg_out);

/* The other drones in the images.  The reference renders the whole Bullet world, so every other vehicle appears in dep and seg;
 * dsim_depth_image_drones is dsim_depth_image with the drones of the world drawn as well — two deviations from Bullet's renderer:
 * a drone is drawn as its BOUNDING SPHERE, not as its mesh, and the camera's OWN drone is never drawn (its eye sits L above its
 * own centre, usually inside its own sphere).
 *
 * Every other drone j of the world with R_j = dsim_type_params.collision_sphere > 0 (or radius_all[j] > 0) is the sphere of
 * radius R_j about its STORED position p_j.  The sphere ray starts at the eye in the world frame, e_w = p_i + (0, 0, L); the
 * triangles and the plane keep the task-frame eye e_w - offset_i; the direction d is the same unnormalised pixel ray, so t is
 * eye-space depth in both and the two are compared directly.  A sphere is hit at the smallest root t of |e_w + t d - p_j| = R_j
 * with near <= t <= min(far, range); a first root below near gives way to the second (both faces are seen, as with triangles).
 * The pixel takes the nearest of the triangle, plane and sphere hits.  R = 0: not drawn.  A drone whose position is not finite is
 * not drawn and faults nothing.  seg_out reports a drone hit as DSIM_SEG_DRONE(k) = -3 - k, k the drone's world index or, with a
 * label table (int32 [m], device), label[world index]; -1 and DSIM_SEG_GROUND keep their meaning, body indices stay >= 0.
 *
 * The drones are binned per call, on the stream, on the xy grid of `grid` exactly as dsim_clearance bins them (pos_all NULL: the
 * world is this fleet, read from the state block; pos_all with radius_all: the gathered world, this block at local_offset; a
 * halo plan: DSIM_E_UNSUPPORTED), cell >= 2 R_max (R_max over the type table; with radius_all the caller keeps cell >= 2 max
 * radius_all).  A ray walks the xy cells and tests the spheres of the cells adjacent to its own, which is exact for such cells.
 * The box [xmin, xmin + nx cell] x [ymin, ymin + ny cell] need not hold every drone: one outside it is still drawn exactly, from
 * a list every ray tests — expected to be empty or short — and counted into *outside_out (nullable device counter, += per call),
 * so that the host can see the list grow and re-measure its box.  set may be NULL: a world of drones and, with DSIM_CAM_GROUND,
 * the plane.  Stream-ordered, allocates nothing, may be captured (a replay assumes nothing about earlier calls): grid->workspace
 * holds dsim_depth_image_drones_workspace(m, nx, ny) int32 entries and is the call's until it has run.  The call drops the
 * context's record of the downwash grid (as dsim_downwash_reset): a dsim_step that binned ahead for the next dsim_downwash is not
 * vouched for, that query bins the fleet itself.  DSIM_E_ARG, nothing enqueued: what dsim_depth_image refuses (a NULL set
 * excepted), a null drones / grid / workspace, range <= 0 or NaN, cell <= 0 or < 2 R_max, nx or ny < 1, m < 1 (pos_all NULL:
 * m is the fleet's size, m > n_pad is refused), a workspace too short, radius_all without pos_all or the reverse. */
#define DSIM_SEG_DRONE(k) (-3 - (k))
typedef struct dsim_camera_drones {
  const dsim_downwash_args* grid;   /* xy grid as for dsim_clearance (pos_all NULL: this fleet; halo plan: DSIM_E_UNSUPPORTED) */
  const float*   radius_all;        /* with grid->pos_all, as dsim_clearance */
  const int32_t* label;             /* nullable [m]: k of DSIM_SEG_DRONE per world index */
  float          range;             /* > 0: drones are drawn for t <= min(far, range) */
  uint64_t*      outside_out;       /* nullable device counter: += drones binned outside the box */
} dsim_camera_drones;
int64_t dsim_depth_image_drones_workspace(int64_t m, int32_t nx, int32_t ny);
int dsim_depth_image_drones(dsim_ctx* ctx, void* stream, dsim_view state, const dsim_obstacles* set,
                            const dsim_camera_params* params, int64_t n_cam, const int32_t* cam_index,
                            const float* offset, const uint8_t* type_id, const dsim_camera_drones* drones,
                            float* depth_out, int32_t* seg_out);

/* Obstacle scenes: per-drone placements of ONE prototype set, for the watch and the camera.  A set is one soup in one frame, which
 * serves any number of replicas of one task; a fleet whose drones fly courses of their own has its gates at each drone's own
 * waypoints.  Distances and ray parameters do not change under a rotation and a shift, so one prototype is instanced at any number
 * of poses: its grids, records and LDS staging stay as they are, and only the query point, or the ray, goes into the placement's
 * frame.  K scenes hold up to G placements each (1 <= G <= 32, K G <= 2^22); drone i looks at scene scene_id[i].
 *
 * dsim_scenes_create: place_host [K][G][12] (host) is R row-major, then t, of the map x_task = R x_proto + t of each placement;
 * count_host [K] (host, each 0 .. G; NULL: G everywhere) says how many slots of a scene are used — a scene may be empty, and the
 * entries of slots at or above the count are never looked at.  Every used R must be finite and orthonormal to 1e-5 with det > 0,
 * every t finite: DSIM_E_ARG otherwise, as for a null pointer or K, G outside their limits.  Allocates, uploads and SYNCHRONISES
 * (not inside a capture; neither is dsim_scenes_destroy, which waits for the work that may still read the table).  The prototype
 * must outlive the scenes.
 *
 * Every output names a hit triangle by the INSTANCE-MAJOR body index g n_bodies + body >= 0: g the placement's slot in the drone's
 * scene, n_bodies = 1 + the largest body index of the prototype.  -1 (none) and DSIM_SEG_GROUND keep their meaning.
 *
 * dsim_obstacle_clearance_scenes is dsim_obstacle_clearance on the placed set: with q_i = p_i - offset_i and s = scene_id[i],
 *     clearance_out[i] = min(margin, min over placements g < count[s] of min_t dist(R_g^T (q_i - t_g), triangle t) - R_i)
 *     nearest_out[i]   = the instance-major body that attains the minimum (the lowest slot among equals), -1 when none is below
 *                        margin
 * (subtract first, then rotate: R^T q - R^T t cancels digits at offsets of 128 m, R^T (q - t) does not).  Ownership, stream
 * ordering, "allocates nothing, never synchronises, may be captured" and the counters (DSIM_Q_OBSTACLE_CONTACTS, contacts_out) are
 * dsim_obstacle_clearance's; scene_id is int32 [n_pad] (device, storage order like offset).  A scene_id[i] outside [0, K) means no
 * obstacles — (margin, -1), a defined case: a drone may have no gates.  DSIM_E_ARG, nothing enqueued: everything
 * dsim_obstacle_clearance refuses (R_max + margin > reach of the PROTOTYPE's grid among it), a null scenes or scene_id.  A drone
 * that is out of reach of every placement of its scene reads its position (offset, type), its id and the first 16 bytes of each
 * of the scene's G slots, and writes its two outputs.
 *
 * dsim_depth_image_scenes is dsim_depth_image on the placed set: the camera of drone i sees the placements of scene scene_id[i]
 * (an id outside [0, K): the plane or the background only); the plane z = 0 stays in the task frame.  The arguments behind
 * `params` are dsim_depth_image's.  DSIM_E_ARG, nothing enqueued: everything dsim_depth_image refuses (a prototype without rays
 * enabled among it), a null scenes or scene_id.  The other drones are not drawn: there is no placed dsim_depth_image_drones. */
typedef struct dsim_scenes dsim_scenes;
int dsim_scenes_create(dsim_ctx* ctx, const dsim_obstacles* proto, const float* place_host, const int32_t* count_host, int64_t K,
                       int32_t G, dsim_scenes** out);
int dsim_scenes_destroy(dsim_ctx* ctx, dsim_scenes* scenes);
int dsim_obstacle_clearance_scenes(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_scenes* scenes,
                                   const int32_t* scene_id, const float* offset, const uint8_t* type_id, float margin,
                                   float* clearance_out, int32_t* nearest_out, uint64_t* contacts_out);
int dsim_depth_image_scenes(dsim_ctx* ctx, void* stream, dsim_view state, const dsim_scenes* scenes, const int32_t* scene_id,
                            const dsim_camera_params* params, int64_t n_cam, const int32_t* cam_index,
                            const float* offset, const uint8_t* type_id, float* depth_out, int32_t* seg_out);

/* Moving scenes: per-placement motion of a dsim_scenes, evaluated on the device in stream order.  Every placed call above and
 * below (the watch, the witness, the camera, the scanner, line of sight, the gate passage watch) reads the scenes' table from
 * device memory when its kernel runs, so dsim_scenes_move moves the world for all of them at once; none of them changes.
 *
 * The law.  Placement (k, g) has the base pose (R0, t0) dsim_scenes_create was given and one dsim_scene_motion record.  At scene
 * time tau = t_start + dt * (*clock)  (clock: a device counter the caller advances, dsim_counter_add; NULL: 0 — it is read when
 * the kernel runs, so a replayed capture, whose arguments are frozen, still puts the world where it belongs):
 *     s      = sin(omega tau + phase)
 *     t(tau) = t0 + vel tau + amp s
 *     theta  = rate tau + swing s
 *     R(tau) = Rot(axis, theta) R0,   Rot(k, theta) v = v cos(theta) + (k x v) sin(theta) + k (k . v) (1 - cos(theta))
 * a rotation about the placement's own origin, applied to each column v of R0.  Everything is evaluated in double from the
 * floats given and rounded to float once; a moving slot's record becomes c_task = R(tau) box_c + t(tau) (box_c: the centre of the
 * prototype's box as dsim_scenes_create rounded it), its r_cull as it was, and R(tau), t(tau) in the layout dsim_scenes_create
 * writes.  A record of all zeros is a static placement: its table entry is never rewritten.  Neither is a slot at or above its
 * scene's count, whose record is not looked at.
 *
 * dsim_scenes_motion_set: motion_host [K][G] (host).  DSIM_E_ARG with nothing changed: a null ctx or scenes; a non-finite entry
 * in a used slot; an axis that is neither of unit length to 1e-5 nor zero with rate == swing == 0.  The first call keeps device
 * copies of the base table and of the records; a later call replaces the records and puts the base table back first; NULL
 * detaches the motion, frees both and restores the base table bit for bit.  Allocates, copies and synchronises the device, as
 * dsim_scenes_create does (not inside a capture).  dsim_scenes_destroy frees what is attached.
 *
 * dsim_scenes_move: stream-ordered; allocates nothing, never synchronises, may be captured.  One lane per slot.  DSIM_E_ARG,
 * nothing enqueued: a null ctx or scenes, scenes without a motion, a non-finite dt or t_start.  Calls that read the scenes on
 * the SAME stream are ordered behind it; ordering against work on other streams is the caller's business.
 *
 * dsim_scenes_read: waits for `stream`, then hands back the table as the device holds it: place_host_out [K][G][12] (host), R
 * row-major then t per slot, exactly the floats of the table (the layout dsim_scenes_create takes, so a static scenes created
 * from it holds the same R and t); NaN in the slots at or above their scene's count.  DSIM_E_ARG: a null ctx, scenes or out.
 *
 * dsim_scenes_move_twist: dsim_scenes_move — the same kernel, the same table bit for bit — that also writes the TWIST of every
 * moving placement at that scene time, the derivative of the law off the same sine and cosine:
 *     t'     = vel + amp omega cos(omega tau + phase)
 *     theta' = rate + swing omega cos(omega tau + phase),   w = theta' axis     (the axis is fixed in the task frame: the
 *                                                                                placement's angular velocity in task axes)
 * in double, rounded to float once.  twist_out: caller-owned device memory, [K G][8] floats, 16-byte aligned: (t'.xyz, 0, w.xyz, 0)
 * per slot.  Only moving slots are written; static and unused slots are never touched, so the caller zeroes the table once, and
 * again after a new dsim_scenes_motion_set.  A material point of the placement at task-frame position x moves with
 * t' + w x (x - t(tau)): dsim_obstacle_witness_scenes_vel below.  The promises of dsim_scenes_move hold; DSIM_E_ARG, nothing
 * enqueued: what dsim_scenes_move refuses (scenes without a motion among it), a null twist_out. */
typedef struct dsim_scene_motion {
  float vel[3];    /* [m/s]                                                    */
  float amp[3];    /* [m]                                                      */
  float omega;     /* [rad/s]                                                  */
  float phase;     /* [rad]                                                    */
  float axis[3];   /* unit, task frame; or zero with rate == swing == 0        */
  float rate;      /* [rad/s]                                                  */
  float swing;     /* [rad]                                                    */
  float pad_[3];   /* to 64 bytes; not looked at                               */
} dsim_scene_motion;
int dsim_scenes_motion_set(dsim_ctx* ctx, dsim_scenes* scenes, const dsim_scene_motion* motion_host);
int dsim_scenes_move(dsim_ctx* ctx, void* stream, dsim_scenes* scenes, const uint64_t* clock, double dt, double t_start);
int dsim_scenes_move_twist(dsim_ctx* ctx, void* stream, dsim_scenes* scenes, const uint64_t* clock, double dt, double t_start,
                           float* twist_out);
int dsim_scenes_read(dsim_ctx* ctx, void* stream, const dsim_scenes* scenes, float* place_host_out);

/* The obstacle witness: the point watch's answer and WHERE the closest point lies.  A watch gives one scalar per drone and no
 * direction; a potential field, a velocity obstacle, a control-barrier filter (h = clearance, grad h = the unit vector away from
 * the closest point) and an obstacle observation need the vector.  With q_i = p_i - offset_i, R_i and margin as in
 * dsim_obstacle_clearance, w* the point of the set (dsim_obstacle_witness) or of the placements of scene scene_id[i]
 * (dsim_obstacle_witness_scenes) closest to q_i and d = |q_i - w*|:
 *     clearance_out[i], nearest_out[i], the counters   what dsim_obstacle_clearance / _scenes write on the same inputs, bit for bit
 *     rel_out[k][i]    = (w* - q_i)_k                  SoA [3][n_pad] (device), required.  A relative vector: offsets of 128 m cost it
 *                                                      no digits.  World axes; with DSIM_WITNESS_BODY_FRAME the drone's body axes,
 *                                                      R(quat_i)^T (w* - q_i), the quaternion (fields 3 .. 6 of `state`, x y z w,
 *                                                      any positive length) read for the drones that have a witness only
 *     triangle_out[i]  = the triangle that holds w*    [n_pad], nullable; on scenes instance-major, g n_tri + t, as the body is
 *                                                      g n_bodies + body.  (Of the triangles that share an edge or a vertex with
 *                                                      w* on it: the one the walk met first.)
 * A drone for which the point watch answers (margin, -1) — out of reach, R_i = 0, a NaN position, a scene id outside [0, K) — gets
 * rel = 0 exactly and triangle = -1.  |rel| = d = clearance + R_i up to rounding, and the unit direction is rel / (clearance + R_i):
 * the library does not normalise, d -> 0 is the caller's to guard.  In the face region of a triangle w* = q - (n . (q - a)) n,
 * in the edge and vertex regions a + v ab + w ac with the barycentric (v, w) whose distance the search minimised.  The position of
 * a closest point is worse conditioned than its distance: where two triangles of a flat face lie within E of each other in
 * distance, the witness may sit on either, up to sqrt(2 d E) apart.
 * Stream-ordered, allocates nothing, never synchronises (may be captured).  DSIM_E_ARG, nothing enqueued: everything
 * dsim_obstacle_clearance (_scenes) refuses, a null args or rel_out, an unknown flag; DSIM_E_LAYOUT: DSIM_WITNESS_BODY_FRAME on a
 * view of fewer than 7 fields.
 *
 * dsim_obstacle_witness_scenes_vel: the witness on MOVING scenes, with the velocity of the closest point.  Against a moving
 * obstacle the filters above need h' = n . (v_drone - v_obstacle); differencing two witnesses mixes in the drone's own motion and
 * jumps when the winning triangle changes, while the device knows the answer.  It writes everything
 * dsim_obstacle_witness_scenes writes, bit for bit, and
 *     vel_out[k][i]    = (t'_g + w_g x r)_k            SoA [3][n_pad] (device), required: the velocity of w* as a material point of
 *                                                      the placement g that holds it, from that slot of `twist`, the table
 *                                                      dsim_scenes_move_twist wrote ([K G][8] floats, device).  r = R_g (l + v_l), with
 *                                                      l the query point and v_l the closest-point vector in the placement's
 *                                                      frame: relative quantities, so offsets of 128 m cost it no digits.  World axes;
 *                                                      with DSIM_WITNESS_BODY_FRAME R(quat_i)^T of it.  The obstacle point's OWN
 *                                                      velocity, not the velocity relative to the drone.
 * A drone without a witness gets zeros, as in rel_out; a witness on a static placement (a zeroed slot of `twist`) reads 0 in
 * every component.  The two twist quarters of the winner are read once, behind the search, by the drones that have a witness.
 * DSIM_E_ARG, nothing enqueued and nothing written: what dsim_obstacle_witness_scenes refuses, a null twist or vel_out. */
enum { DSIM_WITNESS_BODY_FRAME = 1 };   /* rel_out in the drone's body axes */
typedef struct dsim_witness_args {
  const float*   offset;        /* SoA [3][n_pad] or NULL, as dsim_obstacle_clearance                      */
  const uint8_t* type_id;       /* [n_pad]; required with more than one type                               */
  float          margin;        /* > 0                                                                      */
  int32_t        flags;         /* DSIM_WITNESS_BODY_FRAME                                                  */
  float*         clearance_out; /* [n_pad]; required                                                        */
  int32_t*       nearest_out;   /* [n_pad], nullable                                                        */
  float*         rel_out;       /* SoA [3][n_pad]; required                                                 */
  int32_t*       triangle_out;  /* [n_pad], nullable                                                        */
  uint64_t*      contacts_out;  /* device counter, nullable                                                 */
} dsim_witness_args;
int dsim_obstacle_witness(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_obstacles* set,
                          const dsim_witness_args* args);
int dsim_obstacle_witness_scenes(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_scenes* scenes,
                                 const int32_t* scene_id, const dsim_witness_args* args);
int dsim_obstacle_witness_scenes_vel(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_scenes* scenes,
                                     const int32_t* scene_id, const dsim_witness_args* args, const float* twist, float* vel_out);

/* Obstacle witnesses: the m closest BODIES of every drone, each with its vector.  The witness above answers for the one closest
 * point of the whole world; a drone between two gates, or between a wall and a moving gate, has two active constraints, and a
 * repulsion built on the nearer one alone jumps when the winner changes.  With q_i, R_i and margin as above, d_b the least distance
 * from q_i to a triangle of body b (dsim_obstacle_witnesses: the bodies of the set; dsim_obstacle_witnesses_scenes: the
 * instance-major bodies g n_bodies + body of the placements g < count of scene scene_id[i]) and c_b = d_b - R_i: the witnesses of
 * drone i are the bodies with c_b < margin, ascending in d_b, the first m of them, 1 <= m <= DSIM_WITNESSES_MAX.  Slot-major, so that
 * every store of a wave is contiguous, for slot s < m:
 *     clearance_out[s][i]                              [m][n_pad] (device), required; c_b, or margin for an unfilled slot
 *     body_out[s][i]                                   [m][n_pad], required; b, or -1
 *     rel_out[s][k][i]                                 [m][3][n_pad], required; the vector from q_i to the closest point of b, in
 *                                                      world axes or with DSIM_WITNESS_BODY_FRAME in the drone's body axes (the
 *                                                      quaternion is read once per drone); exact zeros for an unfilled slot
 *     triangle_out[s][i]                               [m][n_pad], nullable; the triangle of b that holds the point, on scenes
 *                                                      instance-major g n_tri + t; -1
 *     count_out[i]                                     [n_pad], nullable; the number of slots filled, min(bodies within the margin, m).
 *                                                      count == m may hide further bodies: an exact count beyond m would need a
 *                                                      memory of the bodies the walk evicted, which it does not keep
 *     vel_out[s][k][i]                                 [m][3][n_pad], nullable, on scenes with `twist` (the table
 *                                                      dsim_scenes_move_twist wrote) and only with it: the velocity of each
 *                                                      witness as a material point of its OWN placement, what
 *                                                      dsim_obstacle_witness_scenes_vel gives for the one, in the witness's axes;
 *                                                      zeros for an unfilled slot and on a static placement
 * Ties.  A candidate enters the list or moves up in it only on a strict <: an exact tie between two bodies keeps the one the walk
 * met first, an exact tie between two triangles of one body keeps the first triangle, and placements are walked in slot order.
 * Hence, for every m, slot 0 IS the witness: clearance_out[0], body_out[0], rel_out[0], triangle_out[0] and vel_out[0] are what
 * dsim_obstacle_witness / _scenes / _scenes_vel write on the same inputs.  The counters keep their meaning: one per drone whose
 * slot-0 clearance is negative, added to the ctx's shards (DSIM_Q_OBSTACLE_CONTACTS) and to contacts_out.
 * Stream-ordered, allocates nothing, never synchronises (may be captured).  DSIM_E_ARG, nothing enqueued and every output
 * untouched: a null args, clearance_out, body_out or rel_out; m outside 1 .. DSIM_WITNESSES_MAX; an unknown flag; twist and vel_out
 * not both given or both null, or either given to dsim_obstacle_witnesses; everything the witness refuses.  DSIM_E_LAYOUT:
 * DSIM_WITNESS_BODY_FRAME on a view of fewer than 7 fields. */
enum { DSIM_WITNESSES_MAX = 8 };
typedef struct dsim_witnesses_args {
  const float*   offset;        /* SoA [3][n_pad] or NULL, as dsim_obstacle_clearance                      */
  const uint8_t* type_id;       /* [n_pad]; required with more than one type                               */
  float          margin;        /* > 0                                                                      */
  int32_t        m;             /* 1 .. DSIM_WITNESSES_MAX                                                  */
  int32_t        flags;         /* DSIM_WITNESS_BODY_FRAME                                                  */
  float*         clearance_out; /* [m][n_pad]; required                                                     */
  int32_t*       body_out;      /* [m][n_pad]; required                                                     */
  float*         rel_out;       /* [m][3][n_pad]; required                                                  */
  int32_t*       triangle_out;  /* [m][n_pad], nullable                                                     */
  int32_t*       count_out;     /* [n_pad], nullable                                                        */
  uint64_t*      contacts_out;  /* device counter, nullable                                                 */
  const float*   twist;         /* [K G][8] (device), nullable; scenes only, with vel_out                   */
  float*         vel_out;       /* [m][3][n_pad], nullable; with twist                                      */
} dsim_witnesses_args;
int dsim_obstacle_witnesses(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_obstacles* set,
                            const dsim_witnesses_args* args);
int dsim_obstacle_witnesses_scenes(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_scenes* scenes,
                                   const int32_t* scene_id, const dsim_witnesses_args* args);

/* Velocity safety filter: the consumer of dsim_knn's and dsim_obstacle_witnesses' records.  Per drone i < n of `state` the input is
 * a wished velocity u_i (world axes, m/s) and the output
 *     v_i = argmin |v - u_i|^2   subject to   a_j . v >= b_j   for every row j the drone keeps,
 * the control-barrier half-spaces h' + alpha h >= 0 of at most 25 rows, built from the records in this priority order, which is
 * also the bit order of dropped_out:
 *     bit 0          the floor (has_floor): a = (0, 0, 1), b = -alpha (p_z - offset_z - floor - R_i)
 *     bit 1 + s      obstacle slot s < m <= 8 with wit_body[s][i] >= 0: a = -wit_rel[s][:][i] / (wit_clearance[s][i] + R_i),
 *                    b = a . wit_vel[s][:][i] - alpha (wit_clearance[s][i] - buffer_obstacle)      (wit_vel NULL: a static world)
 *     bit 9 + t      neighbour slot t < k <= 16 with 0 <= nb_index[t][i] < n: a = -nb_rel_pos[t][:][i] / nb_dist[t][i],
 *                    h = nb_dist[t][i] - (R_i + R_j) - buffer_drone with j = nb_index[t][i],
 *                    b = a . v_i + share (a . nb_rel_vel[t][:][i] - alpha h), v_i the drone's velocity in the state block
 * R is dsim_type_params.collision_sphere of the drone's type (type_id, required with more than one type; R_j through type_id[j]).  The
 * neighbour row is reciprocal: the pair's relative normal velocity has to change by c = a . rel_vel - alpha h, drone i takes
 * `share` of it, and two drones that see each other and both apply the filter with share = 1/2 meet h' + alpha h >= 0 between
 * them.  The floor and the obstacles give way to nobody: their rows take the whole change.  The records are slot-major as
 * dsim_knn and dsim_obstacle_witnesses (world axes, not DSIM_WITNESS_BODY_FRAME) write them, in storage order.
 * A slot is no row when its index or body is unused, when an entry of it is not finite, or when nb_dist or wit_clearance + R_i is
 * at or below 1e-6 m.  A drone whose u, position, velocity or offset is not finite has no rows.
 * Rows that cannot all be met: the rows are taken in the order above; a row that is infeasible together with the rows already kept
 * is skipped and its bit set in dropped_out[i]; v is the exact projection of u onto the rows kept.  Deterministic; what cannot
 * yield comes first.  A drone with no rows, and a drone whose u meets every row, gets v == u bit for bit.  There is no speed
 * cap in the program: whoever turns v into a command clamps it, and that clamp can undo a row.
 * counters (nullable, device): [0] += drones with v != u, [1] += drones with a dropped row; at most one atomic per wave and counter.
 * Stream-ordered, allocates nothing, never synchronises (may be captured); one drone per lane, every store coalesced; lanes
 * i >= n are not written.  DSIM_E_ARG, nothing enqueued: a null ctx, args, u, v_out or dropped_out; n <= 0 or > n_pad; k outside
 * 0 .. 16 or m outside 0 .. DSIM_WITNESSES_MAX; k == 0 and m == 0 without the floor; a null nb_* with k > 0; a null wit_clearance,
 * wit_body or wit_rel with m > 0; alpha not finite or <= 0; share outside (0, 1]; a buffer that is negative or not finite; a floor
 * that is not finite; more than one type without type_id.  DSIM_E_LAYOUT: a view of fewer than 10 fields. */
enum { DSIM_FILTER_FLOOR_BIT = 0, DSIM_FILTER_OBSTACLE_BIT = 1, DSIM_FILTER_NEIGHBOR_BIT = 9, DSIM_FILTER_ROWS = 25 };
typedef struct dsim_filter_args {
  const float*   u;               /* SoA [3][n_pad] wished velocity; required                                  */
  const float*   offset;          /* SoA [3][n_pad] or NULL, as dsim_obstacle_clearance (the floor reads z)    */
  const uint8_t* type_id;         /* [n_pad]; required with more than one type                                 */
  float          alpha;           /* > 0 [1/s]: the barrier's rate                                             */
  float          share;           /* (0, 1]: the part of a pair's change this drone takes                      */
  float          buffer_drone;    /* >= 0 [m], kept between two bounding spheres                               */
  float          buffer_obstacle; /* >= 0 [m], kept between a bounding sphere and the world                    */
  float          floor;           /* [m] height of the floor in the task frame, with has_floor                 */
  int32_t        has_floor;       /* 0: no floor row                                                           */
  int32_t        k;               /* 0 .. 16 neighbour slots                                                   */
  int32_t        m;               /* 0 .. DSIM_WITNESSES_MAX obstacle slots                                    */
  const int32_t* nb_index;        /* [k][n_pad]     dsim_knn_args.index_out                                    */
  const float*   nb_dist;         /* [k][n_pad]     ... dist_out                                               */
  const float*   nb_rel_pos;      /* [k][3][n_pad]  ... rel_pos_out                                            */
  const float*   nb_rel_vel;      /* [k][3][n_pad]  ... rel_vel_out                                            */
  const float*   wit_clearance;   /* [m][n_pad]     dsim_witnesses_args.clearance_out                          */
  const int32_t* wit_body;        /* [m][n_pad]     ... body_out                                               */
  const float*   wit_rel;         /* [m][3][n_pad]  ... rel_out, world axes                                    */
  const float*   wit_vel;         /* [m][3][n_pad]  ... vel_out, nullable                                      */
  float*         v_out;           /* SoA [3][n_pad]; required (may be u: a lane reads its u before it writes)  */
  int32_t*       dropped_out;     /* [n_pad]; required                                                         */
  uint64_t*      counters;        /* device [2], nullable: += drones changed, += drones with a dropped row     */
} dsim_filter_args;
int dsim_velocity_filter(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_filter_args* args);

/* Range scanner: a fan of range beams per drone, for EVERY drone — the sensor real vehicles carry (a ToF ring, a downward altimeter,
 * a small lidar fan).  A watch gives one scalar per drone and no direction; the camera gives direction at thousands of rays per
 * drone, which is why it serves a few carriers.  dsim_range_scan casts n_beams rays per drone, one drone per lane.
 *
 * The ray.  For drone i < n and beam b the origin is e = p_i - offset_i, the drone's centre in its task frame, and the direction
 * d = R(quat_i) beam_b, R formed from the unnormalised quaternion exactly as the camera forms it (s = 2 / |q|^2).  d is NOT
 * normalised: t is in units of |beam_b|, metres for a unit beam.  The beam takes the nearest hit with t_min <= t <= t_max over
 *   - both faces of every triangle of `set`;
 *   - with `scenes`, every placement of scene scene_id[i], the ray taken into the placement's frame (subtract first, then rotate,
 *     as dsim_depth_image_scenes does); an id outside [0, K): no obstacles;
 *   - with DSIM_SCAN_GROUND, the plane z = 0 of the task frame: analytic, also for rays that never enter a box;
 *   - with `drones`, the bounding sphere of every OTHER drone j with R_j > 0, as dsim_depth_image_drones draws it: the ray starts
 *     at the STORED position p_i in the world frame with the same d, the first root is taken unless it lies below t_min (then the
 *     second), and the hit must satisfy t <= min(t_max, drones->range).  A drone never sees itself.  Scenes and drones together
 *     are served (the camera refuses that pair).
 *     range_out[b][i] = t of the nearest hit; +inf on a miss, or t_max with DSIM_SCAN_CLAMP
 *     hit_out[b][i]   = the body index; the instance-major g n_bodies + body on scenes; DSIM_SEG_GROUND; DSIM_SEG_DRONE(k) with
 *                       drones->label applied as the camera applies it; -1 on a miss.  Nullable.
 * Both are beam-major [n_beams][n_pad] (device, storage order like offset).  Lanes i >= n are not written.
 *
 * Undefined poses: a non-finite position or quaternion, |q|^2 = 0, a zero or non-finite beam, a beam whose squared length is not
 * finite in float32 (longer than about 1.8e19) — those beams miss and nothing faults.
 * The drone's type plays no part in its own scan (a type with collision_sphere = 0 still scans; it is merely not a target);
 * type_id is what the drones' grid is binned with.
 *
 * Stream-ordered, allocates nothing, never synchronises; may be captured.  With `drones` the fleet is binned per call through the
 * grid of drones->grid (dsim_depth_image_drones has the rules: workspace, outside_out, the box that need not hold every drone) and
 * the call drops the context's record of the downwash grid, as that call does.  DSIM_E_ARG, nothing enqueued: a null ctx, args,
 * beams or range_out; n <= 0 or n > n_pad; n_beams outside 1 .. 64; t_min < 0, t_max <= t_min, either not finite; an unknown flag;
 * a set (or the scenes' prototype) without rays enabled; scenes without scene_id or the reverse; scenes together with a non-NULL
 * set; no world at all (no set, scenes, drones or ground); several types with drones and no type_id; everything
 * dsim_depth_image_drones refuses about `drones` (a halo plan: DSIM_E_UNSUPPORTED). */
enum { DSIM_SCAN_GROUND = 1u << 0,    /* the plane z = 0 of the task frame, body DSIM_SEG_GROUND              */
       DSIM_SCAN_CLAMP  = 1u << 1 };  /* a beam that hits nothing reports t_max instead of +inf               */
typedef struct dsim_scan_args {
  const float*   beams;       /* device [n_beams][3]: beam directions in the BODY frame, used as given        */
  int32_t        n_beams;     /* 1 .. 64                                                                      */
  float          t_min, t_max;/* 0 <= t_min < t_max, both finite                                              */
  uint32_t       flags;       /* DSIM_SCAN_*                                                                  */
  const float*   offset;      /* SoA [3][n_pad] or NULL, as dsim_obstacle_clearance                           */
  const uint8_t* type_id;     /* [n_pad]; required with more than one type when `drones` is given             */
  const dsim_scenes* scenes;  /* nullable: the placed world; then `set` must be NULL (the prototype is its)   */
  const int32_t* scene_id;    /* [n_pad] storage order; with `scenes`, and only with it                       */
  const dsim_camera_drones* drones;   /* nullable: the other drones as their bounding spheres                 */
  float*         range_out;   /* [n_beams][n_pad]: t of the nearest hit                                       */
  int32_t*       hit_out;     /* nullable, same shape: what was hit                                           */
} dsim_scan_args;
int dsim_range_scan(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_obstacles* set,
                    const dsim_scan_args* args);

/* Line of sight: which of a drone's neighbours its obstacles hide, per slot.  dsim_knn tells a drone who its neighbours are,
 * through walls; the watches, the scanner and the camera know the walls, not the neighbours behind them.  dsim_line_of_sight casts,
 * for every drone i < n and slot t < k, the SEGMENT
 *     e + s d,  s in [0, 1],   e = p_i - offset_i (formed in float32 as dsim_range_scan forms it),   d = rel[t][:][i]
 * against the world of the scanner: both faces of every triangle of `set`; with `scenes`, every placement of scene scene_id[i],
 * the segment taken into the placement's frame (subtract first, then rotate; an id outside [0, K): no obstacles); with
 * DSIM_SIGHT_GROUND the plane z = 0 of the task frame, analytic.  d is `rel` as given (world axes, the layout of dsim_knn's
 * rel_pos_out) and is NOT recomputed from positions: a knn record is tested on exactly the vectors it reports, a gathered world of
 * a sharded rank works at this level, and so does any target point (a goal: rel = goal - p).  For dsim_line_of_sight the other
 * drones hide nobody; dsim_line_of_sight_drones (below) lets them.
 *
 * A slot is CAST when its index is not negative (or `index` is NULL), e is finite, and d is finite, not zero, and of a squared
 * length that is finite in float32 (shorter than about 1.8e19).  The hit test is the triangle walk's of the camera and the scanner
 * with near = 0 and far = 1, both ends closed (a wall exactly at the neighbour hides it); the nearest hit wins:
 *     visible_out[t][i] = 1 when the slot was cast and nothing lies in [0, 1];  0 when it is blocked, or was not cast
 *     blocker_out[t][i] = the body of the FIRST hit (instance-major g n_bodies + body on scenes), DSIM_SEG_GROUND for the plane;
 *                         -1 when clear or not cast.  Nullable.
 *     frac_out[t][i]    = s of the first hit; +inf when clear or not cast.  Nullable.
 * All three are slot-major [k][n_pad] (device, storage order like offset), so a slot is one coalesced row and belongs to one
 * workgroup (a small fleet spreads chunks of the slots over the grid as the scanner spreads its beams): there is no packed mask
 * on the device.  Lanes i >= n are not written.  The segment lies in drone i's task frame: with per-drone offsets, i may see j
 * where j does not see i.
 *
 * No bound on the segments' length is asked of the caller: every lane measures the longest slot it will cast in one more pass over
 * its rel rows, and that reach decides what it stages and walks (speed only).  Stream-ordered, allocates nothing, never
 * synchronises; may be captured; all outputs are written with plain vector stores.  DSIM_E_ARG, nothing enqueued: a null ctx,
 * args, rel or visible_out; n <= 0 or n > n_pad; k outside 1 .. 32; an unknown flag; scenes without scene_id or the reverse;
 * scenes together with a non-NULL set; no world at all (no set, no scenes, no ground flag); a set (or the scenes' prototype)
 * without rays enabled. */
enum { DSIM_SIGHT_GROUND = 1u << 0 };  /* the plane z = 0 of the task frame blocks too, body DSIM_SEG_GROUND */
typedef struct dsim_sight_args {
  const float*   rel;          /* device [k][3][n_pad]: the segment of slot t of drone i is e_i + s rel[t][:][i], s in [0, 1]
                                  (world axes; the layout of dsim_knn's rel_pos_out)                               */
  const int32_t* index;        /* device [k][n_pad] or NULL: a slot with index < 0 is not cast (dsim_knn's index_out) */
  int32_t        k;            /* 1 .. 32                                                                      */
  uint32_t       flags;        /* DSIM_SIGHT_GROUND (unknown bits: DSIM_E_ARG)                                 */
  const float*   offset;       /* SoA [3][n_pad] or NULL: e_i = p_i - offset_i, as the scanner                 */
  const dsim_scenes* scenes;   /* nullable: the placed world; then `set` must be NULL (the prototype is its)   */
  const int32_t* scene_id;     /* [n_pad] storage order; with `scenes`, and only with it                       */
  int32_t*       visible_out;  /* [k][n_pad], required: 1 = cast and nothing in [0, 1]; 0 = blocked, or not cast */
  int32_t*       blocker_out;  /* [k][n_pad] or NULL: what hides the neighbour first                           */
  float*         frac_out;     /* [k][n_pad] or NULL: where along the segment                                  */
} dsim_sight_args;
int dsim_line_of_sight(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_obstacles* set,
                       const dsim_sight_args* args);

/* Line of sight among the drones: dsim_line_of_sight with the other drones hiding too, as their bounding spheres.  The segment,
 * the cast rule, the world of triangles and the plane, and the outputs are those above; the segment is ALSO tested against the
 * sphere of radius R_m = collision_sphere of its type (or radius_all[m]) about the STORED position of every other drone m of the
 * world with R_m > 0.
 *   Frame.  The spheres stand at the stored world positions and are met from the stored p_i with the same d = rel[t][:][i]; the
 *     triangles and the plane keep e = p_i - offset_i: the scanner's split.  s is shared, so the nearest of the triangle, plane
 *     and sphere hits wins.
 *   Who never blocks.  Drone i itself, and, when `index` is given, the slot's own target index[t][i]: a WORLD index, as dsim_knn
 *     writes it, compared before any label is applied (the segment ends at the target's centre: without this every neighbour would
 *     hide itself).  With index == NULL (goal segments) only i is left out.
 *   Solid balls, both ends closed, as for triangles.  m blocks when its closed ball meets the closed segment: rho^2 <= R^2,
 *     t0 <= min(1, range) and t1 >= 0, with t0, t1 = tc -+ h in the cancellation-free form of the camera's sphere test;
 *     frac = max(t0, 0).  The camera and the scanner hit a SURFACE (the first root, else the second); the solid ball differs only
 *     for a segment that starts inside another drone's ball: such a drone, already in contact, has all its slots blocked at
 *     frac = 0 (all but a slot whose own target that very drone is).
 *   blocker_out names the drone as DSIM_SEG_DRONE(k) = -3 - k, k the world index or label[world index], as the camera and the
 *     scanner apply the label table.
 *   drones->range bounds s, not metres: a sphere hit needs s <= min(1, range) (1 or more: the whole segment).
 *   A drone whose position is not finite is binned nowhere and hides nobody; a type of radius 0 is no target and still looks.
 * Worlds combine freely: set or scenes, plane, drones; drones alone (no set, no scenes, no ground flag) is a valid world.
 * type_id [n_pad] is what the drones' grid is binned with: required with more than one type.  The fleet is binned per call, on
 * the stream, through drones->grid (dsim_depth_image_drones has the rules: workspace, outside_out, the box that need not hold every
 * drone), and the call drops the context's record of the downwash grid, as that call does.  Stream-ordered, allocates nothing,
 * never synchronises; may be captured.  DSIM_E_ARG, nothing enqueued: what dsim_line_of_sight refuses ("no world at all"
 * excepted), a null drones, several types and no type_id, everything dsim_depth_image_drones refuses about `drones` (a halo plan:
 * DSIM_E_UNSUPPORTED).  dsim_sight_args and dsim_line_of_sight are unchanged. */
int dsim_line_of_sight_drones(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_obstacles* set,
                              const dsim_sight_args* args, const uint8_t* type_id, const dsim_camera_drones* drones);

/* Corridor clearance: is the way there free for a vehicle of my size?  Line of sight casts a segment of zero thickness and the
 * swept watch serves one fixed chord; a local planner asks, for k candidate segments per drone, the clearance of the drone's
 * bounding sphere swept along each.  For every drone i < n and slot t < k:
 *     e  = p_i - offset_i                       (formed in float32, as the watches form it)
 *     d  = rel[t][:][i]                         (world axes, the layout of dsim_knn's rel_pos_out: used as given)
 *     Rs = collision_sphere of its type + sag   (sag >= 0; a type with R = 0 still asks, with the radius sag)
 *     c  = min over the world of dist(segment e -> e + d, .) - Rs
 * The world is the watches': both faces of every triangle of `set`; with `scenes`, every placement of scene scene_id[i] where the
 * table stands at this launch (a table dsim_scenes_move rewrites is seen as it is now), both ends of the segment taken into the
 * placement's frame, the subtraction first (an id outside [0, K): no obstacles); with DSIM_CORRIDOR_GROUND the half-space z <= 0
 * of the task frame, at the distance max(0, min(e.z, e.z + d.z)), as body DSIM_SEG_GROUND.
 *     clearance_out[t][i] = min(margin, c)
 *     body_out[t][i]      = the BODY that attains the minimum (instance-major g n_bodies + body on scenes), -1 when c >= margin.
 *                           Nullable.  Strict <: the ground first, then the placements in slot order, then the lists' order.
 * Both are slot-major [k][n_pad] (device, storage order), written with plain vector stores; lanes i >= n are not written.
 *
 * A slot is NOT EVALUATED when `index` is given and index[t][i] < 0, or when a component of e or d is not finite: it reads
 * clearance = -inf, body = -1 (a slot nobody looked at is never free, as line of sight reads visible = 0 for a slot it did not
 * cast).  A zero d is a valid segment: the point query at the radius Rs.
 *
 * The pieces are dsim_obstacle_sweep's: half = reach - (R_max + sag + margin), K = ceil(|d| / (2 half (1 - 2^-10))), each piece
 * looked up in the cell of its own midpoint, a piece whose midpoint lies outside the grown box reading no list; what a lane
 * stages and walks follows from the segment's bounding box (per placement: from the distance of its cull sphere to the segment),
 * not from its ends.  A slot with K > 32 (or a length float32 does not hold) is UNSERVED: it reads -inf, -1 and adds one to
 * *unserved_out (a device counter, nullable; one atomic per wave and tile at most).  The longest segment served is
 * 64 half (1 - 2^-10).  With the ground alone every finite segment is one piece.
 *
 * A query, not a watch: DSIM_Q_OBSTACLE_CONTACTS is not touched.  Stream-ordered, allocates nothing, never synchronises; may be
 * captured.  DSIM_E_ARG, nothing enqueued: a null ctx, args, rel or clearance_out; n <= 0 or n > n_pad; k outside 1 .. 32; an
 * unknown flag; margin <= 0, sag < 0, either not finite; several types and no type_id; scenes without scene_id or the reverse;
 * scenes together with a non-NULL set; no world at all (no set, no scenes, no ground flag); half < reach / 1024 (make the set
 * with reach >= R_max + sag + margin + half the length one lookup should serve). */
enum { DSIM_CORRIDOR_GROUND = 1u << 0 };  /* the half-space z <= 0 of the task frame counts too, body DSIM_SEG_GROUND */
typedef struct dsim_corridor_args {
  const float*   rel;           /* device [k][3][n_pad]: the segment of slot t of drone i is e_i -> e_i + rel[t][:][i]  */
  const int32_t* index;         /* device [k][n_pad] or NULL: a slot with index < 0 is not evaluated                      */
  int32_t        k;             /* 1 .. 32                                                                                 */
  uint32_t       flags;         /* DSIM_CORRIDOR_GROUND (unknown bits: DSIM_E_ARG)                                         */
  const float*   offset;        /* SoA [3][n_pad] or NULL: e_i = p_i - offset_i, as the watches                            */
  const uint8_t* type_id;       /* [n_pad]; required with more than one type                                               */
  const dsim_scenes* scenes;    /* nullable: the placed world; then `set` must be NULL (the prototype is its)              */
  const int32_t* scene_id;      /* [n_pad] storage order; with `scenes`, and only with it                                  */
  float          margin;        /* > 0                                                                                     */
  float          sag;           /* >= 0 [m]: added to every radius                                                         */
  float*         clearance_out; /* [k][n_pad], required                                                                    */
  int32_t*       body_out;      /* [k][n_pad] or NULL                                                                      */
  uint64_t*      unserved_out;  /* device counter, nullable                                                                */
} dsim_corridor_args;
int dsim_corridor_clearance(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_obstacles* set,
                            const dsim_corridor_args* args);

/* Gate passage watch: which drones flew THROUGH the gates of their scene, in order.  The clearance watches say how close a
 * vehicle came to a gate's frame; a drone that flies round its gate, goes through backwards or never reaches it has a perfect
 * clearance.  Passage is a question about the chord between two states, so the watch keeps its own `prev` under the rules of
 * dsim_obstacle_sweep.  Stream-ordered, allocates nothing, never synchronises; may be captured.
 *
 * The aperture: one planar opening in the PROTOTYPE's frame, the same for every placement.  Centre c, unit normal n (the forward
 * direction), unit in-plane axis u perpendicular to n, v = n x u, half-extents half[0] along u and half[1] along v, a rectangle
 * or the ellipse inscribed in it.  outer[0] >= half[0], outer[1] >= half[1]: an optional rectangle around the opening (the
 * gate's frame seen from the front); (0, 0): none.  The gate index of a placement is its slot g in the scene.
 *
 * For drone i < n with s = scene_id[i] in [0, K), q0 = prev_i - offset_i, q1 = p_i - offset_i, and every slot g < count[s],
 * with l = R_g^T (q - t_g) (subtract first, then rotate, as the placed clearance watch does):
 *     s0 = n.(l0 - c), s1 = n.(l1 - c)          forward crossing: s0 < 0 && s1 >= 0; backward: s0 >= 0 && s1 < 0 (half-open: a
 *                                               state exactly on the plane is counted once across two consecutive chords)
 *     tau = s0 / (s0 - s1), x = l0 + tau (l1 - l0), y = u.(x - c), z = v.(x - c)
 *     inside: |y| <= half[0] && |z| <= half[1]  (rectangle),  (y / half[0])^2 + (z / half[1])^2 <= 1  (ellipse)
 *     fwd_out[i]  bit g: a forward crossing inside the aperture;  back_out[i] bit g: a backward crossing inside it
 *     miss_out[i] bit g: a forward crossing outside the aperture but with |y| <= outer[0] && |z| <= outer[1]: the vehicle went
 *                        over or round the opening (never set without an outer rectangle)
 * Progress: while due_i < count[s] and the due gate has its fwd bit at a tau greater than the last accepted one of this chord,
 * pass_time[due_i][i] := *clock + tau and due_i advances; one chord through three gates standing in order advances by three, the
 * same chord through them in the wrong order by one.  At due_i == count[s] the drone has finished and advances no more; with
 * DSIM_GATE_WRAP due_i returns to 0 instead and laps_i increments.  A due_i outside [0, count[s]) on entry makes no progress.
 * due and laps are in-out, owned by the caller at fixed addresses (a captured and replayed call carries them); due_i is written
 * only when it advanced, laps_i only when it wrapped, pass_time only for the gates passed.
 *
 * The passage time is a double: *clock (a device counter the caller advances between queries, dsim_counter_add; NULL: 0) as the
 * whole part, exact up to 2^53, plus tau in [0, 1] of the chord: the unit is one query, the resolution a float of the chord.
 * It is read from device memory when the kernel runs, so a replayed capture, whose arguments are frozen, stamps the right time.
 *
 * Fleet counters (device uint64, nullable; one atomic per wave and counter at most):
 *     passes_out        advances of due, summed          wrong_way_out     bits set in back_out, summed
 *     out_of_order_out  bits set in fwd_out that did not advance due (a gate that is not due, or a finished course)
 *     misses_out        drones whose due gate — the one due when the query ends — has its miss bit
 *     unswept_out       drones without a usable chord
 * UNSWEPT, as in dsim_obstacle_sweep: a non-finite component of prev_i or p_i, or a chord longer than `travel`.  Such a drone has
 * no event (its masks are 0), makes no progress and is counted once: a teleport across a gate is a reset, not a passage.
 * A scene_id[i] outside [0, K) leaves everything of that drone untouched — masks, due, laps, pass_time, the counters — but prev;
 * so do the slots at or above the count.  Then, unless DSIM_SWEEP_KEEP_PREV is set, prev_i := p_i bit for bit for every i < n.
 * DSIM_SWEEP_KEEP_PREV is a look ahead (on-demand queries, the eager call before a capture): prev, due, laps and pass_time stay as
 * they were; the masks and the counters are those of the query it would have been.
 * DSIM_SWEEP_PRIME: prev_i := p_i for i < n and nothing else; scenes, scene_id and every other field are not looked at.
 *
 * A lane reads the first 16 bytes of each of its scene's G slots and the other 48 only of a slot the chord can reach
 * (|q1 - c_task| <= r_ap + |q1 - q0| is necessary for a crossing point inside the outer rectangle; it decides speed only).
 * DSIM_E_ARG, nothing enqueued: a null ctx / args / prev, n <= 0 or > n_pad, an unknown flag or KEEP_PREV together with PRIME;
 * and unless PRIME: a null scenes / scene_id / due, WRAP without laps, travel <= 0 or not finite, an unknown shape, n or u not of
 * unit length or u not perpendicular to n (each to 1e-5), a half-extent <= 0, an outer rectangle smaller than the aperture in
 * either extent (or only one of its extents given), any non-finite entry of the aperture. */
enum { DSIM_APERTURE_RECT = 0, DSIM_APERTURE_ELLIPSE = 1 };
enum { DSIM_GATE_WRAP = 4 };      /* beside DSIM_SWEEP_KEEP_PREV = 1 and DSIM_SWEEP_PRIME = 2 in dsim_gate_args.flags */
typedef struct dsim_aperture {
  float   center[3];
  float   normal[3];      /* unit: the forward direction                                            */
  float   u[3];           /* unit, perpendicular to normal; v = normal x u                          */
  float   half[2];        /* > 0: half-extents along u and v                                        */
  float   outer[2];       /* (0, 0): none; else outer[k] >= half[k]                                 */
  int32_t shape;          /* DSIM_APERTURE_RECT | DSIM_APERTURE_ELLIPSE                             */
} dsim_aperture;
typedef struct dsim_gate_args {
  dsim_aperture   aperture;
  float           travel;        /* > 0 [m]: a longer chord is unswept                                 */
  int32_t         flags;         /* DSIM_SWEEP_KEEP_PREV | DSIM_SWEEP_PRIME | DSIM_GATE_WRAP           */
  const float*    offset;        /* SoA [3][n_pad] or NULL, as dsim_obstacle_clearance                 */
  float*          prev;          /* SoA [3][n_pad], WORLD frame, in-out; required                      */
  int32_t*        due;           /* [n_pad], in-out; required unless PRIME                             */
  int32_t*        laps;          /* [n_pad], in-out; required with DSIM_GATE_WRAP, else not looked at  */
  const uint64_t* clock;         /* device counter, nullable (0)                                       */
  double*         pass_time;     /* [G][n_pad] slot-major (G of the scenes), nullable                  */
  uint32_t*       fwd_out;       /* [n_pad], nullable                                                  */
  uint32_t*       back_out;      /* [n_pad], nullable                                                  */
  uint32_t*       miss_out;      /* [n_pad], nullable                                                  */
  uint64_t*       passes_out;    /* device counters, each nullable                                     */
  uint64_t*       wrong_way_out;
  uint64_t*       out_of_order_out;
  uint64_t*       misses_out;
  uint64_t*       unswept_out;
} dsim_gate_args;
int dsim_gate_passage(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_scenes* scenes,
                      const int32_t* scene_id, const dsim_gate_args* args);

/* The rotor-noise normals the step kernels draw (diagnostics / distribution studies; no counterpart in the reference, whose
 * draws come from numpy's global generator): for drones [0, n) and the physics sub-steps [0, substeps) of Env.step number
 * step_index, out [substeps][2 * n_act][n_pad] (device) receives the UNIT-variance normals — n_act = 4: rows 0 .. 3 the force noise,
 * 4 .. 7 the moment noise; n_act = 6: rows 0 .. 5 the six normals z of the body wrench (dsim_step_args.noise_seed), rows 6 .. 11 zero —
 * exactly as a launch with the same noise_seed / step_index / phys_substeps / options (DSIM_OPT_NOISE_FINE / _COARSE or neither)
 * draws them.  (dsim_step_args.noise_replay takes PER-ROTOR values, [substeps][2 * n_act][n_pad] times the
 * deviations.  n_act = 4 | 6.  drone_id nullable (the key of drone i's stream: dsim_step_args.drone_id).                 */
int dsim_noise_draw(dsim_ctx* ctx, void* stream, int64_t n, int64_t n_pad, int32_t n_act, uint64_t noise_seed, uint64_t step_index,
                    int32_t substeps, uint32_t options, const int32_t* drone_id, float* out);

/* Diagnostics counters kept by the ctx (device-side, cumulative; this call synchronises `stream`):
 *   DSIM_Q_WLS_FALLBACKS  drones x steps whose 6DOF allocation left the first-iteration fast path and
 *                         ran the full active-set loop of wls_alloc (wls_alloc.py:222-350)
 *   DSIM_Q_WLS_FAILURES   allocations on which the reference would have failed (wls_alloc returns None
 *                         -> `self.cmd += None` raises, INDIControl_6DOF.py:626-630); cmd is left unchanged
 *   DSIM_Q_GROUND_CONTACTS  drone x Env.steps that ended with the vehicle's collision cylinder at or below z = 0, where
 *                         PyBullet's ground plane would have acted (see dsim_type_params.collision_radius)
 *   DSIM_Q_HALO_OVERFLOW  positions dsim_halo_pack selected but could not ship (send_cap too small), or received
 *                         headers that announced more than recv_cap: the force of that step may have missed pairs
 *   DSIM_Q_DW_REUSES      dsim_downwash calls answered from kept candidate lists (dsim_downwash_args.keep)
 *   DSIM_Q_DW_MOVERS      overflow-list entries those calls found, summed: drones that had left the lists' skin (performance
 *                         only — results do not depend on it; / DSIM_Q_DW_REUSES = the mean length every receiver scanned)
 *   DSIM_Q_DRONE_CONTACTS pairs of drones x dsim_clearance calls whose bounding spheres overlapped, where Bullet's world might have
 *                         made the two vehicles collide (see dsim_type_params.collision_sphere; each pair once per call)
 *   DSIM_Q_OBSTACLE_CONTACTS  drones x dsim_obstacle_clearance calls whose bounding sphere overlapped a triangle of the obstacle
 *                         set, where Bullet's world might have made the vehicle collide with a static body                     */
enum { DSIM_Q_WLS_FALLBACKS = 0, DSIM_Q_WLS_FAILURES = 1, DSIM_Q_GROUND_CONTACTS = 2, DSIM_Q_HALO_OVERFLOW = 3,
       DSIM_Q_DW_REUSES = 4, DSIM_Q_DW_MOVERS = 5, DSIM_Q_DRONE_CONTACTS = 6, DSIM_Q_OBSTACLE_CONTACTS = 7 };
int dsim_query(dsim_ctx* ctx, void* stream, int32_t what, int64_t* value_out);

/* error codes */
enum {
  DSIM_OK = 0,
  DSIM_E_ARG = -1,        /* null / inconsistent argument                       */
  DSIM_E_LAYOUT = -2,     /* view violates the layout contract                  */
  DSIM_E_NODEVICE = -3,   /* no HIP device / wrong arch                         */
  DSIM_E_TYPES = -4,      /* bad type table                                     */
  DSIM_E_UNSUPPORTED = -5
};

#ifdef __cplusplus
}
#endif
#endif /* DRONESIM_AMD_H */
