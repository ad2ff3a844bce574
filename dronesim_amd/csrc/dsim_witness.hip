// Obstacle witness (dsim_obstacle_witness, dsim_obstacle_witness_scenes, dsim_obstacle_witness_scenes_vel): the point watch's
// answer and, beside it, the vector from the query point to the closest point of the set (or of the placements of the drone's
// scene) and the triangle that holds it — on moving scenes that point's velocity as well (include/dronesim_amd.h).  Compiled as part of dsim_obstacles.hip, which includes it.  The witness IS the point watch with a
// tail: its kernels are the point watch's two, instantiated with the witness's arguments behind their own
// (k_obstacle_clearance<LDS, WitK>, dsim_obstacles.hip; k_obstacle_clearance_scenes<LDS, WitK>, dsim_scenes.hip), whose walk then
// keeps the winner's record index (obs_cell_walk<.., INDEX>).  What is the witness's own is here: its arguments, the closest point
// off the shared region decision (tri_region), the tail's two steps (wit_point, wit_lane_store) and the entry points.
#pragma once

struct WitK {
  float* rel;                    // SoA [3][n_pad]
  int* triangle;                 // [n_pad] or null
  int body_frame;                // rel in the drone's body axes (the view then has the quaternion: fields 3 .. 6)
};

// ... and with the velocity of the witness beside it (dsim_obstacle_witness_scenes_vel): the scenes' twist table as
// dsim_scenes_move_twist writes it, two quarters per slot, (t'.xyz, 0) and (w.xyz, 0).
struct WitVelK : WitK {
  const float4* twist;           // [K][G][2]
  float* vel;                    // SoA [3][n_pad]
};

// The closest point of one triangle record to q, as the vector from q to it, on the region decision tri_dist2 minimised over
// (tri_region).  Called once per lane, after the walk: the walk carries an index, never a point.
__device__ __forceinline__ void tri_closest(const float4 r0, const float4 r1, const float4 r2, const float4 r3, float qx, float qy,
                                            float qz, float& wx, float& wy, float& wz) {
  float3 to;
  (void)tri_region<true>(r0, r1, r2, r3, qx, qy, qz, &to);
  wx = to.x; wy = to.y; wz = to.z;
}

// The witness of a lane that has one (`in`), from the winner's record — in LDS already, or one 64-byte read through L2 — at the
// point (lx, ly, lz) the walk looked it up with: the vector to the closest point in that frame, and the winner's body.
template <bool LDS>
__device__ __forceinline__ int wit_point(const ObsK& a, const float4* s_rec, int tri, float lx, float ly, float lz, float& wx, float& wy,
                                         float& wz) {
  const float4* r = (LDS ? s_rec : a.rec) + 4 * tri;
  const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
  tri_closest(r0, r1, r2, r3, lx, ly, lz, wx, wy, wz);
  return __float_as_int(r3.w);
}

// The velocity of a witness as a material point of the placement that holds it, v_c = t' + w x r, in world axes: r = R (l + v_l)
// from the local point and the local vector the tail holds, never (q + rel) - t in world coordinates, which at an offset of 128 m
// would cost r five digits.  The slot's two twist quarters are read here, once per lane that has a witness.
__device__ __forceinline__ void wit_velocity(const WitVelK& w, size_t slot, const float4 c0, const float4 c1, const float4 c2,
                                             const float3 l, float vx, float vy, float vz, float& ux, float& uy, float& uz) {
  const float4 td = w.twist[2 * slot], om = w.twist[2 * slot + 1];
  const float lx = l.x + vx, ly = l.y + vy, lz = l.z + vz;
  const float rx = c0.x * lx + c1.x * ly + c2.x * lz, ry = c0.y * lx + c1.y * ly + c2.y * lz, rz = c0.z * lx + c1.z * ly + c2.z * lz;
  ux = td.x + (om.y * rz - om.z * ry); uy = td.y + (om.z * rx - om.x * rz); uz = td.z + (om.x * ry - om.y * rx);
}

// The velocity of lane i into its body axes, R(quat)^T v, as wit_lane_store takes the witness there (stated apart: the witness's
// own instances stay instruction for instruction what they were).
__device__ __forceinline__ void wit_to_body(const ObsK& a, long long i, float& wx, float& wy, float& wz) {
  const float* p = a.st.base + kv_off(a.st, i);
  const long long fs = a.st.field_stride;
  const float qx = p[3 * fs], qy = p[4 * fs], qz = p[5 * fs], qw = p[6 * fs];
  const float s2 = 2.0f / (qx * qx + qy * qy + qz * qz + qw * qw);
  const float xs = qx * s2, ys = qy * s2, zs = qz * s2;
  const float r00 = 1.0f - (qy * ys + qz * zs), r10 = qx * ys + qw * zs, r20 = qx * zs - qw * ys;
  const float r01 = qx * ys - qw * zs, r11 = 1.0f - (qx * xs + qz * zs), r21 = qy * zs + qw * xs;
  const float r02 = qx * zs + qw * ys, r12 = qy * zs - qw * xs, r22 = 1.0f - (qx * xs + qy * ys);
  const float bx = r00 * wx + r10 * wy + r20 * wz, by = r01 * wx + r11 * wy + r21 * wz, bz = r02 * wx + r12 * wy + r22 * wz;
  wx = bx; wy = by; wz = bz;
}

// The lane's vector and triangle beside obs_lane_store's answer: exact zeros and -1 for a lane without a witness.  In the body
// frame the vector goes through R(quat)^T, the quaternion read through the view by the lanes that have a witness only (R(q) as
// k_range_scan forms it, so a quaternion need not be of unit length).
__device__ __forceinline__ void wit_lane_store(const ObsK& a, const WitK& w, long long i, bool live, bool in, float wx, float wy, float wz,
                                               int tri) {
  if (w.body_frame && in) {              // (the flag is the launch's: a wave-uniform branch around a per-lane one)
    const float* p = a.st.base + kv_off(a.st, i);
    const long long fs = a.st.field_stride;
    const float qx = p[3 * fs], qy = p[4 * fs], qz = p[5 * fs], qw = p[6 * fs];
    const float s2 = 2.0f / (qx * qx + qy * qy + qz * qz + qw * qw);
    const float xs = qx * s2, ys = qy * s2, zs = qz * s2;
    const float r00 = 1.0f - (qy * ys + qz * zs), r10 = qx * ys + qw * zs, r20 = qx * zs - qw * ys;
    const float r01 = qx * ys - qw * zs, r11 = 1.0f - (qx * xs + qz * zs), r21 = qy * zs + qw * xs;
    const float r02 = qx * zs + qw * ys, r12 = qy * zs - qw * xs, r22 = 1.0f - (qx * xs + qy * ys);
    const float bx = r00 * wx + r10 * wy + r20 * wz, by = r01 * wx + r11 * wy + r21 * wz, bz = r02 * wx + r12 * wy + r22 * wz;
    wx = bx; wy = by; wz = bz;
  }
  if (live) {
    w.rel[i] = in ? wx : 0.0f;
    w.rel[a.n_pad + i] = in ? wy : 0.0f;
    w.rel[2 * a.n_pad + i] = in ? wz : 0.0f;
    if (w.triangle) w.triangle[i] = in ? tri : -1;
  }
}

// ... and the lane's velocity behind them, through the same rotation in the body frame (the quaternion read before the witness's
// stores, which may alias it for all the compiler knows): exact zeros without a witness.
__device__ __forceinline__ void wit_lane_store(const ObsK& a, const WitVelK& w, long long i, bool live, bool in, float wx, float wy,
                                               float wz, int tri, float ux, float uy, float uz) {
  if (w.body_frame && in) wit_to_body(a, i, ux, uy, uz);
  wit_lane_store(a, static_cast<const WitK&>(w), i, live, in, wx, wy, wz, tri);
  if (live) {
    w.vel[i] = in ? ux : 0.0f;
    w.vel[a.n_pad + i] = in ? uy : 0.0f;
    w.vel[2 * a.n_pad + i] = in ? uz : 0.0f;
  }
}

// what both witness queries refuse and fill alike
static int wit_args(dsim_ctx* ctx, int64_t n, const dsim_view& state, const dsim_obstacles* set, const dsim_witness_args* args, ObsK* a,
                    WitK* w) {
  if (!args || !args->rel_out || (args->flags & ~DSIM_WITNESS_BODY_FRAME)) return DSIM_E_ARG;
  int rc = obs_refuse(ctx, n, state, set, args->type_id, args->margin, 0.0f, args->clearance_out);
  if (rc) return rc;
  rc = obs_kargs(ctx, n, state, set, args->offset, args->type_id, args->margin, args->clearance_out, args->nearest_out,
                 args->contacts_out, a);
  if (rc) return rc;
  w->rel = args->rel_out; w->triangle = args->triangle_out; w->body_frame = (args->flags & DSIM_WITNESS_BODY_FRAME) ? 1 : 0;
  if (w->body_frame) rc = make_kview(state, 7, &a->st);       // (the quaternion behind the position)
  return rc;
}

extern "C" {

int dsim_obstacle_witness(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_obstacles* set,
                          const dsim_witness_args* args) {
  ObsK a;
  WitK w;
  const int rc = wit_args(ctx, n, state, set, args, &a, &w);
  if (rc) return rc;
  return obs_launch(k_obstacle_clearance<true, WitK>, k_obstacle_clearance<false, WitK>, set, a.tiles, stream, a, w);
}

int dsim_obstacle_witness_scenes(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_scenes* scenes,
                                 const int32_t* scene_id, const dsim_witness_args* args) {
  ScnK s;
  int rc = scn_kargs(scenes, scene_id, &s);
  if (rc) return rc;
  const dsim_obstacles* set = scenes->proto;
  ObsK a;
  WitK w;
  rc = wit_args(ctx, n, state, set, args, &a, &w);
  if (rc) return rc;
  return obs_launch(k_obstacle_clearance_scenes<true, WitK>, k_obstacle_clearance_scenes<false, WitK>, set, a.tiles, stream, a, s, w);
}

int dsim_obstacle_witness_scenes_vel(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_scenes* scenes,
                                     const int32_t* scene_id, const dsim_witness_args* args, const float* twist, float* vel_out) {
  if (!twist || !vel_out) return DSIM_E_ARG;
  ScnK s;
  int rc = scn_kargs(scenes, scene_id, &s);
  if (rc) return rc;
  const dsim_obstacles* set = scenes->proto;
  ObsK a;
  WitVelK w;
  rc = wit_args(ctx, n, state, set, args, &a, &w);
  if (rc) return rc;
  w.twist = (const float4*)twist; w.vel = vel_out;
  return obs_launch(k_obstacle_clearance_scenes<true, WitVelK>, k_obstacle_clearance_scenes<false, WitVelK>, set, a.tiles, stream, a, s, w);
}

}  // extern "C"
