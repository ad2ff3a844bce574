// Obstacle witness (dsim_obstacle_witness, dsim_obstacle_witness_scenes): the point watch's answer and, beside it, the vector from
// the query point to the closest point of the set (or of the placements of the drone's scene) and the triangle that holds it
// (include/dronesim_amd.h).  Compiled as part of dsim_obstacles.hip, which includes it: it shares the set's private record, tri_dist2,
// the watches' tile frame (obs_lane, obs_stage_once, obs_lane_store), their arguments and their launcher, and the scenes' table.
#pragma once

struct WitK {
  float* rel;                    // SoA [3][n_pad]
  int* triangle;                 // [n_pad] or null
  int body_frame;                // rel in the drone's body axes (the view then has the quaternion: fields 3 .. 6)
};

// The closest point of one triangle record to q, as the vector from q to it.  The region decisions are tri_dist2's, term for
// term, so the region this picks is the region whose distance the walk minimised: in the vertex and edge regions the barycentric
// (v, w) give a + v ab + w ac - q = -(p - v ab - w ac), whose squared length is what tri_dist2 returned; in the face region the
// point is q - (n . p) n, at |n . p| |n| from q.  Called once per lane, after the walk: the walk carries an index, never a point.
__device__ __forceinline__ void tri_closest(const float4 r0, const float4 r1, const float4 r2, const float4 r3, float qx, float qy,
                                            float qz, float& wx, float& wy, float& wz) {
  const float ax = r0.x, ay = r0.y, az = r0.z, abx = r0.w, aby = r1.x, abz = r1.y, acx = r1.z, acy = r1.w, acz = r2.x;
  const float nx = r2.y, ny = r2.z, nz = r2.w, e00 = r3.x, e01 = r3.y, e11 = r3.z;
  const float px = qx - ax, py = qy - ay, pz = qz - az;
  const float d1 = abx * px + aby * py + abz * pz, d2 = acx * px + acy * py + acz * pz;
  const float d3 = d1 - e00, d4 = d2 - e01, d5 = d1 - e01, d6 = d2 - e11;
  const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  const float d43 = d4 - d3, d56 = d5 - d6;
  const bool rA = d1 <= 0.0f && d2 <= 0.0f;
  const bool rB = d3 >= 0.0f && d4 <= d3;
  const bool rAB = vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f;
  const bool rC = d6 >= 0.0f && d5 <= d6;
  const bool rAC = vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f;
  const bool rBC = va <= 0.0f && d43 >= 0.0f && d56 >= 0.0f;
  float num = 0.0f, den = 1.0f;
  int mode = 6;                        // 0 A, 1 B, 2 AB, 3 C, 4 AC, 5 BC, 6 face: tri_dist2's order
  if (rBC) { mode = 5; num = d43; den = d43 + d56; }
  if (rAC) { mode = 4; num = d2; den = d2 - d6; }
  if (rC) mode = 3;
  if (rAB) { mode = 2; num = d1; den = d1 - d3; }
  if (rB) mode = 1;
  if (rA) mode = 0;
  const float t = den > 0.0f ? num * DSIM_RCP(den) : 0.0f;
  const float v = mode == 1 ? 1.0f : (mode == 2 ? t : (mode == 5 ? 1.0f - t : 0.0f));
  const float w = mode == 3 ? 1.0f : (mode == 4 || mode == 5 ? t : 0.0f);
  const float ex = px - v * abx - w * acx, ey = py - v * aby - w * acy, ez = pz - v * abz - w * acz;
  const float h = nx * px + ny * py + nz * pz;
  wx = mode == 6 ? -(h * nx) : -ex;
  wy = mode == 6 ? -(h * ny) : -ey;
  wz = mode == 6 ? -(h * nz) : -ez;
}

// obs_cell_walk for the point q, keeping the winner's RECORD INDEX instead of its body: the same cell, the same order, the same
// tri_dist2 and the same strict <, so `best` and the winner are the point kernels'.
template <bool LDS>
__device__ __forceinline__ void wit_point_walk(const ObsK& a, const float4* s_rec, float qx, float qy, float qz, int& tri, float& best) {
  const int cx = min(max((int)floorf((qx - a.ox) * a.inv_cell), 0), a.nx - 1);
  const int cy = min(max((int)floorf((qy - a.oy) * a.inv_cell), 0), a.ny - 1);
  const int cz = min(max((int)floorf((qz - a.oz) * a.inv_cell), 0), a.nz - 1);
  const int c = (cz * a.ny + cy) * a.nx + cx;
  const int end = a.cell_start[c + 1];
  for (int k = a.cell_start[c]; k < end; ++k) {
    const int t = a.cell_tri[k];
    const float4* r = (LDS ? s_rec : a.rec) + 4 * t;
    const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
    const float d2 = tri_dist2(r0, r1, r2, r3, qx, qy, qz);
    const bool better = d2 < best;
    best = better ? d2 : best;
    tri = better ? t : tri;
  }
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

// k_obstacle_clearance with the witness: the same tile frame, the same decisions, the same walk order.  Per lane the walk keeps
// the winner's record index; after it, the lanes within the margin evaluate tri_closest once on that record.
template <bool LDS>
__global__ __launch_bounds__(256) void k_obstacle_witness(ObsK a, WitK w) {
  extern __shared__ float4 s_rec[];
  bool staged = false;
  for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const long long i = tile * 256 + threadIdx.x;
    const bool live = i < a.n;
    ObsLane l = {};
    if (live) l = obs_lane(a, i);
    const float qx = l.qx, qy = l.qy, qz = l.qz, R = l.R;
    // (a NaN position fails every comparison: not in the box, clearance = margin, no witness)
    const bool inbox = live && R > 0.0f && qx >= a.lox && qx <= a.hix && qy >= a.loy && qy <= a.hiy && qz >= a.loz && qz <= a.hiz;
    obs_stage_once<LDS>(a, s_rec, staged, inbox);
    float best = INFINITY;
    int tri = -1;
    if (inbox) wit_point_walk<LDS>(a, s_rec, qx, qy, qz, tri, best);     // (a wave with no such lane skips it: the per-wave reject)
    const float c_i = DSIM_SQRT(best) - R;
    const bool in = tri >= 0 && c_i < a.margin;
    float wx = 0.0f, wy = 0.0f, wz = 0.0f;
    int body = -1;
    if (in) body = wit_point<LDS>(a, s_rec, tri, qx, qy, qz, wx, wy, wz);
    obs_lane_store(a, tile, i, live, in, c_i, body);
    wit_lane_store(a, w, i, live, in, wx, wy, wz, tri);
  }
}

// k_obstacle_clearance_scenes with the witness.  The loop over the placements keeps the winner's slot and record index; after
// it, the winner's three columns are read again (the lane read them in the loop: they come from cache), q goes into that
// placement's frame by the loop's own arithmetic, tri_closest gives the local vector and R takes it back: rel = sum_k col_k l_k.
// The triangle is instance-major, g n_tri + t, as the body is g n_bodies + body.
template <bool LDS>
__global__ __launch_bounds__(256) void k_obstacle_witness_scenes(ObsK a, ScnK s, WitK w) {
  extern __shared__ float4 s_rec[];
  bool staged = false;
  for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const long long i = tile * 256 + threadIdx.x;
    const bool live = i < a.n;
    ObsLane l = {};
    int sid = -1;
    if (live) { l = obs_lane(a, i); sid = s.scene_id[i]; }
    const float qx = l.qx, qy = l.qy, qz = l.qz, R = l.R;
    unsigned near = 0u;
    const float4* pl = s.place;
    if (live && R > 0.0f && sid >= 0 && (long long)sid < s.K) {
      pl += 4 * ((size_t)sid * (size_t)s.G);
      for (int g = 0; g < s.G; ++g) {
        const float4 c = pl[4 * g];
        const float ux = qx - c.x, uy = qy - c.y, uz = qz - c.z;
        const float b = (c.w + R + a.margin) * 1.0001f + 1e-5f;                // (-inf for a slot at or above the count)
        near |= (b >= 0.0f && ux * ux + uy * uy + uz * uz <= b * b) ? (1u << g) : 0u;
      }
    }
    obs_stage_once<LDS>(a, s_rec, staged, near != 0u);
    float best = INFINITY;
    int tri = -1, slot = 0;
    while (near != 0u) {                   // (a wave with no such lane skips the loop: the per-wave reject)
      const int g = __ffs((int)near) - 1;
      near &= near - 1u;
      const float4 c0 = pl[4 * g + 1], c1 = pl[4 * g + 2], c2 = pl[4 * g + 3];
      const float tx = qx - c0.w, ty = qy - c1.w, tz = qz - c2.w;
      const float lx = c0.x * tx + c0.y * ty + c0.z * tz, ly = c1.x * tx + c1.y * ty + c1.z * tz, lz = c2.x * tx + c2.y * ty + c2.z * tz;
      if (lx >= a.lox && lx <= a.hix && ly >= a.loy && ly <= a.hiy && lz >= a.loz && lz <= a.hiz) {
        float b2 = best;
        int t2 = -1;
        wit_point_walk<LDS>(a, s_rec, lx, ly, lz, t2, b2);
        if (t2 >= 0) { best = b2; tri = t2; slot = g; }
      }
    }
    const float c_i = DSIM_SQRT(best) - R;
    const bool in = tri >= 0 && c_i < a.margin;
    float wx = 0.0f, wy = 0.0f, wz = 0.0f;
    int body = -1;
    if (in) {
      const float4 c0 = pl[4 * slot + 1], c1 = pl[4 * slot + 2], c2 = pl[4 * slot + 3];
      const float tx = qx - c0.w, ty = qy - c1.w, tz = qz - c2.w;
      const float lx = c0.x * tx + c0.y * ty + c0.z * tz, ly = c1.x * tx + c1.y * ty + c1.z * tz, lz = c2.x * tx + c2.y * ty + c2.z * tz;
      float vx, vy, vz;
      body = slot * s.n_bodies + wit_point<LDS>(a, s_rec, tri, lx, ly, lz, vx, vy, vz);
      wx = c0.x * vx + c1.x * vy + c2.x * vz; wy = c0.y * vx + c1.y * vy + c2.y * vz; wz = c0.z * vx + c1.z * vy + c2.z * vz;
      tri += slot * a.n_tri;
    }
    obs_lane_store(a, tile, i, live, in, c_i, body);
    wit_lane_store(a, w, i, live, in, wx, wy, wz, tri);
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
  return obs_launch(k_obstacle_witness<true>, k_obstacle_witness<false>, set, a.tiles, stream, a, w);
}

int dsim_obstacle_witness_scenes(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_scenes* scenes,
                                 const int32_t* scene_id, const dsim_witness_args* args) {
  if (!scenes || !scene_id) return DSIM_E_ARG;
  const dsim_obstacles* set = scenes->proto;
  ObsK a;
  WitK w;
  const int rc = wit_args(ctx, n, state, set, args, &a, &w);
  if (rc) return rc;
  ScnK s;
  s.place = scenes->place; s.scene_id = scene_id; s.K = scenes->K; s.G = scenes->G; s.n_bodies = set->n_bodies;
  return obs_launch(k_obstacle_witness_scenes<true>, k_obstacle_witness_scenes<false>, set, a.tiles, stream, a, s, w);
}

}  // extern "C"
