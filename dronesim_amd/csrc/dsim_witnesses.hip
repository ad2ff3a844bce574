// Obstacle witnesses (dsim_obstacle_witnesses, dsim_obstacle_witnesses_scenes): the m closest BODIES of every drone within its
// margin, sorted, each with the vector to its closest point — the witness (dsim_witness.hip) answers for the one closest body of the
// whole world and drops every other minimum inside the cell walk (include/dronesim_amd.h).  Compiled as part of dsim_obstacles.hip,
// which includes it.  The tile frame is the watches' (obs_lane, obs_stage_once, obs_kargs, obs_refuse, obs_launch), the placement
// cull, the grown-box test and the per-wave reject are k_obstacle_clearance_scenes', the region decision is tri_dist2 in the walk
// and tri_closest in the tail, the velocity is wit_velocity.  What is this file's own: the walk that keeps a sorted list of
// per-body minima in registers (WitList, wits_offer, wits_cell_walk), the tail that evaluates every filled slot, the slot-major
// stores and the entry points.
#pragma once

struct WitsK {
  int* body;                     // [m][n_pad]        (the clearances [m][n_pad] are ObsK::clearance)
  float* rel;                    // [m][3][n_pad]
  int* triangle;                 // [m][n_pad] or null
  int* count;                    // [n_pad] or null
  const float4* twist;           // [K][G][2] or null (scenes only; with vel)
  float* vel;                    // [m][3][n_pad] or null
  int m, body_frame;
};

// The lane's list: M entries ascending in d2, each the least squared distance met so far to one body (key: the body, on scenes
// g n_bodies + body) and the record that attains it (idx: on scenes instance-major, g n_tri + t).  An empty entry is (inf, -1, -1).
// Every index below is a constant after unrolling: the list lives in 3 M registers, never in scratch.
template <int M>
struct WitList { float d2[M]; int key[M]; int idx[M]; };

// One triangle's (d, key, idx), offered to the list by a caller that has seen d < d2[M - 1] (nothing else can change the list: an
// entry of the same body has d2 <= the last's).  A body that is in the list updates its entry on a strict <; one that is not
// replaces the last.  The changed entry then rises past every entry it is STRICTLY below: one compare-exchange pass from the
// bottom, since only one entry fell.  Ties keep what the walk met first, between bodies and between triangles of one body.  The
// last d2 only ever falls, so a body evicted earlier may re-enter with a closer triangle: the list ends as the M least per-body
// minima.
template <int M>
__device__ __forceinline__ void wits_offer(WitList<M>& L, float d, int key, int idx) {
  bool present = false;
#pragma unroll
  for (int s = 0; s < M; ++s) present = present || L.key[s] == key;
#pragma unroll
  for (int s = 0; s < M; ++s) {
    const bool upd = (present ? L.key[s] == key : s == M - 1) && d < L.d2[s];
    L.d2[s] = upd ? d : L.d2[s];
    L.key[s] = upd ? key : L.key[s];
    L.idx[s] = upd ? idx : L.idx[s];
  }
#pragma unroll
  for (int s = M - 1; s > 0; --s) {
    const bool up = L.d2[s] < L.d2[s - 1];
    const float d_lo = L.d2[s - 1];
    const int k_lo = L.key[s - 1], i_lo = L.idx[s - 1];
    L.d2[s - 1] = up ? L.d2[s] : d_lo; L.key[s - 1] = up ? L.key[s] : k_lo; L.idx[s - 1] = up ? L.idx[s] : i_lo;
    L.d2[s] = up ? d_lo : L.d2[s]; L.key[s] = up ? k_lo : L.key[s]; L.idx[s] = up ? i_lo : L.idx[s];
  }
}

// obs_cell_walk for the list: the cell of q (the set's frame, or a placement's) and every record of its list, in list order;
// key0 / idx0 are the placement's g n_bodies / g n_tri (0 for a set).  cap2 bounds from above every d2 whose slot could be filled
// (wits_cap2): a triangle at or beyond it is never offered.  That decides speed only — such an entry would sit below every entry
// that can be filled, could displace none of them (it is not below a last entry that can be filled) and would be stored as an
// unfilled slot — and most triangles of a cell's list lie beyond the margin of most of its drones.
template <bool LDS, int M>
__device__ __forceinline__ void wits_cell_walk(const ObsK& a, const float4* s_rec, float qx, float qy, float qz, int key0, int idx0,
                                               float cap2, WitList<M>& L) {
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
    if (d2 < L.d2[M - 1] && d2 < cap2) wits_offer(L, d2, key0 + __float_as_int(r3.w), idx0 + t);
  }
}

// An upper bound of the d2 of a filled slot, sqrt(d2) - R < margin: (margin + R)^2 widened by 1e-5 relative, a hundred times the
// roundings of the sum, the square, the root and the difference.
__device__ __forceinline__ float wits_cap2(float margin, float R) {
  const float t = margin + R;
  return t * t * 1.00001f;
}

// The witnesses of a set (SCN false: `s` is not looked at) or of the placements of every drone's scene.  Frame, culling and walk
// order are the point kernels', so slot 0 is the witness: the same lanes, the same triangle, the same arithmetic.  Behind the walk
// the tail pops the list from the top, once per slot s < m (the loop is uniform; the list shifts down by constant indices): a
// filled slot — c = sqrt(d2) - R < margin, a prefix of the list — reads its record again (LDS, or one 64-byte read; on scenes
// the slot's three columns too), applies tri_closest at the point the walk looked it up with, rotates the vector back and, with
// `vel`, takes the velocity off the placement's twist.  The body-frame rotation is formed once per lane.  Stores are slot-major.
template <bool LDS, int M, bool SCN>
__global__ __launch_bounds__(256) void k_obstacle_witnesses(ObsK a, ScnK s, WitsK w) {
  extern __shared__ float4 s_rec[];
  bool staged = false;
  for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const long long i = tile * 256 + threadIdx.x;
    const bool live = i < a.n;
    ObsLane l = {};
    int sid = -1;
    if (live) { l = obs_lane(a, i); if (SCN) sid = s.scene_id[i]; }
    const float qx = l.qx, qy = l.qy, qz = l.qz, R = l.R;
    const float cap2 = wits_cap2(a.margin, R);
    WitList<M> L;
#pragma unroll
    for (int k = 0; k < M; ++k) { L.d2[k] = INFINITY; L.key[k] = -1; L.idx[k] = -1; }
    const float4* pl = s.place;
    if constexpr (SCN) {
      // the placements within reach, one bit each (k_obstacle_clearance_scenes' cull, word for word)
      unsigned near = 0u;
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
      while (near != 0u) {                 // (a wave with no such lane skips the loop: the per-wave reject)
        const int g = __ffs((int)near) - 1;
        near &= near - 1u;
        const float3 p = scn_local(pl[4 * g + 1], pl[4 * g + 2], pl[4 * g + 3], qx, qy, qz);
        if (p.x >= a.lox && p.x <= a.hix && p.y >= a.loy && p.y <= a.hiy && p.z >= a.loz && p.z <= a.hiz)
          wits_cell_walk<LDS, M>(a, s_rec, p.x, p.y, p.z, g * s.n_bodies, g * a.n_tri, cap2, L);
      }
    } else {
      // (a NaN position fails every comparison: not in the box, every slot unfilled)
      const bool inbox = live && R > 0.0f && qx >= a.lox && qx <= a.hix && qy >= a.loy && qy <= a.hiy && qz >= a.loz && qz <= a.hiz;
      obs_stage_once<LDS>(a, s_rec, staged, inbox);
      if (inbox) wits_cell_walk<LDS, M>(a, s_rec, qx, qy, qz, 0, 0, cap2, L);
    }
    // the wave's contacts, as obs_lane_store counts them: the drones whose slot 0 is filled and negative
    {
      const float c0 = DSIM_SQRT(L.d2[0]) - R;
      const unsigned long long hit = __ballot(L.key[0] >= 0 && c0 < a.margin && c0 < 0.0f);
      if (hit != 0ULL && (threadIdx.x & 63u) == 0u) {
        const unsigned long long cnt = (unsigned long long)__popcll(hit);
        atomicAdd(&a.counters[8 + DSIM_GROUND_SHARDS + DSIM_DRONE_SHARDS + (tile & (DSIM_OBST_SHARDS - 1))], cnt);
        if (a.contacts_out) atomicAdd(a.contacts_out, cnt);
      }
    }
    // R(quat)^T for the lanes that have a witness, read once (wit_lane_store's expressions)
    float r00 = 1.0f, r10 = 0.0f, r20 = 0.0f, r01 = 0.0f, r11 = 1.0f, r21 = 0.0f, r02 = 0.0f, r12 = 0.0f, r22 = 1.0f;
    if (w.body_frame && L.key[0] >= 0) {
      const float* p = a.st.base + kv_off(a.st, i);
      const long long fs = a.st.field_stride;
      const float ax = p[3 * fs], ay = p[4 * fs], az = p[5 * fs], aw = p[6 * fs];
      const float s2 = 2.0f / (ax * ax + ay * ay + az * az + aw * aw);
      const float xs = ax * s2, ys = ay * s2, zs = az * s2;
      r00 = 1.0f - (ay * ys + az * zs); r10 = ax * ys + aw * zs; r20 = ax * zs - aw * ys;
      r01 = ax * ys - aw * zs; r11 = 1.0f - (ax * xs + az * zs); r21 = ay * zs + aw * xs;
      r02 = ax * zs + aw * ys; r12 = ay * zs - aw * xs; r22 = 1.0f - (ax * xs + ay * ys);
    }
    int filled = 0;
#pragma unroll 1
    for (int sl = 0; sl < w.m; ++sl) {
      const float d2 = L.d2[0];
      const int key = L.key[0], idx = L.idx[0];
#pragma unroll
      for (int k = 0; k + 1 < M; ++k) { L.d2[k] = L.d2[k + 1]; L.key[k] = L.key[k + 1]; L.idx[k] = L.idx[k + 1]; }
      L.d2[M - 1] = INFINITY; L.key[M - 1] = -1; L.idx[M - 1] = -1;
      const float c_s = DSIM_SQRT(d2) - R;
      const bool in = key >= 0 && c_s < a.margin;
      float wx = 0.0f, wy = 0.0f, wz = 0.0f, ux = 0.0f, uy = 0.0f, uz = 0.0f;
      if (in) {
        if constexpr (SCN) {
          const int g = idx / a.n_tri;
          const float4 c0 = pl[4 * g + 1], c1 = pl[4 * g + 2], c2 = pl[4 * g + 3];
          const float3 p = scn_local(c0, c1, c2, qx, qy, qz);
          float vx, vy, vz;
          (void)wit_point<LDS>(a, s_rec, idx - g * a.n_tri, p.x, p.y, p.z, vx, vy, vz);
          wx = c0.x * vx + c1.x * vy + c2.x * vz; wy = c0.y * vx + c1.y * vy + c2.y * vz; wz = c0.z * vx + c1.z * vy + c2.z * vz;
          if (w.vel) {
            WitVelK wv;
            wv.twist = w.twist;
            wit_velocity(wv, (size_t)sid * (size_t)s.G + (size_t)g, c0, c1, c2, p, vx, vy, vz, ux, uy, uz);
          }
        } else {
          (void)wit_point<LDS>(a, s_rec, idx, qx, qy, qz, wx, wy, wz);
        }
        if (w.body_frame) {
          const float bx = r00 * wx + r10 * wy + r20 * wz, by = r01 * wx + r11 * wy + r21 * wz, bz = r02 * wx + r12 * wy + r22 * wz;
          wx = bx; wy = by; wz = bz;
          const float ex = r00 * ux + r10 * uy + r20 * uz, ey = r01 * ux + r11 * uy + r21 * uz, ez = r02 * ux + r12 * uy + r22 * uz;
          ux = ex; uy = ey; uz = ez;
        }
        ++filled;
      }
      if (live) {
        const size_t np = (size_t)a.n_pad, o1 = (size_t)sl * np + (size_t)i, o3 = (size_t)sl * 3 * np + (size_t)i;
        a.clearance[o1] = in ? c_s : a.margin;
        w.body[o1] = in ? key : -1;
        w.rel[o3] = wx; w.rel[o3 + np] = wy; w.rel[o3 + 2 * np] = wz;
        if (w.triangle) w.triangle[o1] = in ? idx : -1;
        if (w.vel) { w.vel[o3] = ux; w.vel[o3 + np] = uy; w.vel[o3 + 2 * np] = uz; }
      }
    }
    if (live && w.count) w.count[i] = filled;
  }
}

// what both queries refuse and fill alike
static int wits_args(dsim_ctx* ctx, int64_t n, const dsim_view& state, const dsim_obstacles* set, const dsim_witnesses_args* args,
                     bool scenes, ObsK* a, WitsK* w) {
  if (!args || !args->clearance_out || !args->body_out || !args->rel_out) return DSIM_E_ARG;
  if (args->m < 1 || args->m > DSIM_WITNESSES_MAX || (args->flags & ~DSIM_WITNESS_BODY_FRAME)) return DSIM_E_ARG;
  if ((args->twist == nullptr) != (args->vel_out == nullptr) || (args->twist && !scenes)) return DSIM_E_ARG;
  int rc = obs_refuse(ctx, n, state, set, args->type_id, args->margin, 0.0f, args->clearance_out);
  if (rc) return rc;
  rc = obs_kargs(ctx, n, state, set, args->offset, args->type_id, args->margin, args->clearance_out, nullptr, args->contacts_out, a);
  if (rc) return rc;
  w->body = args->body_out; w->rel = args->rel_out; w->triangle = args->triangle_out; w->count = args->count_out;
  w->twist = (const float4*)args->twist; w->vel = args->vel_out;
  w->m = args->m; w->body_frame = (args->flags & DSIM_WITNESS_BODY_FRAME) ? 1 : 0;
  if (w->body_frame) rc = make_kview(state, 7, &a->st);       // (the quaternion behind the position)
  return rc;
}

// the smallest capacity that holds m
template <bool SCN>
static int wits_launch(const dsim_obstacles* set, void* stream, const ObsK& a, const ScnK& s, const WitsK& w) {
  if (w.m <= 4) return obs_launch(k_obstacle_witnesses<true, 4, SCN>, k_obstacle_witnesses<false, 4, SCN>, set, a.tiles, stream, a, s, w);
  return obs_launch(k_obstacle_witnesses<true, 8, SCN>, k_obstacle_witnesses<false, 8, SCN>, set, a.tiles, stream, a, s, w);
}

extern "C" {

int dsim_obstacle_witnesses(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_obstacles* set,
                            const dsim_witnesses_args* args) {
  ObsK a;
  WitsK w;
  const int rc = wits_args(ctx, n, state, set, args, false, &a, &w);
  if (rc) return rc;
  return wits_launch<false>(set, stream, a, ScnK{}, w);
}

int dsim_obstacle_witnesses_scenes(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_scenes* scenes,
                                   const int32_t* scene_id, const dsim_witnesses_args* args) {
  ScnK s;
  int rc = scn_kargs(scenes, scene_id, &s);
  if (rc) return rc;
  const dsim_obstacles* set = scenes->proto;
  ObsK a;
  WitsK w;
  rc = wits_args(ctx, n, state, set, args, true, &a, &w);
  if (rc) return rc;
  return wits_launch<true>(set, stream, a, s, w);
}

}  // extern "C"
