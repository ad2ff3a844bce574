// Obstacle scenes (dsim_scenes_create, dsim_obstacle_clearance_scenes, dsim_depth_image_scenes): K scenes of up to G rigid
// placements of ONE prototype set, and a scene per drone.  Distances and ray parameters do not change under a rotation and a shift,
// so the prototype's grids, records and LDS staging serve every placement: only the query point, or the ray, goes into the
// placement's frame.  Compiled as part of dsim_obstacles.hip, which includes this file: it shares the watch's tile frame and
// cell walk (obs_lane .. obs_point_walk), its arguments and launcher (ObsK, obs_kargs, obs_refuse, obs_launch), the scenes' table
// as the kernels read it (ScnK, scn_kargs: stated there once for the watch, the witness, the camera and the scanner) and the
// camera's kernel (k_depth_image<.., PLACED>, cam_fill).  The placed point kernel here is also the placed witness's.
#pragma once

#define SCN_MAX_G 32                     // one bit per placement in a lane's mask
#define SCN_MAX_SLOTS (1LL << 22)

// A query point in a placement's frame, from the slot's three columns of R, each followed by one component of t: subtract first,
// then rotate.  R^T q - R^T t cancels digits at offsets of 128 m, R^T (q - t) does not.
__device__ __forceinline__ float3 scn_local(const float4 c0, const float4 c1, const float4 c2, float qx, float qy, float qz) {
  const float tx = qx - c0.w, ty = qy - c1.w, tz = qz - c2.w;
  const float lx = c0.x * tx + c0.y * ty + c0.z * tz, ly = c1.x * tx + c1.y * ty + c1.z * tz, lz = c2.x * tx + c2.y * ty + c2.z * tz;
  return make_float3(lx, ly, lz);
}

// k_obstacle_clearance with the set placed, in the same tile frame (dsim_obstacles.hip).  Scene ids differ per lane, so
// placement records are per-lane vector loads: a lane reads the first 16 bytes of each of its scene's G slots, (c_task, r_cull), and the other 48 only of a slot whose sphere it is within reach of — the bound
// is widened (1e-4 relative, 1e-5 m) well beyond the fp32 rounding of q - c and of an R that is orthonormal to 1e-5, so it decides
// speed only.  Then q goes into the placement's frame (scn_local).  There the grown-box test and the cell walk are the unplaced
// kernel's.  The minimum runs over the placements in slot order with a strict <, and the body is g * n_bodies + the triangle's.
// Instantiated with Wit = WitK it is the witness, as k_obstacle_clearance is (dsim_witness.hip): the loop keeps the winner's slot
// and record index; behind it the winner's three columns are read again (the lane read them in the loop: they come from cache), q
// goes into that placement's frame by the loop's own scn_local, tri_closest gives the local vector and R takes it back:
// rel = sum_k col_k l_k.  The triangle is instance-major, g n_tri + t, as the body is g n_bodies + body.
// Instantiated with Wit = WitVelK it is the witness with a velocity (dsim_obstacle_witness_scenes_vel, dsim_witness.hip): the same
// tail, and from the local point and the local vector it already holds the velocity of the witness as a point of the winner's
// placement (wit_velocity: the placement's twist, read once, behind the walk, by the lanes that have a witness).
struct WitVelK;
template <bool LDS, class... Wit>
__global__ __launch_bounds__(256) void k_obstacle_clearance_scenes(ObsK a, ScnK s, Wit... w) {
  constexpr bool WIT = sizeof...(Wit) != 0, VEL = (std::is_same<Wit, WitVelK>::value || ...);
  extern __shared__ float4 s_rec[];
  bool staged = false;
  for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const long long i = tile * 256 + threadIdx.x;
    const bool live = i < a.n;
    ObsLane l = {};
    int sid = -1;
    if (live) { l = obs_lane(a, i); sid = s.scene_id[i]; }
    const float qx = l.qx, qy = l.qy, qz = l.qz, R = l.R;
    // the placements within reach, one bit each (a NaN position fails every comparison; a scene outside [0, K) has none)
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
    int win = -1, slot = 0;                // the winner's body, g * n_bodies + the triangle's; with WIT its record index and its slot
    while (near != 0u) {                   // (a wave with no such lane skips the loop: the per-wave reject)
      const int g = __ffs((int)near) - 1;
      near &= near - 1u;
      const float3 p = scn_local(pl[4 * g + 1], pl[4 * g + 2], pl[4 * g + 3], qx, qy, qz);
      // (the grown box of the prototype, in its own frame: outside it no triangle is within reach)
      if (p.x >= a.lox && p.x <= a.hix && p.y >= a.loy && p.y <= a.hiy && p.z >= a.loz && p.z <= a.hiz) {
        float b2 = best;
        int w2 = -1;
        obs_point_walk<LDS, WIT>(a, s_rec, p.x, p.y, p.z, w2, b2);
        if (w2 >= 0) { best = b2; win = WIT ? w2 : g * s.n_bodies + w2; slot = g; }
      }
    }
    const float c_i = DSIM_SQRT(best) - R;
    const bool in = win >= 0 && c_i < a.margin;
    if constexpr (WIT) {
      float wx = 0.0f, wy = 0.0f, wz = 0.0f, ux = 0.0f, uy = 0.0f, uz = 0.0f;
      int body = -1;
      if (in) {
        const float4 c0 = pl[4 * slot + 1], c1 = pl[4 * slot + 2], c2 = pl[4 * slot + 3];
        const float3 p = scn_local(c0, c1, c2, qx, qy, qz);
        float vx, vy, vz;
        body = slot * s.n_bodies + wit_point<LDS>(a, s_rec, win, p.x, p.y, p.z, vx, vy, vz);
        wx = c0.x * vx + c1.x * vy + c2.x * vz; wy = c0.y * vx + c1.y * vy + c2.y * vz; wz = c0.z * vx + c1.z * vy + c2.z * vz;
        win += slot * a.n_tri;
        if constexpr (VEL) wit_velocity(w..., (size_t)sid * (size_t)s.G + (size_t)slot, c0, c1, c2, p, vx, vy, vz, ux, uy, uz);
      }
      obs_lane_store(a, tile, i, live, in, c_i, body);
      if constexpr (VEL) wit_lane_store(a, w..., i, live, in, wx, wy, wz, win, ux, uy, uz);
      else wit_lane_store(a, w..., i, live, in, wx, wy, wz, win);
    } else {
      obs_lane_store(a, tile, i, live, in, c_i, win);
    }
  }
}

extern "C" {

int dsim_scenes_create(dsim_ctx* ctx, const dsim_obstacles* proto, const float* place_host, const int32_t* count_host, int64_t K,
                       int32_t G, dsim_scenes** out) {
  if (!ctx || !proto || !place_host || !out || K < 1 || G < 1 || G > SCN_MAX_G || K > SCN_MAX_SLOTS / G) return DSIM_E_ARG;
  // the prototype's own box: its centre and half its diagonal
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (size_t k = 0; k < proto->tri_host.size(); ++k) {
    lo[k % 3] = fmin(lo[k % 3], (double)proto->tri_host[k]); hi[k % 3] = fmax(hi[k % 3], (double)proto->tri_host[k]);
  }
  double c[3], hd = 0.0, cn = 0.0;
  for (int k = 0; k < 3; ++k) { c[k] = 0.5 * (lo[k] + hi[k]); hd += 0.25 * (hi[k] - lo[k]) * (hi[k] - lo[k]); cn += c[k] * c[k]; }
  hd = sqrt(hd); cn = sqrt(cn);
  std::vector<float> rec;
  try { rec.assign((size_t)K * G * 16, 0.0f); } catch (const std::bad_alloc&) { return (int)hipErrorOutOfMemory; }
  for (int64_t s = 0; s < K; ++s) {
    const int cnt = count_host ? count_host[s] : G;
    if (cnt < 0 || cnt > G) return DSIM_E_ARG;
    for (int g = 0; g < G; ++g) {
      float* r = rec.data() + ((size_t)s * G + g) * 16;
      if (g >= cnt) { r[3] = -INFINITY; continue; }            // (the host's entry is not looked at)
      const float* p = place_host + ((size_t)s * G + g) * 12;  // R row-major, then t
      for (int k = 0; k < 12; ++k) if (!isfinite(p[k])) return DSIM_E_ARG;
      for (int i = 0; i < 3; ++i)                              // R^T R = I to 1e-5
        for (int j = 0; j < 3; ++j) {
          const double d = (double)p[i] * p[j] + (double)p[3 + i] * p[3 + j] + (double)p[6 + i] * p[6 + j];
          if (!(fabs(d - (i == j ? 1.0 : 0.0)) <= 1e-5)) return DSIM_E_ARG;
        }
      const double det = (double)p[0] * ((double)p[4] * p[8] - (double)p[5] * p[7]) - (double)p[1] * ((double)p[3] * p[8] - (double)p[5] * p[6]) +
                         (double)p[2] * ((double)p[3] * p[7] - (double)p[4] * p[6]);
      if (!(det > 0.0)) return DSIM_E_ARG;
      for (int i = 0; i < 3; ++i) r[i] = (float)((double)p[3 * i] * c[0] + (double)p[3 * i + 1] * c[1] + (double)p[3 * i + 2] * c[2] + (double)p[9 + i]);
      // half the diagonal, and what an R that is orthonormal to 1e-5 only can move the box's centre by; rounded up
      r[3] = nextafterf((float)(hd * (1.0 + 1e-4) + 4e-5 * cn + 1e-5), INFINITY);
      for (int col = 0; col < 3; ++col) {                      // column `col` of R, then t[col]
        r[4 + 4 * col] = p[col]; r[5 + 4 * col] = p[3 + col]; r[6 + 4 * col] = p[6 + col]; r[7 + 4 * col] = p[9 + col];
      }
      if (!isfinite(r[0]) || !isfinite(r[1]) || !isfinite(r[2])) return DSIM_E_ARG;
    }
  }
  dsim_scenes* sc = new (std::nothrow) dsim_scenes();
  if (!sc) return (int)hipErrorOutOfMemory;
  sc->proto = proto; sc->place = nullptr; sc->K = K; sc->G = G;
  for (int k = 0; k < 3; ++k) sc->box_c[k] = (float)c[k];
  hipError_t e = hipSetDevice(ctx->device);
  if (e == hipSuccess) e = hipMalloc((void**)&sc->place, rec.size() * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(sc->place, rec.data(), rec.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) { (void)dsim_scenes_destroy(ctx, sc); return (int)e; }
  *out = sc;
  return DSIM_OK;
}

int dsim_scenes_destroy(dsim_ctx* ctx, dsim_scenes* scenes) {
  (void)ctx;                                          // (may be NULL, as for dsim_obstacles_destroy)
  if (!scenes) return DSIM_OK;
  hipError_t e = hipSuccess;                          // (hipFree waits for the work that may still read the table)
  if (scenes->place) e = hipFree(scenes->place);
  for (float4* p : {scenes->motion, scenes->base})    // (dsim_scenes_motion_set's buffers)
    if (p) { const hipError_t f = hipFree(p); if (e == hipSuccess) e = f; }
  delete scenes;
  return (int)e;
}

int dsim_obstacle_clearance_scenes(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_scenes* scenes,
                                   const int32_t* scene_id, const float* offset, const uint8_t* type_id, float margin,
                                   float* clearance_out, int32_t* nearest_out, uint64_t* contacts_out) {
  ScnK s;
  int rc = scn_kargs(scenes, scene_id, &s);
  if (rc) return rc;
  const dsim_obstacles* set = scenes->proto;
  rc = obs_refuse(ctx, n, state, set, type_id, margin, 0.0f, clearance_out);
  if (rc) return rc;
  ObsK a;
  rc = obs_kargs(ctx, n, state, set, offset, type_id, margin, clearance_out, nearest_out, contacts_out, &a);
  if (rc) return rc;
  return obs_launch(k_obstacle_clearance_scenes<true>, k_obstacle_clearance_scenes<false>, set, a.tiles, stream, a, s);
}

int dsim_depth_image_scenes(dsim_ctx* ctx, void* stream, dsim_view state, const dsim_scenes* scenes, const int32_t* scene_id,
                            const dsim_camera_params* params, int64_t n_cam, const int32_t* cam_index, const float* offset,
                            const uint8_t* type_id, float* depth_out, int32_t* seg_out) {
  ScnK pl;
  int rc = scn_kargs(scenes, scene_id, &pl);
  if (rc) return rc;
  const dsim_obstacles* set = scenes->proto;
  CamK a;
  int64_t blocks;
  rc = cam_fill(ctx, state, set, params, n_cam, cam_index, offset, type_id, depth_out, seg_out, &a, &blocks);
  if (rc) return rc;
  a.pl = pl;
  const hipStream_t st_ = (hipStream_t)stream;
  const bool lds = set->n_tri <= OBS_LDS_TRI;
  const size_t shm = lds ? (size_t)set->n_tri * 64 : 0;
  const dim3 gr((unsigned)blocks), tb(256);
  if (lds && seg_out) hipLaunchKernelGGL((k_depth_image<true, true, false, true, true>), gr, tb, shm, st_, a);
  else if (lds) hipLaunchKernelGGL((k_depth_image<true, false, false, true, true>), gr, tb, shm, st_, a);
  else if (seg_out) hipLaunchKernelGGL((k_depth_image<false, true, false, true, true>), gr, tb, 0, st_, a);
  else hipLaunchKernelGGL((k_depth_image<false, false, false, true, true>), gr, tb, 0, st_, a);
  return (int)hipGetLastError();
}

}  // extern "C"
