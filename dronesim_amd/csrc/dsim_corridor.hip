// Corridor clearance (dsim_corridor_clearance): per drone and slot, the clearance of the vehicle's bounding sphere swept along the
// candidate segment e -> e + rel[t][:][i] against the world the watches see: the set's triangles, or the placements of the
// drone's scene where they stand now, and the half-space z <= 0 (include/dronesim_amd.h has the segment and the outputs).  A
// query, not a watch: no history, no counters of the context.  Compiled as part of dsim_obstacles.hip, which includes this file:
// the arithmetic is the swept watch's (seg_tri_dist2, pieces looked up by their midpoints, dsim_sweep.hip), the tile frame and the
// launcher are the watches' (ObsK, obs_kargs, obs_refuse, obs_stage_once, obs_cell_walk, obs_launch), the placed world is the
// scenes' (ScnK, scn_kargs, scn_local: both ends of the segment go into the placement's frame, the subtraction first), and the
// mapping is line of sight's: one drone per lane, the lane loops over the slots, chunks of the slots spread over blockIdx.y when
// the fleet is small (scan_beams_per_block).
#pragma once

struct CorK {
  ObsK o;                          // the fleet, the set's records and grid, the margin; rec == null: no triangles (the ground alone)
  ScnK pl;                         // PLACED instances
  float sag;
  float inv_piece;                 // 1 / (2 half (1 - 2^-10)), as the swept watch's; 0 without triangles: every segment is one piece
  unsigned flags;
  const float* rel;                // [k][3][n_pad]
  const int* index;                // [k][n_pad] or null
  int k;
  int slots_per_block;             // blockIdx.y takes the slots [y, y + 1) * slots_per_block
  float* clearance;                // [k][n_pad]
  int* body;                       // same shape, or null
  unsigned long long* unserved_out;
};

// The pieces of one segment l0 -> l0 + d (l1 its far end as the caller formed it) against the set in the frame the segment is
// given in: the swept watch's rule.  K equal pieces, each looked up in the cell of its own midpoint; a piece whose midpoint lies
// outside the grown box reads no list.  Piece ends are formed from p and inv_k each time: nothing per piece is kept.
template <bool LDS>
__device__ __forceinline__ void cor_pieces(const ObsK& a, const float4* s_rec, float l0x, float l0y, float l0z, float l1x, float l1y,
                                           float l1z, int K, float inv_k, int& body, float& best) {
  const float dx = l1x - l0x, dy = l1y - l0y, dz = l1z - l0z;
  for (int p = 0; p < K; ++p) {
    const float t0 = (float)p * inv_k, tm = ((float)p + 0.5f) * inv_k, t1 = (float)(p + 1) * inv_k;
    const bool last = p + 1 == K;
    const float mx = l0x + dx * tm, my = l0y + dy * tm, mz = l0z + dz * tm;
    if (mx >= a.lox && mx <= a.hix && my >= a.loy && my <= a.hiy && mz >= a.loz && mz <= a.hiz) {
      const float ax = l0x + dx * t0, ay = l0y + dy * t0, az = l0z + dz * t0;
      const float bx = last ? l1x : l0x + dx * t1, by = last ? l1y : l0y + dy * t1, bz = last ? l1z : l0z + dz * t1;
      obs_cell_walk<LDS>(a, s_rec, mx, my, mz,
                         [=](const float4 r0, const float4 r1, const float4 r2, const float4 r3) {
                           return seg_tri_dist2(r0, r1, r2, r3, ax, ay, az, bx, by, bz, tri_dist2(r0, r1, r2, r3, ax, ay, az));
                         },
                         body, best);
    }
  }
}

// One drone per lane, tiles of 256 grid-stride, the slots of the workgroup's chunk in a loop.  Per slot a lane decides whether
// the slot is evaluated (index, finite e and d), whether it is served (K <= 32), what of the world its segment can touch — the
// segment's bounding box against the grown box, or per placement the distance from c_task to the segment against the cull radius,
// widened: both decide speed only — and takes the minimum over the ground, then the placements in slot order, then the lists in
// their order, with a strict <.  No lane leaves early: the workgroup meets at the staging barrier, which stands in the slot loop
// (the chunk's bounds are uniform over the workgroup) and is passed once the records are staged.
template <bool LDS, bool PLACED>
__global__ __launch_bounds__(256) void k_corridor_clearance(CorK w) {
  const ObsK& a = w.o;
  extern __shared__ float4 s_rec[];
  const bool ground = (w.flags & DSIM_CORRIDOR_GROUND) != 0u;
  const bool tris = a.rec != nullptr;
  const int t_lo = (int)blockIdx.y * w.slots_per_block, t_hi = min(t_lo + w.slots_per_block, w.k);
  bool staged = false;
  for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const long long i = tile * 256 + threadIdx.x;
    const bool lane = i < a.n;
    ObsLane l = {};
    int sid = -1;
    if (lane) {
      l = obs_lane(a, i);
      if (PLACED) sid = w.pl.scene_id[i];
    }
    const float ex = l.qx, ey = l.qy, ez = l.qz, Rs = l.R + w.sag;
    // (a NaN fails the comparison: |x| <= FLT_MAX holds for finite x only)
    const bool defined = lane && fabsf(ex) <= 3.0e38f && fabsf(ey) <= 3.0e38f && fabsf(ez) <= 3.0e38f;
    const float4* pl = w.pl.place;
    const bool scene = PLACED && sid >= 0 && (long long)sid < w.pl.K;
    if (scene) pl += 4 * ((size_t)sid * (size_t)w.pl.G);
    int n_unserved = 0;
    for (int t = t_lo; t < t_hi; ++t) {
      float dx = 0.0f, dy = 0.0f, dz = 0.0f;
      bool used = false;
      if (lane) {
        const float* r = w.rel + (size_t)t * 3u * (size_t)a.n_pad + (size_t)i;
        dx = r[0]; dy = r[a.n_pad]; dz = r[2 * a.n_pad];
        used = !w.index || w.index[(size_t)t * (size_t)a.n_pad + (size_t)i] >= 0;
      }
      const bool valid = defined && used && fabsf(dx) <= 3.0e38f && fabsf(dy) <= 3.0e38f && fabsf(dz) <= 3.0e38f;
      const float len = DSIM_SQRT(dx * dx + dy * dy + dz * dz);
      const float kf = ceilf(len * w.inv_piece);
      const bool served = valid && kf <= SWEEP_MAX_PIECES;       // (a length that overflows float32 fails the comparison: unserved)
      n_unserved += (valid && !served) ? 1 : 0;
      const int K = served ? max((int)kf, 1) : 1;                // (a segment of length 0 is one piece: the point query)
      const float inv_k = DSIM_RCP((float)K);
      const float fx = ex + dx, fy = ey + dy, fz = ez + dz;      // the far end
      float best = INFINITY;
      int body = -1;
      if (ground && served) {                                    // the half-space z <= 0: analytic, also away from every box
        const float gz = fmaxf(fminf(ez, fz), 0.0f);
        best = gz * gz; body = DSIM_SEG_GROUND;
      }
      if (!PLACED) {
        const bool near_box = served && tris && fminf(ex, fx) <= a.hix && fmaxf(ex, fx) >= a.lox && fminf(ey, fy) <= a.hiy &&
                              fmaxf(ey, fy) >= a.loy && fminf(ez, fz) <= a.hiz && fmaxf(ez, fz) >= a.loz;
        obs_stage_once<LDS>(a, s_rec, staged, near_box);
        if (near_box) cor_pieces<LDS>(a, s_rec, ex, ey, ez, fx, fy, fz, K, inv_k, body, best);   // (a wave with no such lane skips it)
      } else {
        // the placements whose cull sphere the segment comes within Rs + margin of, one bit each
        unsigned near = 0u;
        if (served && scene) {
          const float dd = dx * dx + dy * dy + dz * dz;
          const float inv_dd = dd > 0.0f ? DSIM_RCP(dd) : 0.0f;
          for (int g = 0; g < w.pl.G; ++g) {
            const float4 c = pl[4 * g];                          // (c_task, r_cull); r_cull = -inf for a slot at or above the count
            const float mx = c.x - ex, my = c.y - ey, mz = c.z - ez;
            const float tc = fminf(fmaxf((mx * dx + my * dy + mz * dz) * inv_dd, 0.0f), 1.0f);
            const float ux = mx - tc * dx, uy = my - tc * dy, uz = mz - tc * dz;
            // (the point kernel's widening, and the rounding of tc d, which grows with the segment and with the distance)
            const float b = (c.w + Rs + a.margin) * 1.0001f + 1e-5f + 1e-5f * (fabsf(mx) + fabsf(my) + fabsf(mz) + len);
            near |= (b >= 0.0f && ux * ux + uy * uy + uz * uz <= b * b) ? (1u << g) : 0u;
          }
        }
        obs_stage_once<LDS>(a, s_rec, staged, near != 0u);
        while (near != 0u) {                                     // (a wave with no such lane skips the loop)
          const int g = __ffs((int)near) - 1;
          near &= near - 1u;
          const float4 c0 = pl[4 * g + 1], c1 = pl[4 * g + 2], c2 = pl[4 * g + 3];
          const float3 p0 = scn_local(c0, c1, c2, ex, ey, ez), p1 = scn_local(c0, c1, c2, fx, fy, fz);
          float b2 = best;
          int w2 = -1;
          cor_pieces<LDS>(a, s_rec, p0.x, p0.y, p0.z, p1.x, p1.y, p1.z, K, inv_k, w2, b2);
          if (w2 >= 0) { best = b2; body = g * w.pl.n_bodies + w2; }
        }
      }
      if (lane) {
        const float c = DSIM_SQRT(best) - Rs;
        const bool in = c < a.margin;
        const size_t out = (size_t)t * (size_t)a.n_pad + (size_t)i;
        w.clearance[out] = served ? (in ? c : a.margin) : -INFINITY;
        if (w.body) w.body[out] = (served && in) ? body : -1;
      }
    }
    // the tile's unserved slots: one ballot, and one atomic of the wave's sum where it has any
    if (__ballot(n_unserved != 0) != 0ULL) {
      for (int s = 32; s > 0; s >>= 1) n_unserved += __shfl_xor(n_unserved, s, 64);
      if ((threadIdx.x & 63u) == 0u && w.unserved_out) atomicAdd(w.unserved_out, (unsigned long long)n_unserved);
    }
  }
}

extern "C" int dsim_corridor_clearance(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_obstacles* set,
                                       const dsim_corridor_args* args) {
  if (!ctx || !args || !args->rel || !args->clearance_out || n <= 0 || n > state.n_pad) return DSIM_E_ARG;
  const dsim_corridor_args& s = *args;
  if (s.k < 1 || s.k > 32) return DSIM_E_ARG;
  if ((s.flags & ~(uint32_t)DSIM_CORRIDOR_GROUND) != 0u) return DSIM_E_ARG;
  if (!isfinite(s.margin) || !(s.margin > 0.0f) || !isfinite(s.sag) || !(s.sag >= 0.0f)) return DSIM_E_ARG;
  if (ctx->n_types > 1 && !s.type_id) return DSIM_E_ARG;
  if ((s.scenes != nullptr) != (s.scene_id != nullptr) || (s.scenes && set)) return DSIM_E_ARG;
  const dsim_obstacles* tris = s.scenes ? s.scenes->proto : set;
  if (!tris && !(s.flags & DSIM_CORRIDOR_GROUND)) return DSIM_E_ARG;
  CorK w;
  memset(&w, 0, sizeof(w));
  int rc;
  if (tris) {
    if ((rc = obs_refuse(ctx, n, state, tris, s.type_id, s.margin, s.sag, s.clearance_out)) != 0) return rc;
    // the swept watch's pieces: a piece reaches `half` from its midpoint at most, taken 2^-10 shorter when K is chosen
    const double reach = (double)tris->grid.reach;
    const double half = reach - ((double)ctx_r_max(ctx) + (double)s.sag + (double)s.margin);
    if (!(half >= reach / 1024.0)) return DSIM_E_ARG;
    w.inv_piece = (float)(1.0 / (2.0 * half * (1.0 - 1.0 / 1024.0)));
    if ((rc = obs_kargs(ctx, n, state, tris, s.offset, s.type_id, s.margin, s.clearance_out, nullptr, nullptr, &w.o)) != 0) return rc;
    w.o.clearance = nullptr;                         // (the watches' [n_pad] outputs: this kernel has its own, slot-major)
  } else {                                           // the ground alone: the fleet and the margin, no records, one piece
    if ((rc = make_kview(state, 3, &w.o.st)) != 0) return rc;
    w.o.n = n; w.o.n_pad = state.n_pad; w.o.tiles = (n + 255) / 256;
    w.o.offset = s.offset; w.o.type_id = s.type_id; w.o.types = ctx->d_types; w.o.n_types = ctx->n_types;
    w.o.margin = s.margin;
  }
  if (s.scenes && (rc = scn_kargs(s.scenes, s.scene_id, &w.pl)) != 0) return rc;
  w.sag = s.sag; w.flags = s.flags; w.rel = s.rel; w.index = s.index; w.k = s.k;
  w.clearance = s.clearance_out; w.body = s.body_out; w.unserved_out = (unsigned long long*)s.unserved_out;
  w.slots_per_block = scan_beams_per_block(w.o.tiles, w.k);
  const dim3 gr(obs_blocks(w.o.tiles), (unsigned)((w.k + w.slots_per_block - 1) / w.slots_per_block)), tb(256);
  const hipStream_t st_ = (hipStream_t)stream;
  const bool lds = tris && tris->n_tri <= OBS_LDS_TRI;
  const size_t shm = lds ? (size_t)tris->n_tri * 64 : 0;
  if (s.scenes) {
    if (lds) hipLaunchKernelGGL((k_corridor_clearance<true, true>), gr, tb, shm, st_, w);
    else hipLaunchKernelGGL((k_corridor_clearance<false, true>), gr, tb, 0, st_, w);
  } else {
    if (lds) hipLaunchKernelGGL((k_corridor_clearance<true, false>), gr, tb, shm, st_, w);
    else hipLaunchKernelGGL((k_corridor_clearance<false, false>), gr, tb, 0, st_, w);      // (and the ground alone: no records at all)
  }
  return (int)hipGetLastError();
}
