// Swept static-obstacle watch (dsim_obstacle_sweep): per-drone clearance between the vehicle's bounding sphere, swept along the chord
// from the position the previous call saw to the current one, and the set's triangles (include/dronesim_amd.h).  Compiled as part
// of dsim_obstacles.hip, which includes it: it shares the set's private record, tri_dist2, the watches' tile frame and their launcher.

struct SweepK {
  ObsK o;                        // as the point watch's; contacts are counted on its shards (DSIM_Q_OBSTACLE_CONTACTS)
  float sag;
  float inv_piece;               // 1 / (2 half (1 - 2^-10)): pieces per metre of chord, rounded up on the safe side
  float* prev;                   // SoA [3][n_pad], world frame
  int keep_prev;
  unsigned long long* unswept_out;
};

#define SWEEP_MAX_PIECES 32.0f   // a chord that needs more is a teleport: sampled at its end

// Squared distance between the piece P + s u (s in [0, 1], uu = u.u, possibly 0) and the edge E + t d (t in [0, 1], dd = d.d > 0):
// Ericson, Real-Time Collision Detection 5.1.9, with selects.  s of the two infinite lines where they are not parallel (else 0),
// t of the edge closest to that point, clamped; s again for a clamped t.  Whatever rounding does to s and t, the result is the
// distance between a point of the piece and a point of the edge, so never below the true minimum by more than rounding.
__device__ __forceinline__ float seg_seg_dist2(float px, float py, float pz, float ux, float uy, float uz, float uu, float ex, float ey,
                                               float ez, float dx, float dy, float dz, float dd) {
  const float rx = px - ex, ry = py - ey, rz = pz - ez;
  const float b = ux * dx + uy * dy + uz * dz, c = ux * rx + uy * ry + uz * rz, f = dx * rx + dy * ry + dz * rz;
  const float ae = uu * dd, den = ae - b * b;
  const float inv_uu = uu > 0.0f ? DSIM_RCP(uu) : 0.0f;         // (a zero-length piece: s = 0 throughout)
  float s = den > 1e-6f * ae ? fminf(fmaxf((b * f - c * dd) * DSIM_RCP(den), 0.0f), 1.0f) : 0.0f;   // (parallel within 1e-3 rad: s = 0)
  float t = (b * s + f) * DSIM_RCP(dd);
  s = t < 0.0f ? fminf(fmaxf(-c * inv_uu, 0.0f), 1.0f) : (t > 1.0f ? fminf(fmaxf((b - c) * inv_uu, 0.0f), 1.0f) : s);
  t = fminf(fmaxf(t, 0.0f), 1.0f);
  const float wx = rx + s * ux - t * dx, wy = ry + s * uy - t * dy, wz = rz + s * uz - t * dz;
  return wx * wx + wy * wy + wz * wz;
}

// Squared distance between the piece A -> B and one triangle record: the least of the point distances at both ends, the three
// piece-edge distances, and 0 where the piece pierces the face (Moeller-Trumbore on a, ab, ac, decided on signs: no quotient).
// A piece that lies in the triangle's plane has det = 0 and is not "piercing": it meets an edge or has an end in the face.
__device__ __forceinline__ float seg_tri_dist2(const float4 r0, const float4 r1, const float4 r2, const float4 r3, float ax_, float ay_,
                                               float az_, float bx_, float by_, float bz_, float d_a) {
  const float ax = r0.x, ay = r0.y, az = r0.z, abx = r0.w, aby = r1.x, abz = r1.y, acx = r1.z, acy = r1.w, acz = r2.x;
  const float e00 = r3.x, e01 = r3.y, e11 = r3.z;
  const float ux = bx_ - ax_, uy = by_ - ay_, uz = bz_ - az_, uu = ux * ux + uy * uy + uz * uz;
  float best = fminf(d_a, tri_dist2(r0, r1, r2, r3, bx_, by_, bz_));
  best = fminf(best, seg_seg_dist2(ax_, ay_, az_, ux, uy, uz, uu, ax, ay, az, abx, aby, abz, e00));
  best = fminf(best, seg_seg_dist2(ax_, ay_, az_, ux, uy, uz, uu, ax, ay, az, acx, acy, acz, e11));
  best = fminf(best, seg_seg_dist2(ax_, ay_, az_, ux, uy, uz, uu, ax + abx, ay + aby, az + abz, acx - abx, acy - aby, acz - abz,
                                   fmaxf(e00 - 2.0f * e01 + e11, 1e-30f)));
  const float pvx = uy * acz - uz * acy, pvy = uz * acx - ux * acz, pvz = ux * acy - uy * acx;
  const float det = abx * pvx + aby * pvy + abz * pvz;
  const float sg = det < 0.0f ? -1.0f : 1.0f, adet = fabsf(det);
  const float tx = ax_ - ax, ty = ay_ - ay, tz = az_ - az;
  const float bu = sg * (tx * pvx + ty * pvy + tz * pvz);
  const float qx = ty * abz - tz * aby, qy = tz * abx - tx * abz, qz = tx * aby - ty * abx;
  const float bv = sg * (ux * qx + uy * qy + uz * qz);
  const float bt = sg * (acx * qx + acy * qy + acz * qz);
  const bool pierce = adet > 0.0f && bu >= 0.0f && bv >= 0.0f && bu + bv <= adet && bt >= 0.0f && bt <= adet;
  return pierce ? 0.0f : best;
}

// prev := the current position of every live lane, and nothing else (DSIM_SWEEP_PRIME)
__global__ __launch_bounds__(256) void k_sweep_prime(SweepK w) {
  const ObsK& a = w.o;
  for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const long long i = tile * 256 + threadIdx.x;
    if (i < a.n) {
      const long long o = kv_off(a.st, i);
      w.prev[i] = a.st.base[o];
      w.prev[a.n_pad + i] = a.st.base[o + a.st.field_stride];
      w.prev[2 * a.n_pad + i] = a.st.base[o + 2 * a.st.field_stride];
    }
  }
}

// The swept watch, in the tile frame of dsim_obstacles.hip (obs_stage_once, obs_cell_walk, obs_lane_store).  A lane's chord q0 -> q1
// is cut into K equal pieces no longer than 2 half; each piece is looked up in the cell of its own midpoint, and a piece whose midpoint lies outside the grown box reads no list — a wave none
// of whose lanes has such a piece skips the walk (the per-wave reject).  The workgroup stages the records when a chord's
// bounding box meets the grown box (a superset of "some midpoint inside": staging more often costs time, never results).
// An unswept lane (K > 32, or a non-finite prev or position) is the point q1: its chord collapses to q1 and only tri_dist2 at
// that point counts, which makes it the point watch's arithmetic bit for bit.
template <bool LDS>
__global__ __launch_bounds__(256) void k_obstacle_sweep(SweepK w) {
  const ObsK& a = w.o;
  extern __shared__ float4 s_rec[];
  bool staged = false;
  for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const long long i = tile * 256 + threadIdx.x;
    const bool live = i < a.n;
    // The lane's own load, not obs_lane: prev is read, and written, between the position and the offset, and the far case's time
    // follows the order of these loads (measured: profiles/r13_obstacle_watches_refactor.txt).
    float q1x = 0.0f, q1y = 0.0f, q1z = 0.0f, q0x = 0.0f, q0y = 0.0f, q0z = 0.0f, R = 0.0f;
    if (live) {
      const long long o = kv_off(a.st, i);
      const float px = a.st.base[o], py = a.st.base[o + a.st.field_stride], pz = a.st.base[o + 2 * a.st.field_stride];
      q0x = w.prev[i]; q0y = w.prev[a.n_pad + i]; q0z = w.prev[2 * a.n_pad + i];
      if (!w.keep_prev) { w.prev[i] = px; w.prev[a.n_pad + i] = py; w.prev[2 * a.n_pad + i] = pz; }
      q1x = px; q1y = py; q1z = pz;
      if (a.offset) {
        const float fx = a.offset[i], fy = a.offset[a.n_pad + i], fz = a.offset[2 * a.n_pad + i];
        q1x -= fx; q1y -= fy; q1z -= fz; q0x -= fx; q0y -= fy; q0z -= fz;
      }
      R = a.types[a.type_id ? min((int)a.type_id[i], a.n_types - 1) : 0].coll_sphere;
    }
    const bool part = live && R > 0.0f;                  // (a type with R = 0 takes no part, whatever the sag)
    const float Rs = R + w.sag;
    float dx = q1x - q0x, dy = q1y - q0y, dz = q1z - q0z;
    const float kf = ceilf(DSIM_SQRT(dx * dx + dy * dy + dz * dz) * w.inv_piece);
    const bool swept = kf <= SWEEP_MAX_PIECES;           // (NaN or infinity in prev or in the position fails the comparison)
    if (!swept) { q0x = q1x; q0y = q1y; q0z = q1z; dx = 0.0f; dy = 0.0f; dz = 0.0f; }
    const int K = swept ? max((int)kf, 1) : 1;           // (a chord of length 0 is one piece)
    const float inv_k = DSIM_RCP((float)K);
    // (a NaN position fails every comparison: no staging for it, no piece in the box, clearance = margin)
    const bool near_box = part && fminf(q0x, q1x) <= a.hix && fmaxf(q0x, q1x) >= a.lox && fminf(q0y, q1y) <= a.hiy &&
                          fmaxf(q0y, q1y) >= a.loy && fminf(q0z, q1z) <= a.hiz && fmaxf(q0z, q1z) >= a.loz;
    obs_stage_once<LDS>(a, s_rec, staged, near_box);
    float best = INFINITY;
    int body = -1;
    bool inbox = false;
    for (int p = 0; p < (near_box ? K : 0); ++p) {
      const float t0 = (float)p * inv_k, tm = ((float)p + 0.5f) * inv_k;
      const bool last = p + 1 == K;
      const float t1 = (float)(p + 1) * inv_k;
      const float mx = q0x + dx * tm, my = q0y + dy * tm, mz = q0z + dz * tm;
      if (mx >= a.lox && mx <= a.hix && my >= a.loy && my <= a.hiy && mz >= a.loz && mz <= a.hiz) {
        inbox = true;
        const float ax = q0x + dx * t0, ay = q0y + dy * t0, az = q0z + dz * t0;
        const float bx = last ? q1x : q0x + dx * t1, by = last ? q1y : q0y + dy * t1, bz = last ? q1z : q0z + dz * t1;
        // the list of the midpoint's cell; per triangle the piece's distance, or the point A's for an unswept lane
        obs_cell_walk<LDS>(a, s_rec, mx, my, mz,
                           [=](const float4 r0, const float4 r1, const float4 r2, const float4 r3) {
                             const float d_a = tri_dist2(r0, r1, r2, r3, ax, ay, az);
                             const float d_s = seg_tri_dist2(r0, r1, r2, r3, ax, ay, az, bx, by, bz, d_a);
                             return swept ? d_s : d_a;
                           },
                           body, best);
      }
    }
    const float c_i = DSIM_SQRT(best) - Rs;
    obs_lane_store(a, tile, i, live, inbox && c_i < a.margin, c_i, body);
    const unsigned long long pts = __ballot(part && !swept);
    if (pts != 0ULL && (threadIdx.x & 63u) == 0u && w.unswept_out) atomicAdd(w.unswept_out, (unsigned long long)__popcll(pts));
  }
}

extern "C" int dsim_obstacle_sweep(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_obstacles* set,
                                   const dsim_sweep_args* args) {
  if (!ctx || !set || !args || !args->prev || n <= 0 || n > state.n_pad) return DSIM_E_ARG;
  const int32_t fl = args->flags;
  if ((fl & ~(DSIM_SWEEP_KEEP_PREV | DSIM_SWEEP_PRIME)) || fl == (DSIM_SWEEP_KEEP_PREV | DSIM_SWEEP_PRIME)) return DSIM_E_ARG;
  const bool prime = (fl & DSIM_SWEEP_PRIME) != 0;
  SweepK w;
  memset(&w, 0, sizeof(w));
  if (!prime) {
    if (!isfinite(args->margin) || !(args->sag >= 0.0f) || !isfinite(args->sag)) return DSIM_E_ARG;
    const int rc = obs_refuse(ctx, n, state, set, args->type_id, args->margin, args->sag, args->clearance_out);
    if (rc) return rc;
    // a piece reaches `half` from its midpoint at most, so whatever is within R + sag + margin of it is within reach of the midpoint
    const double reach = (double)set->grid.reach;
    const double half = reach - ((double)ctx_r_max(ctx) + (double)args->sag + (double)args->margin);
    if (!(half >= reach / 1024.0)) return DSIM_E_ARG;
    // 2^-10 shorter than allowed: covers the rounding of the length, of the quotient and of the midpoints (the lists carry a
    // hundredth of a cell on top, dsim_obstacle_grid.h)
    w.inv_piece = (float)(1.0 / (2.0 * half * (1.0 - 1.0 / 1024.0)));
  }
  const int rc = obs_kargs(ctx, n, state, set, args->offset, args->type_id, args->margin, args->clearance_out, args->nearest_out,
                           args->contacts_out, &w.o);
  if (rc) return rc;
  w.sag = args->sag; w.prev = args->prev; w.keep_prev = (fl & DSIM_SWEEP_KEEP_PREV) ? 1 : 0;
  w.unswept_out = (unsigned long long*)args->unswept_out;
  if (!prime) return obs_launch(k_obstacle_sweep<true>, k_obstacle_sweep<false>, set, w.o.tiles, stream, w);
  hipLaunchKernelGGL(k_sweep_prime, dim3(obs_blocks(w.o.tiles)), dim3(256), 0, (hipStream_t)stream, w);
  return (int)hipGetLastError();
}
