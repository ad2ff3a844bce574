// Swept drone-drone contact watch (dsim_clearance_sweep): per-drone clearance between the vehicles' bounding spheres, each grown by a
// sag and moved along the chord from the position the previous call saw to the current one, both drones of a pair at the same
// parameter s (include/dronesim_amd.h).  Compiled as part of dsim_downwash.hip, which includes it: it shares the grid's record (DwK),
// the point watch's (ClrK), grid_build, sort_ws and WsWalk.

struct ClrSweepK {
  float4* sorted0;               // [m] (p0, unused) at the slot where DwK.sorted holds (p1, R)
  float* prev;                   // SoA [3][n_pad], world frame
  float sag;
  float travel2;                 // travel^2 (1 - 2^-20): a chord whose squared length, as fp32 rounds it, passes is no longer than travel
  int keep_prev;
  unsigned long long* unswept_out;
};

// prev := the current position of every drone, and nothing else (DSIM_SWEEP_PRIME)
__global__ __launch_bounds__(256) void k_clr_sweep_prime(DwK a, ClrSweepK w) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.n) return;
  w.prev[j] = dw_pos(a, j, 0);
  w.prev[a.n_pad + j] = dw_pos(a, j, 1);
  w.prev[2 * a.n_pad + j] = dw_pos(a, j, 2);
}

// One lane per world entry (the world is this fleet: m = n, no pos_all).  The drone is binned where it IS (the counts are
// k_dw_count's); its chord's other end rides at the same slot of a second array.  A chord the cell rule does not cover — longer than
// travel, or with a component that is not finite on either end (the comparison fails for NaN and infinity) — collapses to its end:
// the drone is a point sample, counted when it takes part (R > 0), by one ballot and one atomic per wave.  Entry j of prev is read by
// this lane alone, before it is written.
__global__ __launch_bounds__(256) void k_clr_sweep_scatter(DwK a, ClrK c, ClrSweepK w) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool live = j < a.m;
  bool point = false;
  if (live) {
    const float x = dw_pos(a, j, 0), y = dw_pos(a, j, 1), z = dw_pos(a, j, 2);
    float x0 = w.prev[j], y0 = w.prev[a.n_pad + j], z0 = w.prev[2 * a.n_pad + j];
    const float r = a.types[a.type_id ? min((int)a.type_id[j], a.n_types - 1) : 0].coll_sphere;
    const float ux = x - x0, uy = y - y0, uz = z - z0;
    const bool swept = ux * ux + uy * uy + uz * uz <= w.travel2;
    if (!swept) { x0 = x; y0 = y; z0 = z; }
    point = !swept && r > 0.0f;
    if (!w.keep_prev) { w.prev[j] = x; w.prev[a.n_pad + j] = y; w.prev[2 * a.n_pad + j] = z; }
    int cx, cy;
    const int slot = atomicAdd(&a.cursor[dw_cell(a, x, y, cx, cy)], 1);
    a.sorted[slot] = make_float4(x, y, z, r);
    w.sorted0[slot] = make_float4(x0, y0, z0, 0.0f);
    c.sidx[slot] = (int)j;
  }
  const unsigned long long pts = __ballot(point);
  if (w.unswept_out && pts != 0ULL && (threadIdx.x & 63u) == 0u) atomicAdd(w.unswept_out, (unsigned long long)__popcll(pts));
}

// As k_clearance_query: receivers in grid order, one lane each, 3 x 3 cells of the grid of the CURRENT positions.  Cells are
// 2 (R_max + sag) + margin + 2 travel or more: a pair with c_ij < margin has |d(s*)| < 2 (R_max + sag) + margin somewhere along the
// step, and |d1| <= |d(s*)| + |Delta| with |Delta| <= the two chords' lengths <= 2 travel, so its current positions are less than one
// cell apart in x and in y (clamping into a border cell is monotone, as in the point query).
// Per candidate, two 16-byte loads: d0 = p0_j - p0_i, d1 = p1_j - p1_i, Delta = d1 - d0 — differences of nearby coordinates first,
// the interpolation after — s* = clamp(-d0.Delta / Delta.Delta, 0, 1) (0 where Delta = 0), and the least of |d0|^2, |d1|^2,
// |d0 + s* Delta|^2: whatever rounding does to s*, the result is not above either end's, which is the point query's there.
// The lane keeps key = dist - (R_j + sag) against margin + R_i + sag; overlap is key < R_i + sag.
__global__ __launch_bounds__(256) void k_clearance_sweep_query(DwK a, ClrK c, ClrSweepK w) {
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  bool live = s < a.m;
  const float4 me = live ? a.sorted[s] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const float4 me0 = live ? w.sorted0[s] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const int jme = live ? c.sidx[s] : -1;
  const long long i = (long long)jme - a.local_offset;
  live = live && i >= 0 && i < a.n;
  const float rs = me.w + w.sag;
  float best = c.margin + rs;
  int bslot = -1;
  unsigned pairs = 0;
  if (live && me.w > 0.0f) {
    int cx, cy;
    dw_cell(a, me.x, me.y, cx, cy);
    for (int yy = max(cy - 1, 0); yy <= min(cy + 1, a.ny - 1); ++yy) {
      const int c0 = yy * a.nx + max(cx - 1, 0), c1 = yy * a.nx + min(cx + 1, a.nx - 1);
      for (int s2 = a.count[c0]; s2 < a.count[c1 + 1]; ++s2) {
        const float4 p = a.sorted[s2], q = w.sorted0[s2];
        const float ex = p.x - me.x, ey = p.y - me.y, ez = p.z - me.z;             // d1
        const float bx = q.x - me0.x, by = q.y - me0.y, bz = q.z - me0.z;          // d0
        const float gx = ex - bx, gy = ey - by, gz = ez - bz;                      // Delta
        const float gg = gx * gx + gy * gy + gz * gz;
        const float bg = bx * gx + by * gy + bz * gz;
        const float t = gg > 0.0f ? fminf(fmaxf(-bg * DSIM_RCP(gg), 0.0f), 1.0f) : 0.0f;
        const float mx = bx + t * gx, my = by + t * gy, mz = bz + t * gz;
        const float d2 = fminf(fminf(bx * bx + by * by + bz * bz, ex * ex + ey * ey + ez * ez), mx * mx + my * my + mz * mz);
        const float key = DSIM_SQRT(d2) - (p.w + w.sag);
        const bool seen = s2 != (int)s && p.w > 0.0f;
        if (seen && key < rs && c.sidx[s2] > jme) ++pairs;
        const bool better = seen && key < best;
        best = better ? key : best;
        bslot = better ? s2 : bslot;
      }
    }
  }
  if (live) {
    c.clearance[i] = bslot >= 0 ? best - rs : c.margin;
    if (c.nearest) c.nearest[i] = bslot >= 0 ? c.sidx[bslot] : -1;
  }
  if (__ballot(pairs != 0u) == 0ULL) return;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) pairs += __shfl_xor(pairs, off);
  if ((threadIdx.x & 63u) == 0u) {
    atomicAdd(&c.counters[8 + DSIM_GROUND_SHARDS + (blockIdx.x & (DSIM_DRONE_SHARDS - 1))], (unsigned long long)pairs);
    if (c.pairs_out) atomicAdd(c.pairs_out, (unsigned long long)pairs);
  }
}

// the contact watch's workspace + the chords' other ends (16-byte aligned float4 [m]): one walk for the size and the pointers
static WsWalk clr_sweep_ws(const int32_t* ws, int64_t ncells, int64_t m, ClrK* c, ClrSweepK* w) {
  WsWalk walk = sort_ws(ws, ncells, m).end;
  c->sidx = walk.take<int>(m);
  w->sorted0 = walk.take<float4>(m, true);
  return walk;
}

extern "C" int64_t dsim_clearance_sweep_workspace(int64_t m, int32_t nx, int32_t ny) {
  const int64_t base = dsim_clearance_workspace(m, nx, ny);
  if (base < 0) return -1;
  ClrK c;
  ClrSweepK w;
  const int64_t len = clr_sweep_ws(nullptr, (int64_t)nx * ny, m, &c, &w).len;
  return len > base ? len : base;
}

extern "C" int dsim_clearance_sweep(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_downwash_args* g,
                                    const dsim_clearance_sweep_args* args) {
  if (!args || !args->prev) return DSIM_E_ARG;
  const int32_t fl = args->flags;
  if ((fl & ~(DSIM_SWEEP_KEEP_PREV | DSIM_SWEEP_PRIME)) || fl == (DSIM_SWEEP_KEEP_PREV | DSIM_SWEEP_PRIME)) return DSIM_E_ARG;
  // a sharded world would need prev for every world entry, the other ranks' too
  if (g && (g->pos_all || g->halo)) return DSIM_E_UNSUPPORTED;
  if (!ctx || n <= 0 || n > state.n_pad || (!g && !(fl & DSIM_SWEEP_PRIME))) return DSIM_E_ARG;
  const hipStream_t st_ = (hipStream_t)stream;
  ClrSweepK w;
  memset(&w, 0, sizeof(w));
  w.prev = args->prev; w.keep_prev = (fl & DSIM_SWEEP_KEEP_PREV) ? 1 : 0; w.unswept_out = (unsigned long long*)args->unswept_out;
  if (fl & DSIM_SWEEP_PRIME) {
    DwK a;
    memset(&a, 0, sizeof(a));
    const int rc = make_kview(state, 20 + ctx->max_act, &a.st);
    if (rc) return rc;
    a.n = n; a.n_pad = state.n_pad;
    hipLaunchKernelGGL(k_clr_sweep_prime, dim3(grid_for(n)), dim3(256), 0, st_, a, w);
    return (int)hipGetLastError();
  }
  const float margin = args->margin, sag = args->sag, travel = args->travel;
  if (!args->clearance_out || !(margin > 0.0f) || !isfinite(margin) || !(sag >= 0.0f) || !isfinite(sag) || !(travel > 0.0f) ||
      !isfinite(travel))
    return DSIM_E_ARG;
  if (ctx->n_types > 1 && !g->type_id) return DSIM_E_ARG;
  const float r_max = ctx_r_max(ctx);
  if (g->nx < 1 || g->ny < 1 || g->m < 1 || g->workspace_len < dsim_clearance_sweep_workspace(g->m, g->nx, g->ny)) return DSIM_E_ARG;
  DwK a;
  // (the cell rule is grid_build's test of cell against min_cell)
  int rc = grid_build(DwCall{ctx, st_, n, state, g, GridGeo(*g)}, 2.0f * (r_max + sag) + margin + 2.0f * travel, &a, nullptr, nullptr,
                      false);
  if (rc) return rc;
  ClrK c;
  memset(&c, 0, sizeof(c));
  clr_sweep_ws(g->workspace, GridGeo(*g).ncells(), g->m, &c, &w);
  c.margin = margin; c.clearance = args->clearance_out; c.nearest = args->nearest_out; c.counters = ctx->d_counters;
  c.pairs_out = (unsigned long long*)args->pairs_out;
  w.sag = sag;
  // 2^-20 below travel^2: the squared length is three products and two sums in fp32, 2^-22 of it at the most
  w.travel2 = (float)((double)travel * (double)travel * (1.0 - 1.0 / 1048576.0));
  hipLaunchKernelGGL(k_clr_sweep_scatter, dim3(grid_for(a.m)), dim3(256), 0, st_, a, c, w);
  hipLaunchKernelGGL(k_clearance_sweep_query, dim3(grid_for(a.m)), dim3(256), 0, st_, a, c, w);
  return (int)hipGetLastError();
}
