// Nearest-neighbour observation (dsim_knn): per local drone the k closest drones within a radius, in ascending order of distance,
// with their distance, relative position and relative velocity, and the exact number of drones within the radius
// (include/dronesim_amd.h).  Compiled as part of dsim_downwash.hip, which includes it: it shares the grid's record (DwK),
// grid_build and the counting-sort entry (x, y, z, world index bits) of the adjacency.

struct KnnK {
  float radius2;
  int k;                 // 1 .. KMAX of the instance
  int* index_out;        // [k][n_pad]
  float* dist_out;       // [k][n_pad] or null
  float* rel_pos_out;    // [k][3][n_pad] or null
  float* rel_vel_out;    // [k][3][n_pad] or null (the world is this fleet: a world index is a state index)
  int* count_out;        // [n_pad] or null
};

#define KNN_NONE 0x7fffffff     // the index of an empty slot while the list is kept (written as -1): above every world index

// Receivers in grid order, one lane each, 3 x 3 cells, as k_adj_query: the lanes of a wave sit in the same or neighbouring cells
// and read the same candidate ranges, one 16-byte load per candidate.  Cells are `radius` or more, so a pair with d_ij < radius is
// less than one cell apart in x and in y: unclamped, its two cell indices differ by at most one per axis, and clamping a drone
// from outside the box into a border cell is monotone — it never moves two indices further apart — so the pair is still found in
// adjacent cells (as k_clearance_query; the cell index is rounded in fp32, which matters only to a pair whose distance along one
// axis is within that rounding of a whole cell: the host's grids keep the cell a thousandth above the radius).
// The lane keeps the KMAX least keys (d^2, j) in registers, ascending: kd[] / kj[] are only ever indexed by unrolled constants.
// An empty slot is (+inf, KNN_NONE).  A candidate is inserted when it is within the radius and below the worst kept key; the
// test is one ballot per candidate, so a wave none of whose lanes improves skips the chain.  The chain is a bubble insertion of
// compare-exchanges, selects only: the carried element takes a slot whose key is above its own and carries that slot's on; a
// lane that does not insert carries the empty key, which moves nothing.  The first k of the KMAX kept are the answer.
// A position that is not finite fails `d^2 < radius^2` on either side of the pair: such a receiver counts nobody, such a candidate
// is nobody's neighbour.
template <int KMAX>
__global__ __launch_bounds__(256) void k_knn_query(DwK a, KnnK q) {
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  if (s >= a.m) return;
  const float4 me = a.sorted[s];
  const int jme = __float_as_int(me.w);
  const long long i = (long long)jme - a.local_offset;
  if (i < 0 || i >= a.n) return;                                // another rank's drone: a candidate only
  const float inf = __int_as_float(0x7f800000);
  float kd[KMAX];
  int kj[KMAX];
#pragma unroll
  for (int t = 0; t < KMAX; ++t) { kd[t] = inf; kj[t] = KNN_NONE; }
  int cx, cy, cnt = 0;
  dw_cell(a, me.x, me.y, cx, cy);
  for (int yy = max(cy - 1, 0); yy <= min(cy + 1, a.ny - 1); ++yy) {
    // the three cells of a row are contiguous in the sorted array
    const int c0 = yy * a.nx + max(cx - 1, 0), c1 = yy * a.nx + min(cx + 1, a.nx - 1);
    const int s_end = a.count[c1 + 1];
    for (int s2 = a.count[c0]; s2 < s_end; ++s2) {
      const float4 p = a.sorted[s2];
      const float dx = p.x - me.x, dy = p.y - me.y, dz = p.z - me.z;
      const float d2 = dx * dx + dy * dy + dz * dz;
      const int j = __float_as_int(p.w);
      const bool near = j != jme && d2 < q.radius2;
      cnt += near ? 1 : 0;
      const bool better = near && (d2 < kd[KMAX - 1] || (d2 == kd[KMAX - 1] && j < kj[KMAX - 1]));
      if (__ballot(better) != 0ULL) {
        float d = better ? d2 : inf;
        int jj = better ? j : KNN_NONE;
#pragma unroll
        for (int t = 0; t < KMAX; ++t) {
          const bool lt = d < kd[t] || (d == kd[t] && jj < kj[t]);
          const float od = kd[t];
          const int oj = kj[t];
          kd[t] = lt ? d : od;
          kj[t] = lt ? jj : oj;
          d = lt ? od : d;
          jj = lt ? oj : jj;
        }
      }
    }
  }
  if (q.count_out) q.count_out[i] = cnt;
  float vx = 0.0f, vy = 0.0f, vz = 0.0f;
  if (q.rel_vel_out) {
    const float* v = a.st.base + kv_off(a.st, i) + (long long)DSIM_F_VEL * a.st.field_stride;
    vx = v[0]; vy = v[a.st.field_stride]; vz = v[2 * a.st.field_stride];
  }
#pragma unroll
  for (int t = 0; t < KMAX; ++t) {
    if (t < q.k) {
      const bool used = kj[t] != KNN_NONE;
      const long long j = used ? kj[t] : jme;                   // (an empty slot reads the receiver itself: a valid address)
      q.index_out[(long long)t * a.n_pad + i] = used ? kj[t] : -1;
      if (q.dist_out) q.dist_out[(long long)t * a.n_pad + i] = used ? DSIM_SQRT(kd[t]) : inf;
      if (q.rel_pos_out) {
        float* o = q.rel_pos_out + (long long)t * 3 * a.n_pad + i;
        o[0] = used ? dw_pos(a, j, 0) - me.x : 0.0f;
        o[a.n_pad] = used ? dw_pos(a, j, 1) - me.y : 0.0f;
        o[2 * a.n_pad] = used ? dw_pos(a, j, 2) - me.z : 0.0f;
      }
      if (q.rel_vel_out) {
        const float* v = a.st.base + kv_off(a.st, j) + (long long)DSIM_F_VEL * a.st.field_stride;
        float* o = q.rel_vel_out + (long long)t * 3 * a.n_pad + i;
        o[0] = used ? v[0] - vx : 0.0f;
        o[a.n_pad] = used ? v[a.st.field_stride] - vy : 0.0f;
        o[2 * a.n_pad] = used ? v[2 * a.st.field_stride] - vz : 0.0f;
      }
    }
  }
}

extern "C" {

// the counting-sort form of the grid, as dsim_adjacency takes it
int64_t dsim_knn_workspace(int64_t m, int32_t nx, int32_t ny) { return dsim_downwash_workspace(m, nx, ny); }

int dsim_knn(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_knn_args* args) {
  if (!ctx || !args || !args->grid || !args->index_out) return DSIM_E_ARG;
  const dsim_downwash_args* g = args->grid;
  if (args->flags != 0 || args->k < 1 || args->k > 16 || !(args->radius > 0.0f) || !isfinite(args->radius)) return DSIM_E_ARG;
  if (g->halo) return DSIM_E_UNSUPPORTED;
  if (args->rel_vel_out && g->pos_all) return DSIM_E_ARG;       // the velocities of the rest of the world do not travel
  if (g->nx < 1 || g->ny < 1 || g->m < 1 || g->workspace_len < dsim_knn_workspace(g->m, g->nx, g->ny)) return DSIM_E_ARG;
  DwK a;
  const hipStream_t st_ = (hipStream_t)stream;
  int rc = grid_build(DwCall{ctx, st_, n, state, g, GridGeo(*g)}, args->radius, &a);
  if (rc) return rc;
  const KnnK q = {args->radius * args->radius, args->k, args->index_out, args->dist_out, args->rel_pos_out, args->rel_vel_out,
                  args->count_out};
  const dim3 grid(grid_for(a.m)), block(256);
  if (args->k <= 4) hipLaunchKernelGGL(k_knn_query<4>, grid, block, 0, st_, a, q);
  else if (args->k <= 8) hipLaunchKernelGGL(k_knn_query<8>, grid, block, 0, st_, a, q);
  else hipLaunchKernelGGL(k_knn_query<16>, grid, block, 0, st_, a, q);
  return (int)hipGetLastError();
}

}  // extern "C"
