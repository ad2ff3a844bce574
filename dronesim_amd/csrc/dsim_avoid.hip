// Velocity safety filter (dsim_velocity_filter): per drone the smallest change of a wished velocity u that meets the control-barrier
// half-spaces a_j . v >= b_j its floor, its obstacle witnesses and its neighbours give (include/dronesim_amd.h has the rows).
// Compiled as part of dsim_downwash.hip, which includes it: it reads the state block and the type table as dsim_knn does.
//
// One drone per lane.  The solve is the incremental one of three-dimensional ORCA, without its speed ball: the rows are taken in
// their priority order and the lane keeps the optimum v of the rows kept so far.  A row that v meets is kept and changes nothing
// (hence v == u bit for bit while nothing is violated).  A violated row puts the new optimum on its own plane — the kept region is
// convex and holds v, so it reaches the half-space only through the plane — and the lane solves the two-dimensional problem there:
// the projection of u onto the plane, against the rows kept so far in order, a violated one of which puts the point on the line of
// the two planes, where the rows before it clip an interval (the one-dimensional problem).  An empty interval, or a plane parallel
// to one it violates, says that the row cannot be met together with the rows kept: it is dropped, its bit set, v stays.
//
// Rows are not stored.  A lane-private array of 25 rows indexed by a loop counter is scratch memory, which no kernel of the
// library uses; 25 x 16 B per lane in LDS is 100 KiB per workgroup of 256 — one workgroup, four waves, per CU, in a kernel whose
// time is the latency of its loads.  A row is REBUILT from its slot-major records each time a loop needs it: the loads are coalesced
// (one 256-byte row segment per wave and field) and every read after the first comes from the vector L1 / L2, and only violated
// rows ever cause a second read.  LDS per workgroup: 0 bytes.  The resource report of the build (78 VGPRs, no scratch) allows 6 waves per
// SIMD, 24 per CU; a drone all of whose rows are met reads each record once: 32 B per neighbour slot, 20 B (32 with velocities) per
// obstacle slot, and 56 B of its own read and written, DESIGN.md section 7.
//
// Directions of nearly parallel planes.  The line of two unit normals at angle t is known from their fp32 cross product only to
// 1e-7 / t when the products are rounded one by one; the cross product here is Kahan's (each difference of products with one fma
// for the rounding of the other), good to 2 ulp, and the step inside the plane goes along (a_i x a_j) x a_i, which has no
// cancellation.  The error of a vertex is then eps |v|, what fp32 allows.

struct AvoidK {
  KView st;
  const DevType* types;
  const uint8_t* type_id;
  int n_types;
  long long n, n_pad;
  const float* u;            // [3][n_pad]
  const float* offset;       // [3][n_pad] or null
  float alpha, share, buffer_drone, buffer_obstacle, floor_z;
  int has_floor, k, m;
  const int* nb_index;       // [k][n_pad]
  const float* nb_dist;      // [k][n_pad]
  const float* nb_rel_pos;   // [k][3][n_pad]
  const float* nb_rel_vel;   // [k][3][n_pad]
  const float* w_clearance;  // [m][n_pad]
  const int* w_body;         // [m][n_pad]
  const float* w_rel;        // [m][3][n_pad]
  const float* w_vel;        // [m][3][n_pad] or null
  float* v_out;              // [3][n_pad]
  int* dropped;              // [n_pad]
  unsigned long long* counters;   // [2] or null
};

#define AVOID_ROWS 25          // bit 0 the floor, 1 .. 8 the obstacle slots, 9 .. 24 the neighbour slots
#define AVOID_TINY 1.0e-6f     // [m] a distance at or below it gives no direction
#define AVOID_PAR2 1.0e-10f    // |a_i x a_j|^2 at or below it: the two planes are parallel
#define AVOID_PAR1 1.0e-5f     // |a_k . d| at or below it: the row is parallel to the line

struct AvoidMe { float px, py, pz, vx, vy, vz, R, offz; };
struct AvoidRow { float x, y, z, b; };          // unit normal (or 0 0 0 for a row without direction) and offset

__device__ __forceinline__ bool avoid_finite(float x) { return fabsf(x) <= 3.0e38f; }
// a b - c d, the rounding of c d recovered by one fma (Kahan)
__device__ __forceinline__ float avoid_dop(float a, float b, float c, float d) {
  const float w = c * d;
  const float e = fmaf(-c, d, w);
  const float f = fmaf(a, b, -w);
  return f + e;
}

// Row r of drone i, or false when the slot is not a row: an unused index or body, a non-finite entry, a distance at or below
// AVOID_TINY.  The normal is brought to unit length (a . v >= b is the same half-space); a normal of no length stays 0 with its b.
__device__ __forceinline__ bool avoid_row(const AvoidK& a, long long i, int r, const AvoidMe& me, AvoidRow& o) {
  float ax, ay, az, b;
  if (r == 0) {
    if (!a.has_floor) return false;
    ax = 0.0f; ay = 0.0f; az = 1.0f;
    b = -a.alpha * (me.pz - me.offz - a.floor_z - me.R);
  } else if (r <= 8) {
    const int s = r - 1;
    if (s >= a.m) return false;
    const long long at = (long long)s * a.n_pad + i;
    if (a.w_body[at] < 0) return false;
    const float c = a.w_clearance[at];
    const float* rel = a.w_rel + (long long)s * 3 * a.n_pad + i;
    const float d = c + me.R;
    if (!(d > AVOID_TINY)) return false;
    ax = -rel[0] / d; ay = -rel[a.n_pad] / d; az = -rel[2 * a.n_pad] / d;
    float vn = 0.0f;
    if (a.w_vel) {
      const float* vel = a.w_vel + (long long)s * 3 * a.n_pad + i;
      vn = ax * vel[0] + ay * vel[a.n_pad] + az * vel[2 * a.n_pad];
    }
    b = vn - a.alpha * (c - a.buffer_obstacle);
  } else {
    const int t = r - 9;
    if (t >= a.k) return false;
    const long long at = (long long)t * a.n_pad + i;
    const int j = a.nb_index[at];
    if (j < 0 || (long long)j >= a.n) return false;
    const float d = a.nb_dist[at];
    if (!(d > AVOID_TINY)) return false;
    const float* rp = a.nb_rel_pos + (long long)t * 3 * a.n_pad + i;
    const float* rv = a.nb_rel_vel + (long long)t * 3 * a.n_pad + i;
    ax = -rp[0] / d; ay = -rp[a.n_pad] / d; az = -rp[2 * a.n_pad] / d;
    const float Rj = a.types[a.type_id ? min((int)a.type_id[j], a.n_types - 1) : 0].coll_sphere;
    const float h = d - (me.R + Rj) - a.buffer_drone;
    const float c = ax * rv[0] + ay * rv[a.n_pad] + az * rv[2 * a.n_pad] - a.alpha * h;
    b = ax * me.vx + ay * me.vy + az * me.vz + a.share * c;
  }
  if (!(avoid_finite(ax) && avoid_finite(ay) && avoid_finite(az) && avoid_finite(b))) return false;
  const float aa = ax * ax + ay * ay + az * az;
  if (aa > 1.0e-12f) {
    const float inv = 1.0f / DSIM_SQRT(aa);
    ax *= inv; ay *= inv; az *= inv; b *= inv;
  } else {
    ax = 0.0f; ay = 0.0f; az = 0.0f;            // 0 . v >= b: met by every v or by none
  }
  o.x = ax; o.y = ay; o.z = az; o.b = b;
  return true;
}

// The closest point to u on the plane of row `ri` that meets the rows of `kept` (all below ri), or false when there is none.
__device__ __forceinline__ bool avoid_on_plane(const AvoidK& a, long long i, const AvoidMe& me, const AvoidRow& ri, unsigned kept,
                                               float ux, float uy, float uz, float& ox, float& oy, float& oz) {
  if (ri.x == 0.0f && ri.y == 0.0f && ri.z == 0.0f) return false;              // a violated row without a plane
  const float s0 = ri.b - (ri.x * ux + ri.y * uy + ri.z * uz);
  float px = ux + s0 * ri.x, py = uy + s0 * ri.y, pz = uz + s0 * ri.z;
  for (unsigned mj = kept; mj != 0u; mj &= mj - 1u) {
    const int j = __builtin_ctz(mj);
    AvoidRow rj;
    avoid_row(a, i, j, me, rj);
    const float gap = rj.b - (rj.x * px + rj.y * py + rj.z * pz);
    if (!(gap > 0.0f)) continue;
    // the line of the two planes: direction d, and from p the step inside plane i that reaches plane j
    float dx = avoid_dop(ri.y, rj.z, ri.z, rj.y), dy = avoid_dop(ri.z, rj.x, ri.x, rj.z), dz = avoid_dop(ri.x, rj.y, ri.y, rj.x);
    const float dd = dx * dx + dy * dy + dz * dz;
    if (!(dd > AVOID_PAR2)) return false;
    const float len = DSIM_SQRT(dd), inv = 1.0f / len;
    dx *= inv; dy *= inv; dz *= inv;
    const float wx = dy * ri.z - dz * ri.y, wy = dz * ri.x - dx * ri.z, wz = dx * ri.y - dy * ri.x;      // d x a_i, unit, a_j . w = len
    const float step = gap / len;
    const float x0 = px + step * wx, y0 = py + step * wy, z0 = pz + step * wz;
    float lo = -INFINITY, hi = INFINITY;
    const unsigned below = kept & ((1u << j) - 1u);
    for (unsigned mk = below; mk != 0u; mk &= mk - 1u) {
      const int k = __builtin_ctz(mk);
      AvoidRow rk;
      avoid_row(a, i, k, me, rk);
      const float den = rk.x * dx + rk.y * dy + rk.z * dz;
      const float num = rk.b - (rk.x * x0 + rk.y * y0 + rk.z * z0);
      if (fabsf(den) <= AVOID_PAR1) {
        if (num > 0.0f) return false;
        continue;
      }
      const float t = num / den;
      if (den > 0.0f) lo = fmaxf(lo, t);
      else hi = fminf(hi, t);
      if (lo > hi) return false;
    }
    const float tu = dx * (ux - x0) + dy * (uy - y0) + dz * (uz - z0);
    const float t = fminf(fmaxf(tu, lo), hi);
    px = x0 + t * dx; py = y0 + t * dy; pz = z0 + t * dz;
  }
  ox = px; oy = py; oz = pz;
  return true;
}

__global__ __launch_bounds__(256) void k_velocity_filter(AvoidK a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < a.n;
  bool changed = false, lost = false;
  if (live) {
    const float* s = a.st.base + kv_off(a.st, i);
    AvoidMe me;
    me.px = s[0]; me.py = s[a.st.field_stride]; me.pz = s[2 * a.st.field_stride];
    const float* sv = s + (long long)DSIM_F_VEL * a.st.field_stride;
    me.vx = sv[0]; me.vy = sv[a.st.field_stride]; me.vz = sv[2 * a.st.field_stride];
    me.R = a.types[a.type_id ? min((int)a.type_id[i], a.n_types - 1) : 0].coll_sphere;
    me.offz = a.offset ? a.offset[2 * a.n_pad + i] : 0.0f;
    const float ux = a.u[i], uy = a.u[a.n_pad + i], uz = a.u[2 * a.n_pad + i];
    float vx = ux, vy = uy, vz = uz;
    unsigned kept = 0u, drop = 0u;
    const bool sane = avoid_finite(ux) && avoid_finite(uy) && avoid_finite(uz) && avoid_finite(me.px) && avoid_finite(me.py)
                      && avoid_finite(me.pz) && avoid_finite(me.vx) && avoid_finite(me.vy) && avoid_finite(me.vz) && avoid_finite(me.offz);
    if (sane) {
      for (int r = a.has_floor ? 0 : 1; r < AVOID_ROWS; ++r) {
        if (r == 1 + a.m) r = 9;                 // (the slots the call does not carry)
        if (r >= 9 + a.k) break;
        AvoidRow row;
        if (!avoid_row(a, i, r, me, row)) continue;
        if (row.x * vx + row.y * vy + row.z * vz >= row.b) { kept |= 1u << r; continue; }
        float nx, ny, nz;
        if (avoid_on_plane(a, i, me, row, kept, ux, uy, uz, nx, ny, nz)) {
          vx = nx; vy = ny; vz = nz; kept |= 1u << r;
        } else {
          drop |= 1u << r;
        }
      }
    }
    a.v_out[i] = vx; a.v_out[a.n_pad + i] = vy; a.v_out[2 * a.n_pad + i] = vz;
    a.dropped[i] = (int)drop;
    changed = sane && (vx != ux || vy != uy || vz != uz);
    lost = drop != 0u;
  }
  if (!a.counters) return;
  const unsigned long long mc = __ballot(changed), ml = __ballot(lost);
  if ((threadIdx.x & 63u) == 0u) {
    if (mc != 0ULL) atomicAdd(&a.counters[0], (unsigned long long)__popcll(mc));
    if (ml != 0ULL) atomicAdd(&a.counters[1], (unsigned long long)__popcll(ml));
  }
}

extern "C" int dsim_velocity_filter(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_filter_args* args) {
  if (!ctx || !args || n <= 0 || n > state.n_pad) return DSIM_E_ARG;
  const dsim_filter_args& f = *args;
  if (!f.u || !f.v_out || !f.dropped_out) return DSIM_E_ARG;
  if (f.k < 0 || f.k > 16 || f.m < 0 || f.m > DSIM_WITNESSES_MAX) return DSIM_E_ARG;
  if (f.k == 0 && f.m == 0 && !f.has_floor) return DSIM_E_ARG;
  if (!(f.alpha > 0.0f) || !isfinite(f.alpha) || !(f.share > 0.0f) || !(f.share <= 1.0f)) return DSIM_E_ARG;
  if (!(f.buffer_drone >= 0.0f) || !isfinite(f.buffer_drone) || !(f.buffer_obstacle >= 0.0f) || !isfinite(f.buffer_obstacle)) return DSIM_E_ARG;
  if (f.has_floor && !isfinite(f.floor)) return DSIM_E_ARG;
  if (f.k > 0 && (!f.nb_index || !f.nb_dist || !f.nb_rel_pos || !f.nb_rel_vel)) return DSIM_E_ARG;
  if (f.m > 0 && (!f.wit_clearance || !f.wit_body || !f.wit_rel)) return DSIM_E_ARG;
  if (ctx->n_types > 1 && !f.type_id) return DSIM_E_ARG;
  AvoidK a;
  memset(&a, 0, sizeof(a));
  const int rc = make_kview(state, 10, &a.st);                  // (position and velocity)
  if (rc) return rc;
  a.types = ctx->d_types; a.type_id = f.type_id; a.n_types = ctx->n_types;
  a.n = n; a.n_pad = state.n_pad; a.u = f.u; a.offset = f.offset;
  a.alpha = f.alpha; a.share = f.share; a.buffer_drone = f.buffer_drone; a.buffer_obstacle = f.buffer_obstacle;
  a.floor_z = f.has_floor ? f.floor : 0.0f; a.has_floor = f.has_floor ? 1 : 0; a.k = f.k; a.m = f.m;
  a.nb_index = f.nb_index; a.nb_dist = f.nb_dist; a.nb_rel_pos = f.nb_rel_pos; a.nb_rel_vel = f.nb_rel_vel;
  a.w_clearance = f.wit_clearance; a.w_body = f.wit_body; a.w_rel = f.wit_rel; a.w_vel = f.m > 0 ? f.wit_vel : nullptr;
  a.v_out = f.v_out; a.dropped = f.dropped_out; a.counters = (unsigned long long*)f.counters;
  hipLaunchKernelGGL(k_velocity_filter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}
