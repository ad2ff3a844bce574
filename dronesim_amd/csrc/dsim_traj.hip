// dsim_traj.hip — the trajectory bank: dsim_trajgen (K min-snap courses in one launch, trajGen.py:13-106) and
// dsim_traj_sample_bank (k_traj_sample with a course per drone).  Compiled as part of dsim_api.hip, which includes it.
#include "dsim_trajgen_tables.h"

// ---- generator ------------------------------------------------------------------------------------------------------
// One lane per course.  The only per-lane arrays indexed at run time are the segment times, their lower bounds and the
// position steps: they live in LDS, one column per lane (a lane touches its own column only: no barrier anywhere).  The
// blocks of the solve are indexed by unrolled loops and stay in registers; what the sweep back needs of the sweep along
// (per interior waypoint R_a, 10, R_ab, 16, and z_a for three axes, 12: R_a a = z_a - R_ab b) goes through the caller's
// workspace, course-minor like the bank.
// The sweep is in square-root form.  A segment's cost is |F e^|^2 / T^7 (F: DSIM_TG_F, 6 x 10, F^T F = M), so the
// cost-so-far is carried as |R a - s|^2 with R upper triangular, and a segment joins it by Householder reflections.  The
// block Cholesky sweep this replaces formed K_bb - Y^T Y, a difference of nearly equal numbers where a short leg follows
// a long one (tests/README_trajgen.md).
#define DSIM_TG_LANES 64
#define DSIM_TG_SEGS (DSIM_TRAJGEN_LMAX - 1)
#define DSIM_TG_KEEP 38
// A pivot of the carried factor smaller than its column was by more than this has lost the digits the published accuracy
// needs (the error goes like 0.2 eps cond^2: tests/README_trajgen.md); squared, because the squares are what is at hand.
#define DSIM_TG_COND_MAX2 (16384.0 * 16384.0)
struct TrajGenK {
  const double* wp; const int* n_wp;
  double *coeffs, *ts; int* n_seg;
  double* cost; int* evals; int* status;
  double* seg_times;      // or null
  double* ws;
  long long K, K_pad;
  int L_max, mode, max_evals;
  double max_vel, gamma;
};

// T, T^2, T^3, T^4 in u; h = u T^-3.5; returns T^-3.5
__device__ __forceinline__ double tg_scales(double T, double u[4], double h[4]) {
  u[0] = T; u[1] = T * T; u[2] = u[1] * T; u[3] = u[1] * u[1];
  const double w = 1.0 / (u[2] * sqrt(T));
#pragma unroll
  for (int r = 0; r < 4; ++r) h[r] = u[r] * w;
  return w;
}

// the sweep along the course: the snap cost at the best interior derivatives.  sT, sD: this lane's LDS columns; segment
// ci takes the time cv instead of its stored one (ci = -1: none).  KEEP: ws (already at this course) receives the factors.
// lost: set where a block that a later segment goes on from has lost its digits (DSIM_TG_COND_MAX2).
template <bool KEEP>
__device__ __forceinline__ double tg_sweep(int n, const double* sT, int ci, double cv, const double* sD, double* ws, long long K_pad,
                                           bool& lost) {
  double top[4][11], c = 0.0;             // columns: R (upper triangular) | what the elimination leaves of b | s, three axes
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int e = 0; e < 11; ++e) top[r][e] = 0.0;
  for (int m = 0; m < n; ++m) {
    const double T = (m == ci) ? cv : sT[m * DSIM_TG_LANES];
    double u[4], h[4], D[6][11];           // columns: F_a U w | F_b U w | -F_d w d, three axes
    const double w = tg_scales(T, u, h);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) { D[i][r] = DSIM_TG_F[i][1 + r] * h[r]; D[i][4 + r] = DSIM_TG_F[i][6 + r] * h[r]; }
#pragma unroll
      for (int x = 0; x < 3; ++x) D[i][8 + x] = -(DSIM_TG_F[i][5] * w) * sD[(m * 3 + x) * DSIM_TG_LANES];
    }
    if (m >= 1) {                                   // (at rest at the start: the first segment has no a)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int e = 4; e < 8; ++e) top[r][e] = 0.0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {                 // the reflection on (top[j], D[:]) that zeroes D[:][j]
        double v0 = top[j][j], nn = v0 * v0;
#pragma unroll
        for (int i = 0; i < 6; ++i) nn += D[i][j] * D[i][j];
        const double norm = sqrt(nn), alpha = v0 >= 0.0 ? -norm : norm;
        v0 -= alpha;
        const double beta = -1.0 / (alpha * v0);
#pragma unroll
        for (int e = j + 1; e < 11; ++e) {
          double dot = v0 * top[j][e];
#pragma unroll
          for (int i = 0; i < 6; ++i) dot += D[i][j] * D[i][e];
          const double f = dot * beta;
          top[j][e] -= f * v0;
#pragma unroll
          for (int i = 0; i < 6; ++i) D[i][e] -= f * D[i][j];
        }
        top[j][j] = alpha;
      }
      if (KEEP) {
        double* o = ws + (long long)(m - 1) * DSIM_TG_KEEP * K_pad;
        int e = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int s = r; s < 4; ++s) o[(e++) * K_pad] = top[r][s];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int s = 4; s < 11; ++s) o[(e++) * K_pad] = top[r][s];
      }
    }
    if (m == n - 1) {                               // at rest at the end: b = 0, what is left of the right-hand sides is cost
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int x = 0; x < 3; ++x) c += D[i][8 + x] * D[i][8 + x];
      break;
    }
    // the six rows left, in b: four reflections make them the next R and s; their last two rows are cost
    double n0[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      n0[j] = 0.0;
#pragma unroll
      for (int i = 0; i < 6; ++i) n0[j] += D[i][4 + j] * D[i][4 + j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double v0 = D[j][4 + j], nn = 0.0;
#pragma unroll
      for (int i = j; i < 6; ++i) nn += D[i][4 + j] * D[i][4 + j];
      const double norm = sqrt(nn), alpha = v0 >= 0.0 ? -norm : norm;
      v0 -= alpha;
      const double beta = -1.0 / (alpha * v0);
#pragma unroll
      for (int e = j + 1; e < 7; ++e) {
        double dot = v0 * D[j][4 + e];
#pragma unroll
        for (int i = j + 1; i < 6; ++i) dot += D[i][4 + j] * D[i][4 + e];
        const double f = dot * beta;
        D[j][4 + e] -= f * v0;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) D[i][4 + e] -= f * D[i][4 + j];
      }
      if (!(n0[j] <= DSIM_TG_COND_MAX2 * nn)) lost = true;
#pragma unroll
      for (int s = 0; s < 4; ++s) top[j][s] = s < j ? 0.0 : (s == j ? alpha : D[j][4 + s]);
#pragma unroll
      for (int x = 0; x < 3; ++x) top[j][8 + x] = D[j][8 + x];
    }
#pragma unroll
    for (int i = 4; i < 6; ++i)
#pragma unroll
      for (int x = 0; x < 3; ++x) c += D[i][8 + x] * D[i][8 + x];
  }
  return c;
}

// the sweep back: interior derivatives from the kept factors, then every segment's ten coefficients per axis and its cost.
// NaN where a coefficient is not finite.
__device__ __forceinline__ double tg_back(int n, const double* sT, const double* sD, const double* ws, long long K_pad,
                                          const double* wp, double* coeffs) {
  double b[3][4], cost = 0.0;
  bool finite = true;
#pragma unroll
  for (int x = 0; x < 3; ++x)
#pragma unroll
    for (int r = 0; r < 4; ++r) b[x][r] = 0.0;                     // at rest at the end
  for (int m = n - 1; m >= 0; --m) {
    const double T = sT[m * DSIM_TG_LANES];
    double u[4], h[4], a[3][4];
    const double w = tg_scales(T, u, h);
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
      for (int r = 0; r < 4; ++r) a[x][r] = 0.0;                   // at rest at the start
    if (m >= 1) {                                                   // R_a a = z_a - R_ab b
      const double* o = ws + (long long)(m - 1) * DSIM_TG_KEEP * K_pad;
      double Ra[4][4], rest[4][7];
      int e = 0;
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int s = r; s < 4; ++s) Ra[r][s] = o[(e++) * K_pad];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int s = 0; s < 7; ++s) rest[r][s] = o[(e++) * K_pad];
#pragma unroll
      for (int x = 0; x < 3; ++x)
#pragma unroll
        for (int r = 3; r >= 0; --r) {
          double t = rest[r][4 + x];
#pragma unroll
          for (int s = 0; s < 4; ++s) t -= rest[r][s] * b[x][s];
#pragma unroll
          for (int k = r + 1; k < 4; ++k) t -= Ra[r][k] * a[x][k];
          a[x][r] = t / Ra[r][r];
        }
    }
    double ip[10];
    ip[0] = 1.0; ip[1] = 1.0 / T;
#pragma unroll
    for (int j = 2; j < 10; ++j) ip[j] = ip[j - 1] * ip[1];
#pragma unroll
    for (int x = 0; x < 3; ++x) {
      double e[10];                                                 // scaled end values of p - wp[m]
      e[0] = 0.0; e[5] = sD[(m * 3 + x) * DSIM_TG_LANES];
#pragma unroll
      for (int r = 0; r < 4; ++r) { e[1 + r] = a[x][r] * u[r]; e[6 + r] = b[x][r] * u[r]; }
      double en = 0.0;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        double t = 0.0;
#pragma unroll
        for (int s = 1; s < 10; ++s) t += DSIM_TG_F[i][s] * e[s];
        en += t * t;
      }
      cost += en * (w * w);
      coeffs[((long long)(m * 10) * 3 + x) * K_pad] = wp[(long long)(m * 3 + x) * K_pad];
#pragma unroll
      for (int j = 1; j < 10; ++j) {
        double t = 0.0;
#pragma unroll
        for (int s = 1; s < 10; ++s) t += DSIM_TG_AINV[j][s] * e[s];
        t *= ip[j];
        finite = finite && isfinite(t);
        coeffs[((long long)(m * 10 + j) * 3 + x) * K_pad] = t;
      }
    }
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
      for (int r = 0; r < 4; ++r) b[x][r] = a[x][r];
  }
  return finite ? cost : __builtin_nan("");
}

// a course that cannot be made: NaN everywhere, n_seg 0 (this course only)
__device__ __forceinline__ void tg_refuse(const TrajGenK& a, long long k, int status, int evals) {
  const double qnan = __builtin_nan("");
  for (int e = 0; e < (a.L_max - 1) * 30; ++e) a.coeffs[(long long)e * a.K_pad + k] = qnan;
  for (int l = 0; l < a.L_max; ++l) a.ts[(long long)l * a.K_pad + k] = qnan;
  if (a.seg_times) for (int m = 0; m < a.L_max - 1; ++m) a.seg_times[(long long)m * a.K_pad + k] = qnan;
  a.cost[k] = qnan; a.evals[k] = evals; a.status[k] = status; a.n_seg[k] = 0;
}

__global__ __launch_bounds__(DSIM_TG_LANES) void k_trajgen(TrajGenK a) {
  __shared__ double s_T[DSIM_TG_SEGS * DSIM_TG_LANES], s_lo[DSIM_TG_SEGS * DSIM_TG_LANES], s_D[DSIM_TG_SEGS * 3 * DSIM_TG_LANES];
  const long long k = (long long)blockIdx.x * DSIM_TG_LANES + threadIdx.x;
  if (k >= a.K) return;
  double* sT = s_T + threadIdx.x; double* sLo = s_lo + threadIdx.x; double* sD = s_D + threadIdx.x;
  const double* wp = a.wp + k;
  double* coeffs = a.coeffs + k;
  double* ts = a.ts + k;
  const double qnan = __builtin_nan("");
  const int L = a.n_wp[k];
  int bad = (L < 2 || L > a.L_max) ? DSIM_TRAJGEN_BAD_COUNT : 0;
  const int n = bad ? 0 : L - 1;
  for (int m = 0; m < n; ++m) {
    // Tmin as numpy makes it (trajGen.py:33-34: LA.norm of the difference over max_vel), rounding for rounding
#pragma clang fp contract(off)
    double s = 0.0;
#pragma unroll
    for (int x = 0; x < 3; ++x) {
      const double p0 = wp[(long long)(m * 3 + x) * a.K_pad], p1 = wp[(long long)((m + 1) * 3 + x) * a.K_pad];
      if (!isfinite(p0) || !isfinite(p1)) bad = bad ? bad : DSIM_TRAJGEN_BAD_WAYPOINT;
      const double e = p0 - p1;
      sD[(m * 3 + x) * DSIM_TG_LANES] = p1 - p0;
      s += e * e;
    }
    const double lo = sqrt(s) / a.max_vel;
    if (!bad && !(lo > 0.0 && isfinite(lo))) bad = DSIM_TRAJGEN_BAD_SEGMENT;
    sLo[m * DSIM_TG_LANES] = lo;
    double T = lo;
    if (a.mode == DSIM_TRAJGEN_GIVEN) {
      T = ts[(long long)(m + 1) * a.K_pad] - ts[(long long)m * a.K_pad];
      if (!bad && !(T > 0.0 && isfinite(T))) bad = DSIM_TRAJGEN_BAD_TIME;
    }
    sT[m * DSIM_TG_LANES] = T;
  }
  if (bad) { tg_refuse(a, k, bad, 0); return; }
  int evals = 0;
  bool lost = false;
  if (a.mode == DSIM_TRAJGEN_OPTIMIZE) {
    // greedy multiplicative pattern search (include/dronesim_amd.h); one pass of the loop is at most one evaluation, so lanes
    // at different points of their own searches still share the sweep's instructions
    double sum = 0.0;
    for (int m = 0; m < n; ++m) sum += sT[m * DSIM_TG_LANES];
    double Jx = tg_sweep<false>(n, sT, -1, 0.0, sD, nullptr, 0, lost) + a.gamma * sum;
    evals = 1;
    double step = 0.5;
    int i = 0, dir = 0;
    bool accepted = false;
    while (step > 1e-4 && evals < a.max_evals) {
      const double xi = sT[i * DSIM_TG_LANES];
      const double yi = fmax(sLo[i * DSIM_TG_LANES], dir == 0 ? xi * (1.0 + step) : xi / (1.0 + step));
      bool took = false;
      if (yi != xi) {
        sum = 0.0;
        for (int m = 0; m < n; ++m) sum += (m == i) ? yi : sT[m * DSIM_TG_LANES];
        const double Jy = tg_sweep<false>(n, sT, i, yi, sD, nullptr, 0, lost) + a.gamma * sum;
        ++evals;
        if (Jy < Jx) { sT[i * DSIM_TG_LANES] = yi; Jx = Jy; accepted = true; took = true; }
      }
      if (took || dir == 1) { dir = 0; ++i; } else dir = 1;       // after a step up that was taken, a step down would only undo it
      if (i == n) {
        i = 0;
        if (!accepted) step *= 0.5;
        accepted = false;
      }
    }
  }
  // what the search met on its way does not count: the course is judged at the times it is made for.  T^9 and T^-9 scale
  // its coefficients and must be normal numbers
  lost = false;
  for (int m = 0; m < n; ++m) {
    const double T = sT[m * DSIM_TG_LANES], T3 = T * T * T, T9 = T3 * T3 * T3;
    if (!(T9 >= 0x1p-1000 && T9 <= 0x1p1000)) lost = true;
  }
  if (a.mode != DSIM_TRAJGEN_GIVEN) {               // TS[1:] = cumsum(T), trajGen.py:42
    double acc = 0.0;
    ts[0] = 0.0;
    for (int m = 0; m < n; ++m) { acc += sT[m * DSIM_TG_LANES]; ts[(long long)(m + 1) * a.K_pad] = acc; }
  }
  for (int l = n + 1; l < a.L_max; ++l) ts[(long long)l * a.K_pad] = qnan;
  if (a.seg_times) for (int m = 0; m < a.L_max - 1; ++m) a.seg_times[(long long)m * a.K_pad + k] = m < n ? sT[m * DSIM_TG_LANES] : qnan;
  double* ws = a.ws ? a.ws + k : nullptr;           // (null only at L_max = 2, where no course has an interior waypoint)
  tg_sweep<true>(n, sT, -1, 0.0, sD, ws, a.K_pad, lost);
  const double cost = tg_back(n, sT, sD, ws, a.K_pad, wp, coeffs);
  if (lost || !isfinite(cost)) { tg_refuse(a, k, DSIM_TRAJGEN_BAD_CONDITION, evals); return; }
  for (int e = n * 30; e < (a.L_max - 1) * 30; ++e) coeffs[(long long)e * a.K_pad] = qnan;
  a.cost[k] = cost; a.evals[k] = evals; a.status[k] = 0; a.n_seg[k] = n;
}

// ---- sampler, a course per drone -------------------------------------------------------------------------------------
struct TrajBankK {
  KView tg;
  const double* coeffs;   // bank, course-minor
  const double* ts;
  const int* n_seg;
  const int* traj_id;     // [n_pad] or null (identity)
  double* t;              // [n_pad]
  double* yaw_state;      // SoA [3][n_pad]
  const float* offset;    // SoA [3][n_pad] or null
  long long n, n_pad, K, K_pad;
  int L_max;
  double dt_advance;
};
__global__ __launch_bounds__(256) void k_traj_sample_bank(TrajBankK a) {
  // k_traj_sample's statements in k_traj_sample's order, with the course's stride in the two table reads; no fused
  // multiply-adds, for the reason written there: with one course the two kernels write the same bits
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  float* q = a.tg.base + kv_off(a.tg, i);
  const long long fs = a.tg.field_stride;
  const long long c = a.traj_id ? (long long)a.traj_id[i] : i;
  const int n_seg = (c >= 0 && c < a.K) ? a.n_seg[c] : 0;
  if (n_seg < 1 || n_seg > a.L_max - 1) {           // no such course, or one that could not be made: NaN, and nothing of the bank is read
    const double qnan = __builtin_nan("");
#pragma unroll
    for (int f = 0; f < DSIM_NT; ++f) q[f * fs] = __builtin_nanf("");
    a.yaw_state[i] = qnan; a.yaw_state[a.n_pad + i] = qnan; a.yaw_state[2 * a.n_pad + i] = qnan;
    a.t[i] += a.dt_advance;
    return;
  }
  const double* ts = a.ts + c;
  const double* coeffs = a.coeffs + c;
  double t = a.t[i];
  const double t_end = ts[(long long)n_seg * a.K_pad];
  if (t > t_end) t = t_end - 0.001;                                   // trajGen.py:110-111
  int seg = 0;
  for (int k = 0; k <= n_seg; ++k) if (t >= ts[(long long)k * a.K_pad]) seg = k;       // :113
  if (seg >= n_seg) seg = n_seg - 1;
  t -= ts[(long long)seg * a.K_pad];                                   // :115
  double pw[10];
  pw[0] = 1.0;
#pragma unroll
  for (int j = 1; j < 10; ++j) pw[j] = pw[j - 1] * t;
  double out[9];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    double p = 0.0, v = 0.0, ac = 0.0;
#pragma unroll
    for (int j = 0; j < 10; ++j) {                                     // coeff @ polyder(t, k), :118-120
      const double cf = coeffs[(long long)((seg * 10 + j) * 3 + d) * a.K_pad];
      p += cf * pw[j];
      if (j >= 1) v += cf * (double)j * pw[j - 1];
      if (j >= 2) ac += cf * (double)(j * (j - 1)) * pw[j - 2];
    }
    out[d] = p; out[3 + d] = v; out[6 + d] = ac;
  }
  // get_yaw(vel[:2]), :128-143 — per-drone memory (yaw, heading)
  double yaw = a.yaw_state[i];
  const double hx = a.yaw_state[a.n_pad + i], hy = a.yaw_state[2 * a.n_pad + i];
  const double nv = sqrt(out[3] * out[3] + out[4] * out[4]);
  const double cx = out[3] / nv, cy = out[4] / nv;
  const double cosine = fmax(-1.0, fmin(hx * cx + hy * cy, 1.0));
  const double dyaw = acos(cosine);
  const double cr = hx * cy - hy * cx;
  yaw += (cr > 0.0 ? 1.0 : (cr < 0.0 ? -1.0 : cr)) * dyaw;            // (np.sign keeps a NaN: see k_traj_sample)
  if (yaw > 3.14159265358979323846) yaw -= 2.0 * 3.14159265358979323846;
  if (yaw < -3.14159265358979323846) yaw += 2.0 * 3.14159265358979323846;
  a.yaw_state[i] = yaw; a.yaw_state[a.n_pad + i] = cx; a.yaw_state[2 * a.n_pad + i] = cy;
  a.t[i] += a.dt_advance;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    q[d * fs] = (float)out[d] + (a.offset ? a.offset[d * a.n_pad + i] : 0.0f);
    q[(3 + d) * fs] = (float)out[3 + d];
    q[(6 + d) * fs] = (float)out[6 + d];
  }
  q[9 * fs] = (float)yaw;
}

// ---- host side ----------------------------------------------------------------------------------------------------------
static bool traj_bank_ok(const dsim_traj_bank* b) {
  return b && b->coeffs && b->ts && b->n_seg && b->K >= 1 && b->K_pad >= b->K && (b->K_pad & 63) == 0 &&
         b->L_max >= 2 && b->L_max <= DSIM_TRAJGEN_LMAX;
}

extern "C" {

int64_t dsim_trajgen_workspace(int64_t K_pad, int32_t L_max) {
  if (K_pad <= 0 || L_max < 2 || L_max > DSIM_TRAJGEN_LMAX) return 0;
  return (int64_t)DSIM_TG_KEEP * (L_max - 2) * K_pad;
}

int dsim_trajgen(dsim_ctx* ctx, void* stream, const dsim_traj_bank* bank, const dsim_trajgen_args* args) {
  if (!ctx || !args || !traj_bank_ok(bank)) return DSIM_E_ARG;
  if (!args->wp || !args->n_wp || !args->cost || !args->evals || !args->status) return DSIM_E_ARG;
  if (!(args->max_vel > 0.0) || !isfinite(args->max_vel) || !isfinite(args->gamma)) return DSIM_E_ARG;
  if (args->mode != DSIM_TRAJGEN_GIVEN && args->mode != DSIM_TRAJGEN_TMIN && args->mode != DSIM_TRAJGEN_OPTIMIZE) return DSIM_E_ARG;
  if (args->max_evals < 1) return DSIM_E_ARG;
  if (args->mode == DSIM_TRAJGEN_OPTIMIZE && !(args->gamma > 0.0)) return DSIM_E_ARG;     // J has no minimum: T runs off to infinity
  const int64_t need = dsim_trajgen_workspace(bank->K_pad, bank->L_max);
  if (need > 0 && (!args->workspace || args->workspace_len < need)) return DSIM_E_ARG;
  TrajGenK a;
  a.wp = args->wp; a.n_wp = args->n_wp; a.coeffs = bank->coeffs; a.ts = bank->ts; a.n_seg = bank->n_seg;
  a.cost = args->cost; a.evals = args->evals; a.status = args->status; a.seg_times = args->seg_times; a.ws = need > 0 ? args->workspace : nullptr;
  a.K = bank->K; a.K_pad = bank->K_pad; a.L_max = bank->L_max; a.mode = args->mode; a.max_evals = args->max_evals;
  a.max_vel = args->max_vel; a.gamma = args->gamma;
  const unsigned grid = (unsigned)((bank->K + DSIM_TG_LANES - 1) / DSIM_TG_LANES);
  hipLaunchKernelGGL(k_trajgen, dim3(grid), dim3(DSIM_TG_LANES), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int dsim_traj_sample_bank(dsim_ctx* ctx, void* stream, int64_t n, const dsim_traj_bank* bank, const int32_t* traj_id,
                          double* t, double dt_advance, double* yaw_state, const float* offset, dsim_view targets_out) {
  if (!ctx || !traj_bank_ok(bank) || !t || !yaw_state || n <= 0 || n > targets_out.n_pad) return DSIM_E_ARG;
  if (!traj_id && bank->K < n) return DSIM_E_ARG;
  TrajBankK a;
  int rc = make_kview(targets_out, DSIM_NT, &a.tg);
  if (rc) return rc;
  a.coeffs = bank->coeffs; a.ts = bank->ts; a.n_seg = bank->n_seg; a.traj_id = traj_id;
  a.t = t; a.yaw_state = yaw_state; a.offset = offset;
  a.n = n; a.n_pad = targets_out.n_pad; a.K = bank->K; a.K_pad = bank->K_pad; a.L_max = bank->L_max; a.dt_advance = dt_advance;
  hipLaunchKernelGGL(k_traj_sample_bank, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

}  // extern "C"
