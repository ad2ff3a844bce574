// dsim_traj.hip — the trajectory bank: dsim_trajgen (K min-snap courses in one launch, trajGen.py:13-106) and
// dsim_traj_sample_bank (k_traj_sample with a course per drone).  Compiled as part of dsim_api.hip, which includes it.
#include "dsim_trajgen_tables.h"

// ---- generator ------------------------------------------------------------------------------------------------------
// One lane per course.  The only per-lane arrays indexed at run time are the segment times, their lower bounds and the
// position steps: they live in LDS, one column per lane (a lane touches its own column only: no barrier anywhere).  The
// 4 x 4 blocks of the solve are indexed by unrolled loops and stay in registers; what the sweep back needs of the sweep
// along (per interior waypoint the Cholesky factor of its block, 10, and z = L^-1 w for three axes, 12) goes through the
// caller's workspace, course-minor like the bank.
#define DSIM_TG_LANES 64
#define DSIM_TG_SEGS (DSIM_TRAJGEN_LMAX - 1)
#define DSIM_TG_KEEP 22
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

__device__ __forceinline__ constexpr int tg_sym(int r, int c) { return r >= c ? r * (r + 1) / 2 + c : c * (c + 1) / 2 + r; }

// T, T^2, T^3, T^4 in u; g = u / T^7; returns 1 / T^7
__device__ __forceinline__ double tg_scales(double T, double u[4], double g[4]) {
  u[0] = T; u[1] = T * T; u[2] = u[1] * T; u[3] = u[1] * u[1];
  const double i7 = 1.0 / (u[3] * u[2]);
#pragma unroll
  for (int r = 0; r < 4; ++r) g[r] = u[r] * i7;
  return i7;
}

// the sweep along the course: the snap cost at the best interior derivatives.  sT, sD: this lane's LDS columns; segment
// ci takes the time cv instead of its stored one (ci = -1: none).  KEEP: ws (already at this course) receives the factors.
template <bool KEEP>
__device__ __forceinline__ double tg_sweep(int n, const double* sT, int ci, double cv, const double* sD, double* ws, long long K_pad) {
  double P[10], q[3][4], c;
  for (int m = 0; m < n; ++m) {
    const double T = (m == ci) ? cv : sT[m * DSIM_TG_LANES];
    double u[4], g[4], d[3];
    const double i7 = tg_scales(T, u, g);
#pragma unroll
    for (int x = 0; x < 3; ++x) d[x] = sD[(m * 3 + x) * DSIM_TG_LANES];
    const double dd = DSIM_TG_M[5][5] * i7 * (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    if (m == 0) {                                  // at rest at the start: the cost so far is the segment's own, in its end derivatives
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int s = 0; s <= r; ++s) P[tg_sym(r, s)] = DSIM_TG_M[6 + r][6 + s] * g[r] * u[s];
#pragma unroll
        for (int x = 0; x < 3; ++x) q[x][r] = DSIM_TG_M[6 + r][5] * g[r] * d[x];
      }
      c = dd;
      continue;
    }
    // S = P + K_aa = L L^T
    double L[10], Li[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int s = 0; s <= r; ++s) L[tg_sym(r, s)] = P[tg_sym(r, s)] + DSIM_TG_M[1 + r][1 + s] * g[r] * u[s];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double s = L[tg_sym(j, j)];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= L[tg_sym(j, k)] * L[tg_sym(j, k)];
      s = sqrt(s);
      L[tg_sym(j, j)] = s;
      Li[j] = 1.0 / s;
#pragma unroll
      for (int i = j + 1; i < 4; ++i) {
        double t = L[tg_sym(i, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) t -= L[tg_sym(i, k)] * L[tg_sym(j, k)];
        L[tg_sym(i, j)] = t * Li[j];
      }
    }
    // z = L^-1 (q + K_ad d) per axis; the cost drops by |z|^2
    double z[3][4];
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double t = q[x][r] + DSIM_TG_M[1 + r][5] * g[r] * d[x];
#pragma unroll
        for (int k = 0; k < r; ++k) t -= L[tg_sym(r, k)] * z[x][k];
        z[x][r] = t * Li[r];
      }
    double zz = 0.0;
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
      for (int r = 0; r < 4; ++r) zz += z[x][r] * z[x][r];
    c += dd - zz;
    if (KEEP) {
      double* w = ws + (long long)(m - 1) * DSIM_TG_KEEP * K_pad;
#pragma unroll
      for (int e = 0; e < 10; ++e) w[e * K_pad] = L[e];
#pragma unroll
      for (int x = 0; x < 3; ++x)
#pragma unroll
        for (int r = 0; r < 4; ++r) w[(10 + x * 4 + r) * K_pad] = z[x][r];
    }
    // Y = L^-1 K_ab; P' = K_bb - Y^T Y; q' = K_bd d - Y^T z
    double Y[4][4];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double t = DSIM_TG_M[1 + r][6 + s] * g[r] * u[s];
#pragma unroll
        for (int k = 0; k < r; ++k) t -= L[tg_sym(r, k)] * Y[k][s];
        Y[r][s] = t * Li[r];
      }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int s = 0; s <= r; ++s) {
        double t = DSIM_TG_M[6 + r][6 + s] * g[r] * u[s];
#pragma unroll
        for (int k = 0; k < 4; ++k) t -= Y[k][r] * Y[k][s];
        P[tg_sym(r, s)] = t;
      }
#pragma unroll
      for (int x = 0; x < 3; ++x) {
        double t = DSIM_TG_M[6 + r][5] * g[r] * d[x];
#pragma unroll
        for (int k = 0; k < 4; ++k) t -= Y[k][r] * z[x][k];
        q[x][r] = t;
      }
    }
  }
  return c;
}

// the sweep back: interior derivatives from the kept factors, then every segment's ten coefficients per axis and its cost
__device__ __forceinline__ double tg_back(int n, const double* sT, const double* sD, const double* ws, long long K_pad,
                                          const double* wp, double* coeffs) {
  double b[3][4], cost = 0.0;
#pragma unroll
  for (int x = 0; x < 3; ++x)
#pragma unroll
    for (int r = 0; r < 4; ++r) b[x][r] = 0.0;                     // at rest at the end
  for (int m = n - 1; m >= 0; --m) {
    const double T = sT[m * DSIM_TG_LANES];
    double u[4], g[4], a[3][4];
    const double i7 = tg_scales(T, u, g);
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
      for (int r = 0; r < 4; ++r) a[x][r] = 0.0;                   // at rest at the start
    if (m >= 1) {                                                   // a = -L^-T (z + L^-1 K_ab b)
      const double* w = ws + (long long)(m - 1) * DSIM_TG_KEEP * K_pad;
      double L[10], Li[4];
#pragma unroll
      for (int e = 0; e < 10; ++e) L[e] = w[e * K_pad];
#pragma unroll
      for (int r = 0; r < 4; ++r) Li[r] = 1.0 / L[tg_sym(r, r)];
#pragma unroll
      for (int x = 0; x < 3; ++x) {
        double y[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          double t = 0.0;
#pragma unroll
          for (int s = 0; s < 4; ++s) t += DSIM_TG_M[1 + r][6 + s] * g[r] * u[s] * b[x][s];
#pragma unroll
          for (int k = 0; k < r; ++k) t -= L[tg_sym(r, k)] * y[k];
          y[r] = t * Li[r];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) y[r] += w[(10 + x * 4 + r) * K_pad];
#pragma unroll
        for (int r = 3; r >= 0; --r) {
          double t = y[r];
#pragma unroll
          for (int k = r + 1; k < 4; ++k) t -= L[tg_sym(k, r)] * a[x][k];
          a[x][r] = t * Li[r];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) a[x][r] = -a[x][r];
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
      for (int r = 1; r < 10; ++r) {
        double t = 0.0;
#pragma unroll
        for (int s = 1; s < 10; ++s) t += DSIM_TG_M[r][s] * e[s];
        en += e[r] * t;
      }
      cost += en * i7;
      coeffs[((long long)(m * 10) * 3 + x) * K_pad] = wp[(long long)(m * 3 + x) * K_pad];
#pragma unroll
      for (int j = 1; j < 10; ++j) {
        double t = 0.0;
#pragma unroll
        for (int s = 1; s < 10; ++s) t += DSIM_TG_AINV[j][s] * e[s];
        coeffs[((long long)(m * 10 + j) * 3 + x) * K_pad] = t * ip[j];
      }
    }
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
      for (int r = 0; r < 4; ++r) b[x][r] = a[x][r];
  }
  return cost;
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
  if (bad) {                                        // this course only: NaN everywhere, n_seg 0
    for (int e = 0; e < (a.L_max - 1) * 30; ++e) coeffs[(long long)e * a.K_pad] = qnan;
    for (int l = 0; l < a.L_max; ++l) ts[(long long)l * a.K_pad] = qnan;
    if (a.seg_times) for (int m = 0; m < a.L_max - 1; ++m) a.seg_times[(long long)m * a.K_pad + k] = qnan;
    a.cost[k] = qnan; a.evals[k] = 0; a.status[k] = bad; a.n_seg[k] = 0;
    return;
  }
  int evals = 0;
  if (a.mode == DSIM_TRAJGEN_OPTIMIZE) {
    // greedy multiplicative pattern search (include/dronesim_amd.h); one pass of the loop is at most one evaluation, so lanes
    // at different points of their own searches still share the sweep's instructions
    double sum = 0.0;
    for (int m = 0; m < n; ++m) sum += sT[m * DSIM_TG_LANES];
    double Jx = tg_sweep<false>(n, sT, -1, 0.0, sD, nullptr, 0) + a.gamma * sum;
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
        const double Jy = tg_sweep<false>(n, sT, i, yi, sD, nullptr, 0) + a.gamma * sum;
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
  if (a.mode != DSIM_TRAJGEN_GIVEN) {               // TS[1:] = cumsum(T), trajGen.py:42
    double acc = 0.0;
    ts[0] = 0.0;
    for (int m = 0; m < n; ++m) { acc += sT[m * DSIM_TG_LANES]; ts[(long long)(m + 1) * a.K_pad] = acc; }
  }
  for (int l = n + 1; l < a.L_max; ++l) ts[(long long)l * a.K_pad] = qnan;
  if (a.seg_times) for (int m = 0; m < a.L_max - 1; ++m) a.seg_times[(long long)m * a.K_pad + k] = m < n ? sT[m * DSIM_TG_LANES] : qnan;
  double* ws = a.ws ? a.ws + k : nullptr;           // (null only at L_max = 2, where no course has an interior waypoint)
  tg_sweep<true>(n, sT, -1, 0.0, sD, ws, a.K_pad);
  const double cost = tg_back(n, sT, sD, ws, a.K_pad, wp, coeffs);
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
