// Gate passage watch (dsim_gate_passage): which drones flew through the gates of their scene, in order (include/dronesim_amd.h).
// One aperture — a planar opening in the prototype's frame — per placement; the chord from the position the previous call saw to
// the current one is taken into each placement's frame and crossed with the aperture's plane.  Compiled as part of
// dsim_obstacles.hip, which includes it: it shares the watches' tile frame (256-drone tiles grid-stride, kv_off, obs_blocks), the
// scenes' placement table (struct dsim_scenes) and the swept watch's prime kernel (k_sweep_prime).  It needs no triangle records,
// no LDS and no cell walk.
#pragma once

// the aperture, wave-uniform: it travels by value in the kernel arguments and lives in SGPRs
struct GateAp {
  float cx, cy, cz, nx, ny, nz, ux, uy, uz, vx, vy, vz;   // v = n x u
  float a, b, inv_a, inv_b;                                // half-extents along u and v
  float ao, bo;                                            // the outer rectangle, 0: none
  int ellipse;
};

struct GateK {
  KView st;
  long long n, n_pad, tiles;
  const float* offset;           // SoA [3][n_pad] or null
  const float4* place;           // [K][G][4] (struct dsim_scenes)
  const int* scene_id;           // [n_pad]
  long long K;
  int G;
  GateAp ap;
  float r_ap;                    // from c_task of a slot, how far a crossing point inside the (outer) rectangle can lie; widened
  float travel2;                 // travel^2 (1 - 2^-20), as the swept drone-drone watch takes it
  float* prev;                   // SoA [3][n_pad], world frame
  int keep_prev, wrap;
  int* due;                      // [n_pad] in-out
  int* laps;                     // [n_pad] in-out (with wrap)
  const unsigned long long* clock;
  double* pass_time;             // [G][n_pad] or null
  unsigned* fwd;                 // [n_pad] each, or null
  unsigned* back;
  unsigned* miss;
  unsigned long long* passes;    // fleet counters, each nullable
  unsigned long long* wrong;
  unsigned long long* ooo;
  unsigned long long* misses;
  unsigned long long* unswept;
};

// What the chord q0 -> q1 does at the aperture of slot g: 0 nothing, 1 a forward crossing inside the aperture, 2 a backward
// crossing inside it, 3 a forward crossing outside it but inside the outer rectangle.  Both ends go into the placement's frame,
// subtract first, then rotate (k_obstacle_clearance_scenes); s0, s1 are the signed distances from the plane, half-open so that a
// state exactly on the plane is one crossing across two consecutive chords; tau = s0 / (s0 - s1) is in (0, 1] forward, [0, 1)
// backward, and the crossing point is taken relative to the aperture's centre: e = d0 + tau (d1 - d0) with d = l - c.
__device__ __forceinline__ int gate_eval(const float4* pl, int g, const GateAp& ap, float q0x, float q0y, float q0z, float q1x,
                                         float q1y, float q1z, float& tau) {
  const float4 c0 = pl[4 * g + 1], c1 = pl[4 * g + 2], c2 = pl[4 * g + 3];
  const float t0x = q0x - c0.w, t0y = q0y - c1.w, t0z = q0z - c2.w;
  const float t1x = q1x - c0.w, t1y = q1y - c1.w, t1z = q1z - c2.w;
  const float d0x = (c0.x * t0x + c0.y * t0y + c0.z * t0z) - ap.cx, d0y = (c1.x * t0x + c1.y * t0y + c1.z * t0z) - ap.cy,
              d0z = (c2.x * t0x + c2.y * t0y + c2.z * t0z) - ap.cz;
  const float d1x = (c0.x * t1x + c0.y * t1y + c0.z * t1z) - ap.cx, d1y = (c1.x * t1x + c1.y * t1y + c1.z * t1z) - ap.cy,
              d1z = (c2.x * t1x + c2.y * t1y + c2.z * t1z) - ap.cz;
  const float s0 = ap.nx * d0x + ap.ny * d0y + ap.nz * d0z, s1 = ap.nx * d1x + ap.ny * d1y + ap.nz * d1z;
  const bool fw = s0 < 0.0f && s1 >= 0.0f, bw = s0 >= 0.0f && s1 < 0.0f;
  tau = 0.0f;
  if (!fw && !bw) return 0;
  tau = s0 / (s0 - s1);
  const float ex = d0x + tau * (d1x - d0x), ey = d0y + tau * (d1y - d0y), ez = d0z + tau * (d1z - d0z);
  const float y = ap.ux * ex + ap.uy * ey + ap.uz * ez, z = ap.vx * ex + ap.vy * ey + ap.vz * ez;
  const float ya = y * ap.inv_a, zb = z * ap.inv_b;
  const bool in = ap.ellipse ? ya * ya + zb * zb <= 1.0f : (fabsf(y) <= ap.a && fabsf(z) <= ap.b);
  if (in) return fw ? 1 : 2;
  return fw && ap.ao > 0.0f && fabsf(y) <= ap.ao && fabsf(z) <= ap.bo ? 3 : 0;
}

__device__ __forceinline__ unsigned gate_wave_sum(unsigned v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// One drone per lane in the watches' tile frame.  Scene ids differ per lane, so the slot heads are per-lane vector loads, as in
// the placed clearance watch: 16 bytes per slot, and the other 48 only of a slot the chord can reach.  A lane whose chord
// reaches no slot reads neither its due gate nor the clock, and a wave with no event skips the sums: the far case is the
// position, prev read and written, the offset, the id, the slot heads and the masks.
// The due gate is evaluated on its own in the progress loop (no per-gate tau is kept: nothing here is indexed at run time).
__global__ __launch_bounds__(256) void k_gate_passage(GateK a) {
  unsigned n_pass = 0u, n_wrong = 0u, n_ooo = 0u, n_miss = 0u, n_uns = 0u;      // the wave's counts over its tiles
  for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const long long i = tile * 256 + threadIdx.x;
    const bool live = i < a.n;
    float q1x = 0.0f, q1y = 0.0f, q1z = 0.0f, q0x = 0.0f, q0y = 0.0f, q0z = 0.0f;
    int sid = -1;
    if (live) {
      const long long o = kv_off(a.st, i);
      const float px = a.st.base[o], py = a.st.base[o + a.st.field_stride], pz = a.st.base[o + 2 * a.st.field_stride];
      q0x = a.prev[i]; q0y = a.prev[a.n_pad + i]; q0z = a.prev[2 * a.n_pad + i];
      if (!a.keep_prev) { a.prev[i] = px; a.prev[a.n_pad + i] = py; a.prev[2 * a.n_pad + i] = pz; }
      q1x = px; q1y = py; q1z = pz;
      if (a.offset) {
        const float fx = a.offset[i], fy = a.offset[a.n_pad + i], fz = a.offset[2 * a.n_pad + i];
        q1x -= fx; q1y -= fy; q1z -= fz; q0x -= fx; q0y -= fy; q0z -= fz;
      }
      sid = a.scene_id[i];
    }
    const bool look = live && sid >= 0 && (long long)sid < a.K;      // (any other id: nothing of this drone is touched but prev)
    const float dx = q1x - q0x, dy = q1y - q0y, dz = q1z - q0z;
    const float len2 = dx * dx + dy * dy + dz * dz;
    const bool swept = len2 <= a.travel2;                            // (NaN or infinity on either end fails the comparison)
    // the slots the chord can reach, one bit each, and the scene's count: the used slots, which come first (r_cull = -inf above)
    unsigned reach = 0u;
    int cnt = 0;
    const float4* pl = a.place;
    if (look && swept) {
      pl += 4 * ((size_t)sid * (size_t)a.G);
      const float b = (a.r_ap + DSIM_SQRT(len2)) * 1.0001f + 1e-5f;
      for (int g = 0; g < a.G; ++g) {
        const float4 w = pl[4 * g];
        const float ux = q1x - w.x, uy = q1y - w.y, uz = q1z - w.z;
        const bool used = w.w >= 0.0f;
        cnt += used ? 1 : 0;
        reach |= (used && ux * ux + uy * uy + uz * uz <= b * b) ? (1u << g) : 0u;
      }
    }
    unsigned fwd = 0u, back = 0u, miss = 0u;
    while (reach != 0u) {                  // (a wave with no such lane skips the loop: the per-wave reject)
      const int g = __ffs((int)reach) - 1;
      reach &= reach - 1u;
      float tau;
      const int kind = gate_eval(pl, g, a.ap, q0x, q0y, q0z, q1x, q1y, q1z, tau);
      fwd |= kind == 1 ? (1u << g) : 0u;
      back |= kind == 2 ? (1u << g) : 0u;
      miss |= kind == 3 ? (1u << g) : 0u;
    }
    // progress: the due gate, while it was crossed forward inside its aperture later along the chord than the one before it
    unsigned adv = 0u;
    bool miss_due = false;
    if ((fwd | miss) != 0u) {
      int due = a.due[i], wrapped = 0;
      float last = -1.0f;
      const unsigned long long clk = a.clock ? *a.clock : 0ULL;
      for (int it = 0; it < cnt; ++it) {
        if (due < 0 || due >= cnt || ((fwd >> due) & 1u) == 0u) break;
        float tau;
        (void)gate_eval(pl, due, a.ap, q0x, q0y, q0z, q1x, q1y, q1z, tau);
        if (!(tau > last)) break;
        last = tau;
        if (a.pass_time && !a.keep_prev) a.pass_time[(size_t)due * (size_t)a.n_pad + (size_t)i] = (double)clk + (double)tau;
        ++adv;
        ++due;
        if (due == cnt && a.wrap) { due = 0; ++wrapped; }
      }
      if (adv != 0u && !a.keep_prev) a.due[i] = due;        // (KEEP_PREV: a look ahead, the course stays where it is)
      if (wrapped != 0 && !a.keep_prev) a.laps[i] += wrapped;
      miss_due = due >= 0 && due < cnt && ((miss >> due) & 1u) != 0u;
    }
    if (look) {
      if (a.fwd) a.fwd[i] = fwd;
      if (a.back) a.back[i] = back;
      if (a.miss) a.miss[i] = miss;
    }
    // the fleet counters: one ballot for "anything at all", then one sum per counter, kept by the wave across its tiles
    const bool uns = look && !swept;
    if (__ballot((fwd | back | miss) != 0u || uns) != 0ULL) {
      n_pass += gate_wave_sum(adv);
      n_wrong += gate_wave_sum((unsigned)__popc(back));
      n_ooo += gate_wave_sum((unsigned)__popc(fwd) - adv);
      n_miss += (unsigned)__popcll(__ballot(miss_due));
      n_uns += (unsigned)__popcll(__ballot(uns));
    }
  }
  // one atomic per wave and counter at the most, behind the wave's last tile: near a gate nearly every wave has an event, and the
  // atomics of 65 536 waves on five addresses would be what the query waits for
  if ((threadIdx.x & 63u) == 0u) {
    if (a.passes && n_pass) atomicAdd(a.passes, (unsigned long long)n_pass);
    if (a.wrong && n_wrong) atomicAdd(a.wrong, (unsigned long long)n_wrong);
    if (a.ooo && n_ooo) atomicAdd(a.ooo, (unsigned long long)n_ooo);
    if (a.misses && n_miss) atomicAdd(a.misses, (unsigned long long)n_miss);
    if (a.unswept && n_uns) atomicAdd(a.unswept, (unsigned long long)n_uns);
  }
}

// the aperture as the kernel takes it, or false for one the call refuses
static bool gate_aperture(const dsim_aperture& p, GateAp* out) {
  const float* f = p.center;                                   // (center, normal, u, half, outer: 13 floats in a row)
  for (int k = 0; k < 13; ++k) if (!isfinite(f[k])) return false;
  if (p.shape != DSIM_APERTURE_RECT && p.shape != DSIM_APERTURE_ELLIPSE) return false;
  const double n[3] = {p.normal[0], p.normal[1], p.normal[2]}, u[3] = {p.u[0], p.u[1], p.u[2]};
  const double nn = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]), uu = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  const double nu = n[0] * u[0] + n[1] * u[1] + n[2] * u[2];
  if (!(fabs(nn - 1.0) <= 1e-5) || !(fabs(uu - 1.0) <= 1e-5) || !(fabs(nu) <= 1e-5)) return false;
  if (!(p.half[0] > 0.0f) || !(p.half[1] > 0.0f)) return false;
  const bool outer = p.outer[0] != 0.0f || p.outer[1] != 0.0f;
  if (outer && (!(p.outer[0] >= p.half[0]) || !(p.outer[1] >= p.half[1]))) return false;
  GateAp& g = *out;
  g.cx = p.center[0]; g.cy = p.center[1]; g.cz = p.center[2];
  g.nx = p.normal[0]; g.ny = p.normal[1]; g.nz = p.normal[2];
  g.ux = p.u[0]; g.uy = p.u[1]; g.uz = p.u[2];
  g.vx = (float)(n[1] * u[2] - n[2] * u[1]); g.vy = (float)(n[2] * u[0] - n[0] * u[2]); g.vz = (float)(n[0] * u[1] - n[1] * u[0]);
  g.a = p.half[0]; g.b = p.half[1]; g.inv_a = 1.0f / p.half[0]; g.inv_b = 1.0f / p.half[1];
  g.ao = p.outer[0]; g.bo = p.outer[1];
  g.ellipse = p.shape == DSIM_APERTURE_ELLIPSE ? 1 : 0;
  return true;
}

extern "C" int dsim_gate_passage(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_scenes* scenes,
                                 const int32_t* scene_id, const dsim_gate_args* args) {
  if (!ctx || !args || !args->prev || n <= 0 || n > state.n_pad) return DSIM_E_ARG;
  const int32_t fl = args->flags;
  if ((fl & ~(DSIM_SWEEP_KEEP_PREV | DSIM_SWEEP_PRIME | DSIM_GATE_WRAP)) ||
      (fl & (DSIM_SWEEP_KEEP_PREV | DSIM_SWEEP_PRIME)) == (DSIM_SWEEP_KEEP_PREV | DSIM_SWEEP_PRIME))
    return DSIM_E_ARG;
  const hipStream_t st_ = (hipStream_t)stream;
  if (fl & DSIM_SWEEP_PRIME) {
    SweepK w;
    memset(&w, 0, sizeof(w));
    const int rc = make_kview(state, 3, &w.o.st);
    if (rc) return rc;
    w.o.n = n; w.o.n_pad = state.n_pad; w.o.tiles = (n + 255) / 256; w.prev = args->prev;
    hipLaunchKernelGGL(k_sweep_prime, dim3(obs_blocks(w.o.tiles)), dim3(256), 0, st_, w);
    return (int)hipGetLastError();
  }
  if (!scenes || !scene_id || !args->due || ((fl & DSIM_GATE_WRAP) && !args->laps)) return DSIM_E_ARG;
  if (!(args->travel > 0.0f) || !isfinite(args->travel)) return DSIM_E_ARG;
  GateK a;
  memset(&a, 0, sizeof(a));
  if (!gate_aperture(args->aperture, &a.ap)) return DSIM_E_ARG;
  const int rc = make_kview(state, 3, &a.st);
  if (rc) return rc;
  a.n = n; a.n_pad = state.n_pad; a.tiles = (n + 255) / 256;
  a.offset = args->offset; a.place = scenes->place; a.scene_id = scene_id; a.K = scenes->K; a.G = scenes->G;
  // A crossing point inside the outer rectangle (the aperture without one) lies within half its diagonal of the aperture's
  // centre, which lies |c - box centre| from the point c_task is the image of; widened as dsim_scenes_create widens its radius
  // (1e-4 relative, and what an R that is orthonormal to 1e-5 only can move a centre by).  It decides speed only.
  const dsim_aperture& p = args->aperture;
  const bool outer = p.outer[0] != 0.0f || p.outer[1] != 0.0f;
  const double ea = outer ? p.outer[0] : p.half[0], eb = outer ? p.outer[1] : p.half[1];
  double dc = 0.0, cn = 0.0;
  for (int k = 0; k < 3; ++k) {
    const double d = (double)p.center[k] - (double)scenes->box_c[k];
    dc += d * d;
    cn += (double)p.center[k] * p.center[k] + (double)scenes->box_c[k] * scenes->box_c[k];
  }
  a.r_ap = nextafterf((float)((sqrt(dc) + sqrt(ea * ea + eb * eb)) * (1.0 + 1e-4) + 4e-5 * sqrt(cn) + 1e-5), INFINITY);
  // 2^-20 below travel^2: the squared length is three products and two sums in fp32, 2^-22 of it at the most
  a.travel2 = (float)((double)args->travel * (double)args->travel * (1.0 - 1.0 / 1048576.0));
  a.prev = args->prev; a.keep_prev = (fl & DSIM_SWEEP_KEEP_PREV) ? 1 : 0; a.wrap = (fl & DSIM_GATE_WRAP) ? 1 : 0;
  a.due = args->due; a.laps = args->laps; a.clock = (const unsigned long long*)args->clock; a.pass_time = args->pass_time;
  a.fwd = args->fwd_out; a.back = args->back_out; a.miss = args->miss_out;
  a.passes = (unsigned long long*)args->passes_out; a.wrong = (unsigned long long*)args->wrong_way_out;
  a.ooo = (unsigned long long*)args->out_of_order_out; a.misses = (unsigned long long*)args->misses_out;
  a.unswept = (unsigned long long*)args->unswept_out;
  hipLaunchKernelGGL(k_gate_passage, dim3(obs_blocks(a.tiles)), dim3(256), 0, st_, a);
  return (int)hipGetLastError();
}
