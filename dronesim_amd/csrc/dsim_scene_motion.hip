// Moving obstacle scenes (dsim_scenes_motion_set, dsim_scenes_move, dsim_scenes_move_twist, dsim_scenes_read): per-placement motion of the scenes' table,
// evaluated on the device in stream order.  Every placed kernel reads the [K][G] table of 64-byte records from device memory on
// every launch (ScnK.place), so rewriting a record moves that placement for the watch, the witness, the camera, the scanner and
// line of sight at once: none of them changes.  Compiled as part of dsim_obstacles.hip, which includes this file behind
// dsim_scenes.hip: it shares dsim_scenes and the record's layout (c_task, r_cull; R's columns, each followed by a component of t).
//
// The law, at scene time tau = t_start + dt * (*clock), for a placement with base pose (R0, t0):
//     s = sin(omega tau + phase),  t = t0 + vel tau + amp s,  theta = rate tau + swing s,  R = Rot(axis, theta) R0  (Rodrigues)
// in double from the floats of the record and of the base table, rounded to float once: a float phase at a clock of 2^33 would be
// wrong by radians, and the result can be checked against an fp64 restatement to an ulp of float.
// Its derivative, off the same sincos (dsim_scenes_move_twist: the placement's twist, for the velocity of a witness on it):
//     t' = vel + amp omega cos(omega tau + phase),  theta' = rate + swing omega cos(omega tau + phase),  w = theta' axis
#pragma once

#define SCM_BLOCK 256
#define SCM_MAX_BLOCKS 2048     // as OBS_MAX_BLOCKS: a sweep of the grid covers 524 288 slots, the stride the rest

// One slot of the motion table as the kernel reads it: the 13 floats of dsim_scene_motion, then in the padding the `moving` flag
// and the slot's r_cull, so that a lane reads nothing of the record it is about to write.
//   m0 = (vel.xyz, amp.x)  m1 = (amp.yz, omega, phase)  m2 = (axis.xyz, rate)  m3 = (swing, moving ? 1 : 0, r_cull, 0)
struct ScmK {
  const float4* motion;          // [slots][4]
  const float4* base;            // [slots][4]: the table as dsim_scenes_create wrote it
  float4* place;                 // [slots][4]: the live table
  float4* twist;                 // [slots][2] or null: (t'.xyz, 0), (w.xyz, 0) of the moving slots (dsim_scenes_move_twist)
  const unsigned long long* clock;
  long long slots;
  double dt, t_start;
  float bx, by, bz;              // the centre of the prototype's box in its own frame
};

// The record of moving slot i at scene time tau, from its motion record (m3 is its last quarter, which the caller read for the
// flag) and its base pose: o0 = (c_task, r_cull), o1 .. o3 = R's columns, each followed by a component of t.  And its twist at
// that time, w0 = (t', 0), w1 = (theta' axis, 0): the derivative of the law, a few multiplies on the first sincos's cosine.
__device__ __forceinline__ void scm_record(const ScmK& a, long long i, double tau, const float4 m3, float4& o0, float4& o1, float4& o2,
                                           float4& o3, float4& w0, float4& w1) {
  const float4 m0 = a.motion[4 * i], m1 = a.motion[4 * i + 1], m2 = a.motion[4 * i + 2];
  const float4 c0 = a.base[4 * i + 1], c1 = a.base[4 * i + 2], c2 = a.base[4 * i + 3];
  double s, c;
  sincos((double)m1.z * tau + (double)m1.w, &s, &c);
  const double tx = (double)c0.w + (double)m0.x * tau + (double)m0.w * s;
  const double ty = (double)c1.w + (double)m0.y * tau + (double)m1.x * s;
  const double tz = (double)c2.w + (double)m0.z * tau + (double)m1.y * s;
  double st, ct;
  sincos((double)m2.w * tau + (double)m3.x * s, &st, &ct);
  // Rodrigues: Rot v = v cos + (k x v) sin + k (k . v) (1 - cos), column by column of R0 (column j is (cj.x, cj.y, cj.z))
  const double kx = m2.x, ky = m2.y, kz = m2.z, vc = 1.0 - ct;
  if (a.twist) {                         // (the launch's: a plain move evaluates nothing of it)
    const double oc = (double)m1.z * c, thd = (double)m2.w + (double)m3.x * oc;
    w0 = make_float4((float)((double)m0.x + (double)m0.w * oc), (float)((double)m0.y + (double)m1.x * oc),
                     (float)((double)m0.z + (double)m1.y * oc), 0.0f);
    w1 = make_float4((float)(thd * kx), (float)(thd * ky), (float)(thd * kz), 0.0f);
  }
  double r[3][3];
  const float4 col[3] = {c0, c1, c2};
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double vx = col[j].x, vy = col[j].y, vz = col[j].z;
    const double kv = (kx * vx + ky * vy + kz * vz) * vc;
    r[j][0] = vx * ct + (ky * vz - kz * vy) * st + kx * kv;
    r[j][1] = vy * ct + (kz * vx - kx * vz) * st + ky * kv;
    r[j][2] = vz * ct + (kx * vy - ky * vx) * st + kz * kv;
  }
  // c_task = R box_c + t: row k of R is (r[0][k], r[1][k], r[2][k])
  const double bx = a.bx, by = a.by, bz = a.bz;
  o0 = make_float4((float)(r[0][0] * bx + r[1][0] * by + r[2][0] * bz + tx), (float)(r[0][1] * bx + r[1][1] * by + r[2][1] * bz + ty),
                   (float)(r[0][2] * bx + r[1][2] * by + r[2][2] * bz + tz), m3.z);
  o1 = make_float4((float)r[0][0], (float)r[0][1], (float)r[0][2], (float)tx);
  o2 = make_float4((float)r[1][0], (float)r[1][1], (float)r[1][2], (float)ty);
  o3 = make_float4((float)r[2][0], (float)r[2][1], (float)r[2][2], (float)tz);
}

// One lane per slot, a block per 256 consecutive slots, grid-stride.  A lane reads its motion record (64 bytes; the flag first: a
// static or unused slot ends there with 16 bytes read) and the base pose (the last 48 bytes of the base record), and owns the 64
// bytes of its record.  The records go through LDS and are stored transposed: store instruction j of lane t writes quarter
// 256 j + t of the block's 16 KiB, so each store instruction of a wave covers 1 KiB of contiguous table, where four 16-byte stores
// per lane straight from its registers leave every instruction of a wave strided by 64 bytes.  Only the quarters of moving slots
// are written.  Measured against that direct form and against a per-block choice between the two: DESIGN.md section 7.
// With a twist table (dsim_scenes_move_twist) a moving lane also stores the two quarters of its twist, straight from its
// registers: 32 contiguous bytes per lane, so the two store instructions of a wave cover 2 KiB between them.  Measured against
// the same two quarters through an LDS transpose of their own (8 KiB more): within 3 % in every case.
// LDS holds quarter q of lane t at float4 index 4 t + (q ^ (t & 3)): a lane's four writes and a wave's transposed reads both spread
// over the 16-byte slots of a bank row.
__global__ __launch_bounds__(SCM_BLOCK) void k_scenes_move(ScmK a) {
  __shared__ float4 s_out[SCM_BLOCK * 4];
  __shared__ int s_mv[SCM_BLOCK];
  const double tau = a.t_start + a.dt * (double)(a.clock ? *a.clock : 0ULL);
  const int tid = threadIdx.x, x = tid & 3;
  for (long long base = (long long)blockIdx.x * SCM_BLOCK; base < a.slots; base += (long long)gridDim.x * SCM_BLOCK) {
    const long long i = base + tid;
    bool mv = false;
    if (i < a.slots) {
      const float4 m3 = a.motion[4 * i + 3];
      if (m3.y != 0.0f) {
        mv = true;
        float4 o0, o1, o2, o3, w0 = {}, w1 = {};
        scm_record(a, i, tau, m3, o0, o1, o2, o3, w0, w1);
        if (a.twist) { a.twist[2 * i] = w0; a.twist[2 * i + 1] = w1; }
        s_out[4 * tid + x] = o0; s_out[4 * tid + (1 ^ x)] = o1; s_out[4 * tid + (2 ^ x)] = o2; s_out[4 * tid + (3 ^ x)] = o3;
      }
    }
    s_mv[tid] = mv ? 1 : 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = j * SCM_BLOCK + tid, t = e >> 2, q = e & 3;       // quarter q of slot base + t (a slot at or above `slots` does not move)
      if (s_mv[t]) a.place[4 * base + e] = s_out[4 * t + (q ^ (t & 3))];
    }
    __syncthreads();                                                  // (before the next turn writes LDS again)
  }
}

static void scm_free(dsim_scenes* sc, hipError_t* e) {
  if (sc->motion) { const hipError_t f = hipFree(sc->motion); if (*e == hipSuccess) *e = f; }
  if (sc->base) { const hipError_t f = hipFree(sc->base); if (*e == hipSuccess) *e = f; }
  sc->motion = sc->base = nullptr;
}

// both moves: the one kernel, with the twist table or without
static int scm_move(dsim_ctx* ctx, void* stream, dsim_scenes* scenes, const uint64_t* clock, double dt, double t_start, float* twist) {
  if (!ctx || !scenes || !scenes->motion || !isfinite(dt) || !isfinite(t_start)) return DSIM_E_ARG;
  ScmK a;
  a.motion = scenes->motion; a.base = scenes->base; a.place = scenes->place; a.clock = (const unsigned long long*)clock;
  a.twist = (float4*)twist;
  a.slots = scenes->K * (long long)scenes->G; a.dt = dt; a.t_start = t_start;
  a.bx = scenes->box_c[0]; a.by = scenes->box_c[1]; a.bz = scenes->box_c[2];
  long long blocks = (a.slots + SCM_BLOCK - 1) / SCM_BLOCK;
  if (blocks > SCM_MAX_BLOCKS) blocks = SCM_MAX_BLOCKS;
  hipLaunchKernelGGL(k_scenes_move, dim3((unsigned)blocks), dim3(SCM_BLOCK), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

extern "C" {

int dsim_scenes_motion_set(dsim_ctx* ctx, dsim_scenes* scenes, const dsim_scene_motion* motion_host) {
  if (!ctx || !scenes) return DSIM_E_ARG;
  const size_t slots = (size_t)scenes->K * (size_t)scenes->G, bytes = slots * 64;
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return (int)e;
  if (!motion_host) {                                   // detach: the base table back, bit for bit
    if (!scenes->motion) return DSIM_OK;
    e = hipDeviceSynchronize();                         // (a move in flight on any stream lands before the table is put back)
    if (e == hipSuccess) e = hipMemcpy(scenes->place, scenes->base, bytes, hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    scm_free(scenes, &e);
    return (int)e;
  }
  // the base table: the kept copy, or on the first call the table itself, which nothing has moved yet
  std::vector<float> base, rec;
  try { base.resize(slots * 16); rec.assign(slots * 16, 0.0f); } catch (const std::bad_alloc&) { return (int)hipErrorOutOfMemory; }
  e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(base.data(), scenes->motion ? scenes->base : scenes->place, bytes, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return (int)e;
  for (size_t i = 0; i < slots; ++i) {
    const float r_cull = base[16 * i + 3];
    if (r_cull == -INFINITY) continue;                  // a slot at or above its scene's count: the host's entry is not looked at
    const dsim_scene_motion& m = motion_host[i];
    const float* f = m.vel;                             // the 13 floats, in the struct's order
    bool any = false;
    for (int k = 0; k < 13; ++k) {
      if (!isfinite(f[k])) return DSIM_E_ARG;
      any = any || f[k] != 0.0f;
    }
    const double n2 = (double)m.axis[0] * m.axis[0] + (double)m.axis[1] * m.axis[1] + (double)m.axis[2] * m.axis[2];
    if (n2 == 0.0) { if (m.rate != 0.0f || m.swing != 0.0f) return DSIM_E_ARG; }
    else if (!(fabs(sqrt(n2) - 1.0) <= 1e-5)) return DSIM_E_ARG;
    float* r = rec.data() + 16 * i;
    for (int k = 0; k < 13; ++k) r[k] = f[k];
    r[13] = any ? 1.0f : 0.0f;
    r[14] = r_cull;
  }
  float4 *d_motion = nullptr, *d_base = nullptr;
  if (!scenes->motion) {
    e = hipMalloc((void**)&d_motion, bytes);
    if (e == hipSuccess) e = hipMalloc((void**)&d_base, bytes);
    if (e == hipSuccess) e = hipMemcpy(d_base, scenes->place, bytes, hipMemcpyDeviceToDevice);
    if (e != hipSuccess) { (void)hipFree(d_motion); (void)hipFree(d_base); return (int)e; }
    scenes->motion = d_motion; scenes->base = d_base;
  } else {
    // a new motion starts from the base table: what the old one moved and the new one leaves alone must not stay where it was
    e = hipMemcpy(scenes->place, scenes->base, bytes, hipMemcpyDeviceToDevice);
    if (e != hipSuccess) return (int)e;
  }
  e = hipMemcpy(scenes->motion, rec.data(), bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  return (int)e;
}

int dsim_scenes_move(dsim_ctx* ctx, void* stream, dsim_scenes* scenes, const uint64_t* clock, double dt, double t_start) {
  return scm_move(ctx, stream, scenes, clock, dt, t_start, nullptr);
}

int dsim_scenes_move_twist(dsim_ctx* ctx, void* stream, dsim_scenes* scenes, const uint64_t* clock, double dt, double t_start,
                           float* twist_out) {
  if (!twist_out) return DSIM_E_ARG;
  return scm_move(ctx, stream, scenes, clock, dt, t_start, twist_out);
}

int dsim_scenes_read(dsim_ctx* ctx, void* stream, const dsim_scenes* scenes, float* place_host_out) {
  if (!ctx || !scenes || !place_host_out) return DSIM_E_ARG;
  const size_t slots = (size_t)scenes->K * (size_t)scenes->G;
  std::vector<float> rec;
  try { rec.resize(slots * 16); } catch (const std::bad_alloc&) { return (int)hipErrorOutOfMemory; }
  hipError_t e = hipSetDevice(ctx->device);
  if (e == hipSuccess) e = hipMemcpyAsync(rec.data(), scenes->place, slots * 64, hipMemcpyDeviceToHost, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  for (size_t i = 0; i < slots; ++i) {
    const float* r = rec.data() + 16 * i;
    float* p = place_host_out + 12 * i;
    if (r[3] == -INFINITY) { for (int k = 0; k < 12; ++k) p[k] = NAN; continue; }
    for (int col = 0; col < 3; ++col) {                 // column `col` of R, then t[col]: back to R row-major, then t
      p[col] = r[4 + 4 * col]; p[3 + col] = r[5 + 4 * col]; p[6 + col] = r[6 + 4 * col]; p[9 + col] = r[7 + 4 * col];
    }
  }
  return DSIM_OK;
}

}  // extern "C"
