// Range scanner (dsim_range_scan): a fan of range beams per drone, for EVERY drone, against the obstacle set's ray grid (or the
// placements of the drone's scene), the plane z = 0 and the other drones as their bounding spheres (include/dronesim_amd.h has
// the ray).  The camera's kernel maps a workgroup onto a 16 x 16 pixel block of ONE camera and keeps the pose in scalar registers:
// at 8 .. 64 rays per drone that is 256 lanes for at most 64 rays and one pose read per workgroup.  Here the mapping is the
// watches': one drone per lane, tiles of 256 walked grid-stride, the pose loaded coalesced once, the lane loops over the beams.
// Compiled as part of dsim_obstacles.hip, which includes this file: it reads the set's and the scenes' private records and uses
// what dsim_camera.hip states for both sensors: the ray grid's record, the triangle walk (dsim_camera_walk.inc), the walk of the
// drones' grid (dsim_camera_drones.inc), the drone targets' host set-up (cam_drones_fill) and the argument records ScnK / CamDr.
#pragma once

struct ScanK {
  KView st;
  long long n, n_pad, tiles;
  const float* offset;             // SoA [3][n_pad] or null
  RayGridK rg;
  float far, t_min;                       // t_max (`far`: the walk's name for it) and t_min
  unsigned flags;
  const float* beams;                     // [n_beams][3]
  int n_beams;
  int beams_per_block;                    // blockIdx.y takes the beams [y, y + 1) * beams_per_block (n_beams: one chunk)
  float* range;                           // [n_beams][n_pad]
  int* hit;                               // same shape, or null
  ScnK pl;                                // PLACED instances (not a union with dr: a placed scan sees drones)
  CamDr dr;                               // DRONES instances
};

// One drone per lane.  Per tile a lane reads its position, quaternion and offset through the view (coalesced in both layouts),
// forms R(q) once (nine registers) and walks the beams: the table is wave-uniform and comes through the scalar path, d = R beam,
// and outputs are beam-major, so every store is a coalesced row.  Per beam: the plane, then the triangle walk of the camera
// (dsim_camera_walk.inc) — once in the task frame, or once per placement of the lane's scene — then the camera's walk of the
// drones' grid (dsim_camera_drones.inc) from the WORLD-frame origin; `best` and `body` carry through all of them.
// A lane whose pose is undefined (a non-finite position or R: every such value fails a comparison) casts nothing and reports
// misses; so does a beam that is zero or not finite.  No lane returns early: the workgroup meets at the staging barrier.
// A fleet too small to fill the device with one workgroup per tile spreads chunks of the beams over blockIdx.y (scan_beams_per_block: the
// pose is read once per chunk; every beam is cast by exactly one workgroup with the same arithmetic, so results do not depend on it).
// The records are staged in LDS before the first tile of which some lane can REACH the set: no nearer to the box (to the cull
// sphere of a placement) than t_max |beam|_max, widened well beyond float32 rounding, so the test decides speed only; the same
// test gates that lane's walks, so a workgroup that has not staged never reads LDS.
template <bool LDS, bool PLACED, bool DRONES, bool TRIS>
__global__ __launch_bounds__(256) void k_range_scan(ScanK a) {
  extern __shared__ float4 s_cam_rec[];
  const float near = a.t_min;
#ifdef DSIM_CAM_COUNT
  unsigned n_tests = 0u;           // the walk's text counts into it; the measuring build reports the camera's tests only
#endif
  const float miss = (a.flags & DSIM_SCAN_CLAMP) != 0u ? a.far : INFINITY;
  const bool ground = (a.flags & DSIM_SCAN_GROUND) != 0u;
  // how far a beam reaches (uniform): t_max times the longest beam of the table (a non-finite beam casts nothing)
  float bl2 = 0.0f;
  for (int b = 0; b < a.n_beams; ++b) {
    const float bx = a.beams[3 * b], by = a.beams[3 * b + 1], bz = a.beams[3 * b + 2];
    const float l2 = bx * bx + by * by + bz * bz;
    bl2 = l2 <= 3.0e38f ? fmaxf(bl2, l2) : bl2;
  }
  const float reach = a.far * sqrtf(bl2) * 1.001f + 1e-4f;
  bool staged = false;
  for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const long long i = tile * 256 + threadIdx.x;
    const bool lane = i < a.n;
    float ex = 0.0f, ey = 0.0f, ez = 0.0f, wx = 0.0f, wy = 0.0f, wz = 0.0f;
    float r00 = 1.0f, r01 = 0.0f, r02 = 0.0f, r10 = 0.0f, r11 = 1.0f, r12 = 0.0f, r20 = 0.0f, r21 = 0.0f, r22 = 1.0f;
    int sid = -1;
    bool defined = false;
    if (lane) {
      const long long o = kv_off(a.st, i);
      const float* p = a.st.base + o;
      const long long fs = a.st.field_stride;
      wx = p[0]; wy = p[fs]; wz = p[2 * fs];                    // the stored position: the world frame
      const float qx = p[3 * fs], qy = p[4 * fs], qz = p[5 * fs], qw = p[6 * fs];
      ex = wx; ey = wy; ez = wz;
      if (a.offset) { ex -= a.offset[i]; ey -= a.offset[a.n_pad + i]; ez -= a.offset[2 * a.n_pad + i]; }
      if (PLACED) sid = a.pl.scene_id[i];
      const float qq = qx * qx + qy * qy + qz * qz + qw * qw;
      const float s2 = 2.0f / qq;
      const float xs = qx * s2, ys = qy * s2, zs = qz * s2;
      r00 = 1.0f - (qy * ys + qz * zs); r10 = qx * ys + qw * zs; r20 = qx * zs - qw * ys;       // R(q), as k_depth_image forms it
      r01 = qx * ys - qw * zs; r11 = 1.0f - (qx * xs + qz * zs); r21 = qy * zs + qw * xs;
      r02 = qx * zs + qw * ys; r12 = qy * zs - qw * xs; r22 = 1.0f - (qx * xs + qy * ys);
      // (a NaN anywhere fails a comparison here: |x| <= FLT_MAX holds for finite x only)
      defined = fabsf(ex) <= 3.0e38f && fabsf(ey) <= 3.0e38f && fabsf(ez) <= 3.0e38f && fabsf(wx) <= 3.0e38f && fabsf(wy) <= 3.0e38f &&
                fabsf(wz) <= 3.0e38f && fabsf(r00) <= 2.0f && fabsf(r01) <= 2.0f && fabsf(r02) <= 2.0f && fabsf(r10) <= 2.0f &&
                fabsf(r11) <= 2.0f && fabsf(r12) <= 2.0f && fabsf(r20) <= 2.0f && fabsf(r21) <= 2.0f && fabsf(r22) <= 2.0f;
    }
    // ---- what of the set this lane can reach ----------------------------------------------------------------------------------
    bool reach_set = false;                                    // unplaced: the set's box
    unsigned reach_pl = 0u;                                    // PLACED: one bit per placement of the lane's scene
    const float4* pl = a.pl.place;
    if (TRIS && !PLACED && defined) {
      const float bx = fmaxf(fmaxf(a.rg.ox - ex, ex - a.rg.hix), 0.0f), by = fmaxf(fmaxf(a.rg.oy - ey, ey - a.rg.hiy), 0.0f);
      const float bz = fmaxf(fmaxf(a.rg.oz - ez, ez - a.rg.hiz), 0.0f);
      const float rr = reach + 1e-4f * (fabsf(ex) + fabsf(ey) + fabsf(ez));
      reach_set = bx * bx + by * by + bz * bz <= rr * rr;
    }
    if (PLACED && defined && sid >= 0 && (long long)sid < a.pl.K) {
      pl += 4 * ((size_t)sid * (size_t)a.pl.G);
      for (int g = 0; g < a.pl.G; ++g) {
        const float4 w = pl[4 * g];                            // (c_task, r_cull); r_cull = -inf for a slot at or above the count
        const float ux = ex - w.x, uy = ey - w.y, uz = ez - w.z;
        const float rr = (w.w + reach) * 1.001f + 1e-4f * (fabsf(ex) + fabsf(ey) + fabsf(ez));
        reach_pl |= (w.w >= 0.0f && ux * ux + uy * uy + uz * uz <= rr * rr) ? (1u << g) : 0u;
      }
    }
    if (LDS) {
      if (!staged && __syncthreads_or((reach_set || reach_pl != 0u) ? 1 : 0)) {
        obs_stage(s_cam_rec, a.rg.rec, a.rg.n_tri);
        staged = true;
      }
    }
    // ---- the beams ------------------------------------------------------------------------------------------------------------
    const int b_lo = (int)blockIdx.y * a.beams_per_block, b_hi = min(b_lo + a.beams_per_block, a.n_beams);
    for (int b = b_lo; b < b_hi; ++b) {
      const float bx = a.beams[3 * b], by = a.beams[3 * b + 1], bz = a.beams[3 * b + 2];
      // (a beam whose squared length overflows float32 is a non-finite beam: the reach above never counted it)
      const bool beam_ok = fabsf(bx) <= 3.0e38f && fabsf(by) <= 3.0e38f && fabsf(bz) <= 3.0e38f && (bx != 0.0f || by != 0.0f || bz != 0.0f) &&
                           bx * bx + by * by + bz * bz <= 3.0e38f;
      const float dx = r00 * bx + r01 * by + r02 * bz, dy = r10 * bx + r11 * by + r12 * bz, dz = r20 * bx + r21 * by + r22 * bz;
      const bool ray = defined && beam_ok && fabsf(dx) <= 3.0e38f && fabsf(dy) <= 3.0e38f && fabsf(dz) <= 3.0e38f;
      float best = INFINITY;
      int body = -1;
      if (ground && ray) {                                     // the plane z = 0: analytic, also for rays that miss the box
        const float tg = -ez / dz;                             // (dz = 0: +-inf or NaN, which fail the test)
        if (tg >= near && tg <= a.far) { best = tg; body = DSIM_SEG_GROUND; }
      }
      const bool live = ray && reach_set;
      // the set in the task frame (every instance with triangles but the PLACED ones)
#define CW_EX ex
#define CW_EY ey
#define CW_EZ ez
#define CW_DX dx
#define CW_DY dy
#define CW_DZ dz
#define CW_GATE (TRIS && !PLACED)
#define CW_BODY(rb) rb
#include "dsim_camera_walk.inc"
      if (PLACED) {
        // The ray into each placement's frame, subtract first, then rotate; t does not change, so best and body carry across
        // placements and bound every later walk.  A ray that passes the placement's cull sphere by (widened: speed only) is
        // skipped after the first 16 bytes of the slot.
        unsigned todo = ray ? reach_pl : 0u;
        const float inv_dd = 1.0f / (dx * dx + dy * dy + dz * dz);
        while (todo != 0u) {                                   // (a wave with no such lane skips the loop)
          const int g = __ffs((int)todo) - 1;
          todo &= todo - 1u;
          const float4 w0 = pl[4 * g];
          const float mx = w0.x - ex, my = w0.y - ey, mz = w0.z - ez;
          const float tc = fminf(fmaxf((mx * dx + my * dy + mz * dz) * inv_dd, 0.0f), fminf(a.far, best));
          const float cx_ = mx - tc * dx, cy_ = my - tc * dy, cz_ = mz - tc * dz;
          const float rr = w0.w * 1.001f + 1e-4f + 1e-4f * (fabsf(mx) + fabsf(my) + fabsf(mz));
          if (!(cx_ * cx_ + cy_ * cy_ + cz_ * cz_ <= rr * rr)) continue;
          const float4 c0 = pl[4 * g + 1], c1 = pl[4 * g + 2], c2 = pl[4 * g + 3];
          const float tx = ex - c0.w, ty = ey - c1.w, tz = ez - c2.w;
          const float lex = c0.x * tx + c0.y * ty + c0.z * tz, ley = c1.x * tx + c1.y * ty + c1.z * tz, lez = c2.x * tx + c2.y * ty + c2.z * tz;
          const float ldx = c0.x * dx + c0.y * dy + c0.z * dz, ldy = c1.x * dx + c1.y * dy + c1.z * dz, ldz = c2.x * dx + c2.y * dy + c2.z * dz;
          const int body_add = g * a.pl.n_bodies;
          const bool live = true;
#define CW_EX lex
#define CW_EY ley
#define CW_EZ lez
#define CW_DX ldx
#define CW_DY ldy
#define CW_DZ ldz
#define CW_GATE true
#define CW_BODY(rb) (rb + body_add)
#include "dsim_camera_walk.inc"
        }
      }
      if (DRONES) {                                            // from the stored position in the world frame
#define CD_GATE ray
#include "dsim_camera_drones.inc"
      }
      if (lane) {
        const bool got = best < INFINITY;
        const size_t out = (size_t)b * (size_t)a.n_pad + (size_t)i;
        a.range[out] = got ? best : miss;
        if (a.hit) {
          int sg = got ? body : -1;
          if (DRONES && sg <= DSIM_SEG_DRONE(0) && a.dr.label) sg = DSIM_SEG_DRONE(a.dr.label[DSIM_SEG_DRONE(sg)]);   // (its own inverse)
          a.hit[out] = sg;
        }
      }
    }
  }
}

// How many beams one workgroup casts.  With one workgroup per tile of 256 drones a fleet below SCAN_FILL_BLOCKS tiles (262 144
// drones: four workgroups per CU of a 256-CU device) leaves the device short of waves to hide the walk's latency behind — measured
// on an MI355X, 16 beams on the gate scene: 65 536 drones took 334 us in one chunk where 1 048 576 took 1 111 us.  Such a fleet
// spreads chunks of the beams over blockIdx.y until the grid has about SCAN_FILL_BLOCKS workgroups.
#define SCAN_FILL_BLOCKS 1024
static int scan_beams_per_block(long long tiles, int n_beams) {
  if (tiles >= SCAN_FILL_BLOCKS) return n_beams;
  const long long want = (SCAN_FILL_BLOCKS + tiles - 1) / tiles;             // chunks that would fill the device
  const int chunks = (int)(want < n_beams ? want : n_beams);
  return (n_beams + chunks - 1) / chunks;
}

extern "C" {

int dsim_range_scan(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_obstacles* set, const dsim_scan_args* args) {
  if (!ctx || !args || !args->beams || !args->range_out || n <= 0 || n > state.n_pad) return DSIM_E_ARG;
  const dsim_scan_args& s = *args;
  if (s.n_beams < 1 || s.n_beams > 64) return DSIM_E_ARG;
  if (!isfinite(s.t_min) || !isfinite(s.t_max) || !(s.t_min >= 0.0f) || !(s.t_max > s.t_min)) return DSIM_E_ARG;
  if ((s.flags & ~(uint32_t)(DSIM_SCAN_GROUND | DSIM_SCAN_CLAMP)) != 0u) return DSIM_E_ARG;
  if ((s.scenes != nullptr) != (s.scene_id != nullptr) || (s.scenes && set)) return DSIM_E_ARG;
  const dsim_obstacles* tris = s.scenes ? s.scenes->proto : set;
  if (tris && !tris->ray_start) return DSIM_E_ARG;
  if (!tris && !s.drones && !(s.flags & DSIM_SCAN_GROUND)) return DSIM_E_ARG;
  if (s.drones && ctx->n_types > 1 && !s.type_id) return DSIM_E_ARG;
  ScanK a;
  memset(&a, 0, sizeof(a));
  int rc = make_kview(state, 7, &a.st);
  if (rc) return rc;
  a.n = n; a.n_pad = state.n_pad; a.tiles = (n + 255) / 256; a.offset = s.offset;
  if (tris) ray_grid_fill(tris, &a.rg);
  a.far = s.t_max; a.t_min = s.t_min; a.flags = s.flags; a.beams = s.beams; a.n_beams = s.n_beams;
  a.range = s.range_out; a.hit = s.hit_out;
  if (s.scenes && (rc = scn_kargs(s.scenes, s.scene_id, &a.pl)) != 0) return rc;
  const hipStream_t st_ = (hipStream_t)stream;
  if (s.drones && (rc = cam_drones_fill(ctx, st_, state, s.drones, &a.dr)) != 0) return rc;
  const bool placed = s.scenes != nullptr, dr = s.drones != nullptr, lds = tris && tris->n_tri <= OBS_LDS_TRI;
  const size_t shm = lds ? (size_t)tris->n_tri * 64 : 0;
  a.beams_per_block = scan_beams_per_block(a.tiles, a.n_beams);
  const dim3 gr((unsigned)(a.tiles < OBS_MAX_BLOCKS ? a.tiles : OBS_MAX_BLOCKS), (unsigned)((a.n_beams + a.beams_per_block - 1) / a.beams_per_block)), tb(256);
  if (!tris) {
    if (dr) hipLaunchKernelGGL((k_range_scan<false, false, true, false>), gr, tb, 0, st_, a);
    else hipLaunchKernelGGL((k_range_scan<false, false, false, false>), gr, tb, 0, st_, a);
  } else if (placed) {
    if (lds && dr) hipLaunchKernelGGL((k_range_scan<true, true, true, true>), gr, tb, shm, st_, a);
    else if (lds) hipLaunchKernelGGL((k_range_scan<true, true, false, true>), gr, tb, shm, st_, a);
    else if (dr) hipLaunchKernelGGL((k_range_scan<false, true, true, true>), gr, tb, 0, st_, a);
    else hipLaunchKernelGGL((k_range_scan<false, true, false, true>), gr, tb, 0, st_, a);
  } else {
    if (lds && dr) hipLaunchKernelGGL((k_range_scan<true, false, true, true>), gr, tb, shm, st_, a);
    else if (lds) hipLaunchKernelGGL((k_range_scan<true, false, false, true>), gr, tb, shm, st_, a);
    else if (dr) hipLaunchKernelGGL((k_range_scan<false, false, true, true>), gr, tb, 0, st_, a);
    else hipLaunchKernelGGL((k_range_scan<false, false, false, true>), gr, tb, 0, st_, a);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
