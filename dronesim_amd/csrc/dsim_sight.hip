// Line of sight (dsim_line_of_sight): per drone and slot, whether the segment e_i + s rel[t][:][i], s in [0, 1], is cut by the
// obstacle set's triangles (or the placements of the drone's scene) or the plane z = 0, and by what first (include/dronesim_amd.h
// has the segment).  The mapping is the scanner's: one drone per lane, tiles of 256 walked grid-stride, the position loaded
// coalesced once, the lane loops over the slots; where the scanner rotates a shared beam table, every lane here reads its own
// direction from the slot-major rows the nearest-neighbour observation writes (dsim_knn's rel_pos_out), used as given.
// Compiled as part of dsim_obstacles.hip, which includes this file: it reads the set's and the scenes' private records and uses
// what dsim_camera.hip and dsim_scan.hip state: the ray grid's record, the triangle walk (dsim_camera_walk.inc, with near = 0 and
// far = 1), the scenes' table (ScnK) and the spreading of a small fleet over blockIdx.y (scan_beams_per_block).
// dsim_line_of_sight_drones: the other drones hide too, as their bounding spheres — the walk of the drones' grid
// (dsim_camera_drones.inc) and its host set-up (cam_drones_fill) as the scanner uses them, with a sphere test of its own.
#pragma once

struct SightK {
  KView st;
  long long n, n_pad, tiles;
  const float* offset;             // SoA [3][n_pad] or null
  RayGridK rg;                     // rec == null: no triangles at all (the plane alone)
  float far;                       // 1: the walk's name for the segment's far end
  unsigned flags;
  const float* rel;                // [k][3][n_pad]
  const int* index;                // [k][n_pad] or null
  int k;
  int slots_per_block;             // blockIdx.y takes the slots [y, y + 1) * slots_per_block (k: one chunk)
  int* visible;                    // [k][n_pad]
  int* blocker;                    // same shape, or null
  float* frac;                     // same shape, or null
  ScnK pl;                         // PLACED instances
  CamDr dr;                        // DRONES instances (not a union with pl: scenes and drones go together)
};

// One sphere (x, y, z, R) against the SEGMENT w + s d, s in [0, tmax], as a solid ball with both ends closed, as for triangles:
// the ball blocks when it meets the segment at all — rho^2 <= R^2, t0 <= tmax, t1 >= 0, the roots in cam_sphere's
// cancellation-free form — at s = max(t0, 0): a segment that starts inside the ball is blocked at 0 (cam_sphere, a surface, would
// take the second root there).  The world index is read only by a lane that hits: neither the lane's own drone nor the slot's
// target (`tgt`, a world index; -1: none) blocks.
__device__ __forceinline__ void sight_sphere(const float4 p, const int* __restrict__ idx, int k, int own, int tgt, float wx, float wy,
                                             float wz, float dx, float dy, float dz, float inv_a, float tmax, float& best, int& body) {
  const float mx = p.x - wx, my = p.y - wy, mz = p.z - wz;
  const float tc = (mx * dx + my * dy + mz * dz) * inv_a;
  const float qx = mx - tc * dx, qy = my - tc * dy, qz = mz - tc * dz;
  const float disc = p.w * p.w - (qx * qx + qy * qy + qz * qz);
  const float h = DSIM_SQRT(fmaxf(disc, 0.0f) * inv_a);
  const float t0 = tc - h, t1 = tc + h;
  const float t = fmaxf(t0, 0.0f);
  if (p.w > 0.0f && disc >= 0.0f && t0 <= tmax && t1 >= 0.0f && t < best) {    // (a NaN anywhere fails a comparison)
    const int j = idx[k];
    if (j != own && j != tgt) { best = t; body = DSIM_SEG_DRONE(j); }
  }
}

// One drone per lane.  Per tile a lane reads its position and offset through the view (coalesced in both layouts), then passes
// over the rel rows of its chunk of slots twice: once for the longest segment it will cast, which says what of the world the lane
// can REACH, and once to cast.  Outputs are slot-major, so every store is a coalesced row, and a slot belongs to exactly one
// workgroup, so chunks of the slots spread over blockIdx.y race with nobody.  Per slot: the plane, then the triangle walk of the
// camera (dsim_camera_walk.inc) — once in the task frame, or once per placement of the lane's scene, `best` and `body` carrying
// across — with near = 0 and far = 1, both ends closed, both faces seen, the nearest hit winning.
// A slot is cast when its index is not negative, e is finite, and d is finite, not zero and of a squared length float32 holds;
// every other slot reads 0 / -1 / +inf.  No lane returns early: the workgroup meets at the staging barrier.
// The records are staged in LDS before the first tile of which some lane can reach the set: no nearer to the box (to the cull
// sphere of a placement) than its own longest segment, widened as the scanner widens its reach, well beyond float32 rounding, so
// the test decides speed only; the same test gates that lane's walks, so a workgroup that has not staged never reads LDS.
// DRONES: behind the triangle walks the lane walks the drones' grid from the STORED position in the world frame with the same d
// (the scanner's split: the triangles and the plane keep e), `best` and `body` carrying on; the reach plays no part in it, the
// walk ends where the segment does.  TRIS = false: no triangles at all (drones and, by the flag, the plane).
template <bool LDS, bool PLACED, bool DRONES = false, bool TRIS = true>
__global__ __launch_bounds__(256) void k_line_of_sight(SightK a) {
  extern __shared__ float4 s_cam_rec[];
  const float near = 0.0f;
#ifdef DSIM_CAM_COUNT
  unsigned n_tests = 0u;           // the walk's text counts into it; the measuring build reports the camera's tests only
#endif
  const bool ground = (a.flags & DSIM_SIGHT_GROUND) != 0u;
  const bool tris = TRIS && a.rg.rec != nullptr;
  const int t_lo = (int)blockIdx.y * a.slots_per_block, t_hi = min(t_lo + a.slots_per_block, a.k);
  bool staged = false;
  for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const long long i = tile * 256 + threadIdx.x;
    const bool lane = i < a.n;
    float ex = 0.0f, ey = 0.0f, ez = 0.0f, wx = 0.0f, wy = 0.0f, wz = 0.0f;
    int sid = -1;
    bool defined = false;
    float l2max = 0.0f;
    bool any = false;                                          // some slot of the chunk will be cast
    if (lane) {
      const long long o = kv_off(a.st, i);
      const float* p = a.st.base + o;
      const long long fs = a.st.field_stride;
      ex = p[0]; ey = p[fs]; ez = p[2 * fs];
      if (DRONES) { wx = ex; wy = ey; wz = ez; }                // the stored position: the world frame
      if (a.offset) { ex -= a.offset[i]; ey -= a.offset[a.n_pad + i]; ez -= a.offset[2 * a.n_pad + i]; }
      if (PLACED) sid = a.pl.scene_id[i];
      // (a NaN anywhere fails a comparison here: |x| <= FLT_MAX holds for finite x only)
      defined = fabsf(ex) <= 3.0e38f && fabsf(ey) <= 3.0e38f && fabsf(ez) <= 3.0e38f;
      if (DRONES) defined = defined && fabsf(wx) <= 3.0e38f && fabsf(wy) <= 3.0e38f && fabsf(wz) <= 3.0e38f;
      // how far this lane's segments reach: the longest slot of its chunk whose index is not negative
      for (int t = t_lo; t < t_hi; ++t) {
        const float* r = a.rel + (size_t)t * 3u * (size_t)a.n_pad + (size_t)i;
        const float dx = r[0], dy = r[a.n_pad], dz = r[2 * a.n_pad];
        const float l2 = dx * dx + dy * dy + dz * dz;
        const bool used = !a.index || a.index[(size_t)t * (size_t)a.n_pad + (size_t)i] >= 0;
        // (a slot that will not be cast for its length — not finite, or a square that overflows — counts as the longest there
        // is: fminf drops the NaN.  The reach decides speed only, so it need not repeat the cast test to the bit)
        l2max = used ? fmaxf(l2max, fminf(l2, 3.0e38f)) : l2max;
        any = any || used;
      }
    }
    const float reach = sqrtf(l2max) * 1.001f + 1e-4f;
    // ---- what of the set this lane can reach ----------------------------------------------------------------------------------
    bool reach_set = false;                                    // unplaced: the set's box
    unsigned reach_pl = 0u;                                    // PLACED: one bit per placement of the lane's scene
    const float4* pl = a.pl.place;
    if (!PLACED && tris && defined && any) {
      const float bx = fmaxf(fmaxf(a.rg.ox - ex, ex - a.rg.hix), 0.0f), by = fmaxf(fmaxf(a.rg.oy - ey, ey - a.rg.hiy), 0.0f);
      const float bz = fmaxf(fmaxf(a.rg.oz - ez, ez - a.rg.hiz), 0.0f);
      const float rr = reach + 1e-4f * (fabsf(ex) + fabsf(ey) + fabsf(ez));
      reach_set = bx * bx + by * by + bz * bz <= rr * rr;
    }
    if (PLACED && defined && any && sid >= 0 && (long long)sid < a.pl.K) {
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
    // ---- the slots ------------------------------------------------------------------------------------------------------------
    for (int t = t_lo; t < t_hi; ++t) {
      float dx = 0.0f, dy = 0.0f, dz = 0.0f;
      bool used = false;
      int tgt = -1;                                            // DRONES: the slot's own target, a world index (none without index)
      if (lane) {
        const float* r = a.rel + (size_t)t * 3u * (size_t)a.n_pad + (size_t)i;
        dx = r[0]; dy = r[a.n_pad]; dz = r[2 * a.n_pad];
        if (DRONES) {
          if (a.index) tgt = a.index[(size_t)t * (size_t)a.n_pad + (size_t)i];
          used = tgt >= 0 || !a.index;
        } else {
          used = !a.index || a.index[(size_t)t * (size_t)a.n_pad + (size_t)i] >= 0;
        }
      }
      // (a segment whose squared length overflows float32 is a non-finite segment: the reach above never counted it)
      const bool ray = defined && used && fabsf(dx) <= 3.0e38f && fabsf(dy) <= 3.0e38f && fabsf(dz) <= 3.0e38f &&
                       (dx != 0.0f || dy != 0.0f || dz != 0.0f) && dx * dx + dy * dy + dz * dz <= 3.0e38f;
      float best = INFINITY;
      int body = -1;
      if (ground && ray) {                                     // the plane z = 0: analytic, also for segments that miss the box
        const float tg = -ez / dz;                             // (dz = 0: +-inf or NaN, which fail the test)
        if (tg >= near && tg <= a.far) { best = tg; body = DSIM_SEG_GROUND; }
      }
      const bool live = ray && reach_set;
      // the set in the task frame (the unplaced instances)
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
        // The segment into each placement's frame, subtract first, then rotate; s does not change, so best and body carry across
        // placements and bound every later walk.  A segment that passes the placement's cull sphere by (widened: speed only) is
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
#define CD_SPHERE(p, idx, k) sight_sphere(p, idx, k, own, tgt, wx, wy, wz, dx, dy, dz, inv_a, tmax, best, body)
#include "dsim_camera_drones.inc"
      }
      if (lane) {
        const bool got = best < INFINITY;
        const size_t out = (size_t)t * (size_t)a.n_pad + (size_t)i;
        a.visible[out] = (ray && !got) ? 1 : 0;
        if (a.blocker) {
          int sg = got ? body : -1;
          if (DRONES && sg <= DSIM_SEG_DRONE(0) && a.dr.label) sg = DSIM_SEG_DRONE(a.dr.label[DSIM_SEG_DRONE(sg)]);   // (its own inverse)
          a.blocker[out] = sg;
        }
        if (a.frac) a.frac[out] = got ? best : INFINITY;
      }
    }
  }
}

// Both entry points: the arguments checked, the fleet binned (with drones) and the instance chosen.
static int sight_call(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_obstacles* set, const dsim_sight_args* args,
                      bool with_drones, const uint8_t* type_id, const dsim_camera_drones* drones) {
  if (!ctx || !args || !args->rel || !args->visible_out || n <= 0 || n > state.n_pad) return DSIM_E_ARG;
  const dsim_sight_args& s = *args;
  if (s.k < 1 || s.k > 32) return DSIM_E_ARG;
  if ((s.flags & ~(uint32_t)DSIM_SIGHT_GROUND) != 0u) return DSIM_E_ARG;
  if ((s.scenes != nullptr) != (s.scene_id != nullptr) || (s.scenes && set)) return DSIM_E_ARG;
  const dsim_obstacles* tris = s.scenes ? s.scenes->proto : set;
  if (tris && !tris->ray_start) return DSIM_E_ARG;
  if (!with_drones && !tris && !(s.flags & DSIM_SIGHT_GROUND)) return DSIM_E_ARG;
  if (with_drones && (!drones || (ctx->n_types > 1 && !type_id))) return DSIM_E_ARG;
  SightK a;
  memset(&a, 0, sizeof(a));
  int rc = make_kview(state, 3, &a.st);
  if (rc) return rc;
  a.n = n; a.n_pad = state.n_pad; a.tiles = (n + 255) / 256; a.offset = s.offset;
  if (tris) ray_grid_fill(tris, &a.rg);
  a.far = 1.0f; a.flags = s.flags; a.rel = s.rel; a.index = s.index; a.k = s.k;
  a.visible = s.visible_out; a.blocker = s.blocker_out; a.frac = s.frac_out;
  if (s.scenes && (rc = scn_kargs(s.scenes, s.scene_id, &a.pl)) != 0) return rc;
  const hipStream_t st_ = (hipStream_t)stream;
  if (with_drones && (rc = cam_drones_fill(ctx, st_, state, drones, &a.dr)) != 0) return rc;
  const bool placed = s.scenes != nullptr, lds = tris && tris->n_tri <= OBS_LDS_TRI;
  const size_t shm = lds ? (size_t)tris->n_tri * 64 : 0;
  a.slots_per_block = scan_beams_per_block(a.tiles, a.k);
  const dim3 gr((unsigned)(a.tiles < OBS_MAX_BLOCKS ? a.tiles : OBS_MAX_BLOCKS), (unsigned)((a.k + a.slots_per_block - 1) / a.slots_per_block)), tb(256);
  if (with_drones) {
    if (!tris) hipLaunchKernelGGL((k_line_of_sight<false, false, true, false>), gr, tb, 0, st_, a);     // (and the plane, by the flag)
    else if (placed && lds) hipLaunchKernelGGL((k_line_of_sight<true, true, true, true>), gr, tb, shm, st_, a);
    else if (placed) hipLaunchKernelGGL((k_line_of_sight<false, true, true, true>), gr, tb, 0, st_, a);
    else if (lds) hipLaunchKernelGGL((k_line_of_sight<true, false, true, true>), gr, tb, shm, st_, a);
    else hipLaunchKernelGGL((k_line_of_sight<false, false, true, true>), gr, tb, 0, st_, a);
  } else if (placed) {
    if (lds) hipLaunchKernelGGL((k_line_of_sight<true, true>), gr, tb, shm, st_, a);
    else hipLaunchKernelGGL((k_line_of_sight<false, true>), gr, tb, 0, st_, a);
  } else {
    if (lds) hipLaunchKernelGGL((k_line_of_sight<true, false>), gr, tb, shm, st_, a);
    else hipLaunchKernelGGL((k_line_of_sight<false, false>), gr, tb, 0, st_, a);      // (and the plane alone: no records at all)
  }
  return (int)hipGetLastError();
}

extern "C" {

int dsim_line_of_sight(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_obstacles* set, const dsim_sight_args* args) {
  return sight_call(ctx, stream, n, state, set, args, false, nullptr, nullptr);
}

int dsim_line_of_sight_drones(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_obstacles* set,
                              const dsim_sight_args* args, const uint8_t* type_id, const dsim_camera_drones* drones) {
  return sight_call(ctx, stream, n, state, set, args, true, type_id, drones);
}

}  // extern "C"
