// Depth camera (dsim_depth_image, dsim_depth_image_drones): per-drone depth and segmentation images of the static obstacle set —
// and, with the second entry point, of the other drones as their bounding spheres — one ray per pixel against
// the set's RAY grid (dsim_obstacle_grid.h: ray_plan; include/dronesim_amd.h has the camera model).  Compiled as part of
// dsim_obstacles.hip, which includes this file: it reads the set's private record (struct dsim_obstacles) and shares OBS_LDS_TRI and
// obs_stage.  What the range scanner (dsim_scan.hip) shares with the camera is stated here once: the ray grid's record (RayGridK,
// ray_grid_fill), the triangle walk (dsim_camera_walk.inc) and the walk of the drones' grid (dsim_camera_drones.inc), both as
// text, the drone targets' record and host set-up (CamDr, cam_drones_fill) and the sphere test (cam_sphere).
#pragma once

#include <stdlib.h>

#define CAM_TILE 8                 // a wave is an 8 x 8 pixel tile; a workgroup the 2 x 2 tiles of a 16 x 16 pixel block

// The other drones as their bounding spheres (dsim_depth_image_drones): the fleet binned on the contact watch's xy grid
// (dsim_kernels.h: SphereGrid), the caller's label table and the range beyond which no drone is drawn.
struct CamDr {
  SphereGrid g;
  const int* label;                // [m] k of DSIM_SEG_DRONE per world index, or null: the world index
  float range;
};

// The set's ray grid as a kernel reads it (dsim_camera_walk.inc; zeroed: no set).  Its box is [o, hi].
struct RayGridK {
  const float4* rec;
  const int* cell_start;
  const int* cell_tri;
  int n_tri;
  float ox, oy, oz, cell, inv_cell;
  int nx, ny, nz;
  float hix, hiy, hiz;
};

struct CamK {
  KView st;
  long long n_pad;
  const int* cam_index;            // [n_cam] drone indices in storage order, or null: the camera's own number
  const float* offset;             // SoA [3][n_pad] or null
  const uint8_t* type_id;          // or null: type 0
  const DevType* types;
  int n_types;
  RayGridK rg;
  int W, H, bx;                           // image size; 16 x 16 blocks per image row
  unsigned blocks_per_cam;
  float inv_w, inv_h, th, tha, far;       // 1 / W, 1 / H, tan(fov / 2), ... x aspect
  unsigned flags;
  float* depth;                           // [n_cam][H][W]
  int* seg;                               // same shape, or null
#ifdef DSIM_CAM_COUNT
  unsigned long long* tests;              // triangle tests, summed over every ray (a measuring build: tools/bench_camera.py)
#endif
  union {
    CamDr dr;                             // DRONES instances only
    ScnK pl;                              // PLACED instances only (never both: scenes with drones are refused); dsim_obstacles.hip
  };
};

// One sphere (x, y, z, R) against the ray w + t d, cancellation-free: m = c - w, tc = m.d / d.d the parameter of the ray's closest
// point, rho^2 = |m - tc d|^2, roots tc -+ sqrt((R^2 - rho^2) / d.d).  (b^2 - a c loses a 5 cm sphere at 50 m in float32: both
// terms are ~2500 and their difference ~0.0025.)  The first root unless it lies in front of the near plane: both faces are seen,
// as with triangles.  The world index is read only by a lane that hits: the camera's own drone is never drawn.
__device__ __forceinline__ void cam_sphere(const float4 p, const int* __restrict__ idx, int k, int own, float wx, float wy, float wz,
                                           float dx, float dy, float dz, float inv_a, float near, float tmax, float& best, int& body) {
  const float mx = p.x - wx, my = p.y - wy, mz = p.z - wz;
  const float tc = (mx * dx + my * dy + mz * dz) * inv_a;
  const float qx = mx - tc * dx, qy = my - tc * dy, qz = mz - tc * dz;
  const float disc = p.w * p.w - (qx * qx + qy * qy + qz * qz);
  const float h = DSIM_SQRT(fmaxf(disc, 0.0f) * inv_a);
  const float t0 = tc - h, t1 = tc + h;
  const float t = t0 >= near ? t0 : t1;
  if (p.w > 0.0f && disc >= 0.0f && t >= near && t <= tmax && t < best) {       // (a NaN anywhere fails a comparison)
    const int j = idx[k];
    if (j != own) { best = t; body = DSIM_SEG_DRONE(j); }
  }
}

// One lane per pixel.  The pose and the basis are the same for the whole workgroup: the drone's index comes from blockIdx, its
// position and quaternion are read through the view with that uniform index, and f, s, u and the eye stay in scalar registers.
// A lane slab-clips its ray against the grid's box, walks the cells by 3-D DDA (Amanatides & Woo, three named scalars per
// quantity and selects: an array indexed by the stepping axis would live in scratch), tests the list of every cell with
// Moller-Trumbore from the records (a, ab, ac; body in r3.w) and stops as soon as its best t is not beyond the cell's exit.
// DRONES: behind the triangle walk the same lane walks the drones' grid (dsim_camera_drones.inc) from the eye in the WORLD frame
// (p_i + (0, 0, L): the triangles and the plane keep the task frame p_i - offset_i; d is the same, so both t are eye-space depth
// and share `best`).  TRIS = false: no obstacle set (drones and, optionally, the plane).  PLACED (dsim_depth_image_scenes): the set is
// a prototype, walked once per placement of the camera's scene in that placement's frame (dsim_camera_walk.inc is the walk, as
// text, for both); the plane stays in the task frame.
template <bool LDS, bool SEG, bool DRONES = false, bool TRIS = true, bool PLACED = false>
__global__ __launch_bounds__(256) void k_depth_image(CamK a) {
  extern __shared__ float4 s_cam_rec[];
  const unsigned cam = blockIdx.x / a.blocks_per_cam, blk = blockIdx.x - cam * a.blocks_per_cam;
  const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const int by = (int)(blk / (unsigned)a.bx), bxi = (int)(blk - (unsigned)by * (unsigned)a.bx);
  const int col = bxi * 16 + (int)(wave & 1u) * CAM_TILE + (int)(lane & 7u);
  const int row = by * 16 + (int)(wave >> 1) * CAM_TILE + (int)(lane >> 3);
  const bool live = col < a.W && row < a.H;                   // tiles at the right and bottom edge are masked
  const bool metric = (a.flags & DSIM_CAM_METRIC) != 0u;
  const float miss = metric ? INFINITY : 1.0f;
  const size_t out = ((size_t)cam * (size_t)a.H + (size_t)row) * (size_t)a.W + (size_t)col;

  // ---- the camera (uniform) -------------------------------------------------------------------------------------------------
  const long long i = a.cam_index ? (long long)a.cam_index[cam] : (long long)cam;
  bool defined = i >= 0 && i < a.n_pad;
  float wx = 0.0f, wy = 0.0f, wz = 0.0f;                        // DRONES: the eye in the world frame
  float ex = 0.0f, ey = 0.0f, ez = 0.0f, fx = 1.0f, fy = 0.0f, fz = 0.0f, sx = 0.0f, sy = 0.0f, near = 1.0f;
  if (defined) {
    const long long o = kv_off(a.st, i);
    const float* p = a.st.base + o;
    const long long fs = a.st.field_stride;
    float px = p[0], py = p[fs], pz = p[2 * fs];
    const float rx = px, ry = py, rz = pz;                     // the stored position: the world frame
    Q4 q;
    q.x = p[3 * fs]; q.y = p[4 * fs]; q.z = p[5 * fs]; q.w = p[6 * fs];
    if (a.offset) { px -= a.offset[i]; py -= a.offset[a.n_pad + i]; pz -= a.offset[2 * a.n_pad + i]; }
    near = dev_type(a.types, a.type_id ? min((int)a.type_id[i], a.n_types - 1) : 0).arm;
    const float qq = q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w;
    const float s2 = 2.0f / qq;
    const float xs = q.x * s2, ys = q.y * s2, zs = q.z * s2;
    const float r0 = 1.0f - (q.y * ys + q.z * zs), r3 = q.x * ys + q.w * zs, r6 = q.x * zs - q.w * ys;   // R(q) (1, 0, 0)
    fx = 1000.0f * r0; fy = 1000.0f * r3; fz = 1000.0f * r6 - near;                                       // target - eye
    const float fi = 1.0f / sqrtf(fx * fx + fy * fy + fz * fz);
    fx *= fi; fy *= fi; fz *= fi;
    const float ss = fx * fx + fy * fy;                        // |f x up|^2 with up = (0, 0, 1): f x up = (fy, -fx, 0)
    const float si = 1.0f / sqrtf(ss);
    sx = fy * si; sy = -fx * si;
    ex = px; ey = py; ez = pz + near;
    if (DRONES) { wx = rx; wy = ry; wz = rz + near; }
    // (a NaN anywhere fails a comparison here: |x| <= FLT_MAX holds for finite x only)
    defined = fabsf(ex) <= 3.0e38f && fabsf(ey) <= 3.0e38f && fabsf(ez) <= 3.0e38f && fabsf(fx) <= 2.0f && fabsf(fy) <= 2.0f &&
              fabsf(fz) <= 2.0f && ss >= 1e-12f && fabsf(sx) <= 2.0f && fabsf(sy) <= 2.0f && near > 0.0f;
  }
  if (!defined) {                                              // no defined image: background everywhere (a uniform branch)
    if (live) {
      a.depth[out] = miss;
      if (SEG) a.seg[out] = -1;
    }
    return;
  }
  const float ux = sy * fz, uy = -(sx * fz), uz = sx * fy - sy * fx;        // u = s x f, s = (sx, sy, 0)
  if (LDS) obs_stage(s_cam_rec, a.rg.rec, a.rg.n_tri);         // the whole set's records, once per workgroup (as the watch does)

  // ---- the ray of this pixel -------------------------------------------------------------------------------------------------
  const float ca = (2.0f * ((float)col + 0.5f) * a.inv_w - 1.0f) * a.tha;
  const float cb = (1.0f - 2.0f * ((float)row + 0.5f) * a.inv_h) * a.th;
  const float dx = fx + ca * sx + cb * ux, dy = fy + ca * sy + cb * uy, dz = fz + cb * uz;
  float best = INFINITY;
  int body = -1;
  if ((a.flags & DSIM_CAM_GROUND) != 0u) {                     // the plane z = 0: analytic, also for rays that miss the box
    const float tg = -ez / dz;                                 // (dz = 0: +-inf or NaN, which fail the test)
    if (tg >= near && tg <= a.far) { best = tg; body = DSIM_SEG_GROUND; }
  }
#ifdef DSIM_CAM_COUNT
  unsigned n_tests = 0u;
#endif
  // the set in the task frame (every instance but the PLACED ones, of which nothing of this survives)
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
    // The camera's scene is uniform: its placements are read through the scalar path, the eye and the basis go into each
    // placement's frame once (subtract first, then rotate), and a lane forms its ray from the rotated basis.  t is eye-space depth
    // in every frame, so best and body carry across placements and bound every later walk.  A scene outside [0, K): no obstacles.
    const int sid = a.pl.scene_id[i];
    if (sid >= 0 && (long long)sid < a.pl.K) {
      const float4* pl = a.pl.place + 4 * ((size_t)sid * (size_t)a.pl.G);
      for (int g = 0; g < a.pl.G; ++g) {
        const float4 w0 = pl[4 * g];
        if (!(w0.w >= 0.0f)) continue;                         // a slot at or above the scene's count
        const float4 c0 = pl[4 * g + 1], c1 = pl[4 * g + 2], c2 = pl[4 * g + 3];
        const float tx = ex - c0.w, ty = ey - c1.w, tz = ez - c2.w;
        const float lex = c0.x * tx + c0.y * ty + c0.z * tz, ley = c1.x * tx + c1.y * ty + c1.z * tz, lez = c2.x * tx + c2.y * ty + c2.z * tz;
        const float lfx = c0.x * fx + c0.y * fy + c0.z * fz, lfy = c1.x * fx + c1.y * fy + c1.z * fz, lfz = c2.x * fx + c2.y * fy + c2.z * fz;
        const float lsx = c0.x * sx + c0.y * sy, lsy = c1.x * sx + c1.y * sy, lsz = c2.x * sx + c2.y * sy;
        const float lux = c0.x * ux + c0.y * uy + c0.z * uz, luy = c1.x * ux + c1.y * uy + c1.z * uz, luz = c2.x * ux + c2.y * uy + c2.z * uz;
        const float ldx = lfx + ca * lsx + cb * lux, ldy = lfy + ca * lsy + cb * luy, ldz = lfz + ca * lsz + cb * luz;
        const int body_add = g * a.pl.n_bodies;
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
  }
  if (DRONES) {
#define CD_GATE live
#include "dsim_camera_drones.inc"
  }
  if (live) {
    const bool got = best < INFINITY;
    a.depth[out] = metric ? best : (got ? a.far * (best - near) * DSIM_RCP(best * (a.far - near)) : 1.0f);
    if (SEG) {
      int sg = got ? body : -1;
      if (DRONES && sg <= DSIM_SEG_DRONE(0) && a.dr.label) sg = DSIM_SEG_DRONE(a.dr.label[DSIM_SEG_DRONE(sg)]);   // (its own inverse)
      a.seg[out] = sg;
    }
  }
#ifdef DSIM_CAM_COUNT
  if (a.tests && n_tests) atomicAdd(a.tests, (unsigned long long)n_tests);
#endif
}

#ifdef DSIM_CAM_COUNT
static unsigned long long* g_cam_tests = nullptr;              // device counter of the measuring build
#endif

// the ray grid of a set with rays enabled, as the kernels read it
static void ray_grid_fill(const dsim_obstacles* set, RayGridK* r) {
  const dsim_obstacle_grid& g = set->ray_grid;
  r->rec = set->rec; r->cell_start = set->ray_start; r->cell_tri = set->ray_tri; r->n_tri = set->n_tri;
  r->ox = g.origin[0]; r->oy = g.origin[1]; r->oz = g.origin[2]; r->cell = g.cell; r->inv_cell = 1.0f / g.cell;
  r->nx = g.nx; r->ny = g.ny; r->nz = g.nz; r->hix = g.hi[0]; r->hiy = g.hi[1]; r->hiz = g.hi[2];
}

// The drone targets of a call (dsim_depth_image_drones, dsim_range_scan): the caller's record checked, the fleet binned on the
// stream (dsim_sphere_grid_build) and the kernel's record filled.  Called once the sensor's own arguments have passed: a call that is
// refused for them has binned nothing.
static int cam_drones_fill(dsim_ctx* ctx, hipStream_t st_, const dsim_view& state, const dsim_camera_drones* drones, CamDr* out) {
  if (!drones || !drones->grid || !(drones->range > 0.0f)) return DSIM_E_ARG;
  const dsim_downwash_args* g = drones->grid;
  if (g->halo) return DSIM_E_UNSUPPORTED;
  // the drones of the state block among the world's: all of them (pos_all NULL), or those from local_offset on
  const int64_t m = g->pos_all ? (g->m - g->local_offset < state.n_pad ? g->m - g->local_offset : state.n_pad) : g->m;
  const int rc = dsim_sphere_grid_build(ctx, st_, m, state, g, drones->radius_all, (unsigned long long*)drones->outside_out, &out->g);
  if (rc) return rc;
  out->label = drones->label; out->range = drones->range;
  return DSIM_OK;
}

// the arguments both entry points share, checked and laid out for the kernel; set = null (dsim_depth_image_drones): no triangles
static int cam_fill(dsim_ctx* ctx, const dsim_view& state, const dsim_obstacles* set, const dsim_camera_params* params, int64_t n_cam,
                    const int32_t* cam_index, const float* offset, const uint8_t* type_id, float* depth_out, int32_t* seg_out,
                    CamK* out, int64_t* blocks_out) {
  if (!ctx || !params || !depth_out || (set && !set->ray_start) || n_cam < 1) return DSIM_E_ARG;
  const dsim_camera_params& p = *params;
  if (p.width < 1 || p.width > 1024 || p.height < 1 || p.height > 1024) return DSIM_E_ARG;
  if (!(p.far > 0.0f) || !isfinite(p.far) || !(p.fov_deg > 0.0f) || !(p.fov_deg < 180.0f) || !(p.aspect > 0.0f) || !isfinite(p.aspect))
    return DSIM_E_ARG;
  if (ctx->n_types > 1 && !type_id) return DSIM_E_ARG;
  for (int t = 0; t < ctx->n_types; ++t) if (!((float)ctx->h_types[t].arm > 0.0f)) return DSIM_E_ARG;
  if (!cam_index && n_cam > state.n_pad) return DSIM_E_ARG;
  CamK& a = *out;
  memset(&a, 0, sizeof(a));
  const int rc = make_kview(state, 7, &a.st);
  if (rc) return rc;
  a.n_pad = state.n_pad; a.cam_index = cam_index; a.offset = offset; a.type_id = type_id;
  a.types = ctx->d_types; a.n_types = ctx->n_types;
  if (set) ray_grid_fill(set, &a.rg);
  a.W = p.width; a.H = p.height; a.bx = (p.width + 15) / 16;
  a.blocks_per_cam = (unsigned)(a.bx * ((p.height + 15) / 16));
  a.inv_w = 1.0f / (float)p.width; a.inv_h = 1.0f / (float)p.height;
  a.th = (float)tan((double)p.fov_deg * (M_PI / 360.0)); a.tha = a.th * p.aspect;
  a.far = p.far; a.flags = p.flags; a.depth = depth_out; a.seg = seg_out;
  const int64_t blocks = n_cam * (int64_t)a.blocks_per_cam;
  if (blocks > 0x7fffffffLL) return DSIM_E_ARG;
#ifdef DSIM_CAM_COUNT
  if (!g_cam_tests && hipMalloc((void**)&g_cam_tests, sizeof(unsigned long long)) == hipSuccess)
    (void)hipMemset(g_cam_tests, 0, sizeof(unsigned long long));
  a.tests = g_cam_tests;
#endif
  *blocks_out = blocks;
  return DSIM_OK;
}

extern "C" {

int dsim_obstacle_ray_grid_plan(const float* tri, int64_t n_tri, dsim_obstacle_grid* out) {
  return dsim_obs::ray_plan(tri, n_tri, false, out);
}

int dsim_obstacle_ray_grid_build(const float* tri, int64_t n_tri, const dsim_obstacle_grid* g, int32_t* cell_start, int32_t* cell_tri) {
  return dsim_obs::ray_build(tri, n_tri, false, g, cell_start, cell_tri);
}

int dsim_obstacles_enable_rays(dsim_ctx* ctx, dsim_obstacles* set) {
  if (!ctx || !set) return DSIM_E_ARG;
  if (set->ray_start) return DSIM_OK;
  // DSIM_RAY_ONE_CELL=1: the whole box as one cell that lists every triangle, the brute-force caster a measurement compares
  // the grid against (tools/bench_camera.py); results do not depend on it
  const char* env = getenv("DSIM_RAY_ONE_CELL");
  const bool one_cell = env && env[0] == '1';
  const float* tri = set->tri_host.data();
  dsim_obstacle_grid g;
  int rc = dsim_obs::ray_plan(tri, set->n_tri, one_cell, &g);
  if (rc) return rc;
  const int64_t cells = (int64_t)g.nx * g.ny * g.nz;
  std::vector<int32_t> start, list;
  try {
    start.resize(cells + 1); list.resize(g.list_len > 0 ? g.list_len : 1);
  } catch (const std::bad_alloc&) { return (int)hipErrorOutOfMemory; }
  rc = dsim_obs::ray_build(tri, set->n_tri, one_cell, &g, start.data(), list.data());
  if (rc) return rc;
  int *d_start = nullptr, *d_list = nullptr;
  hipError_t e = hipSetDevice(ctx->device);
  if (e == hipSuccess) e = hipMalloc((void**)&d_start, start.size() * sizeof(int32_t));
  if (e == hipSuccess) e = hipMalloc((void**)&d_list, list.size() * sizeof(int32_t));
  if (e == hipSuccess) e = hipMemcpy(d_start, start.data(), start.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_list, list.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    if (d_start) (void)hipFree(d_start);
    if (d_list) (void)hipFree(d_list);
    return (int)e;
  }
  set->ray_start = d_start; set->ray_tri = d_list; set->ray_grid = g;
  return DSIM_OK;
}

int dsim_depth_image(dsim_ctx* ctx, void* stream, dsim_view state, const dsim_obstacles* set, const dsim_camera_params* params,
                     int64_t n_cam, const int32_t* cam_index, const float* offset, const uint8_t* type_id, float* depth_out,
                     int32_t* seg_out) {
  if (!set) return DSIM_E_ARG;
  CamK a;
  int64_t blocks;
  const int rc = cam_fill(ctx, state, set, params, n_cam, cam_index, offset, type_id, depth_out, seg_out, &a, &blocks);
  if (rc) return rc;
  const hipStream_t st_ = (hipStream_t)stream;
  const bool lds = set->n_tri <= OBS_LDS_TRI;
  const size_t shm = lds ? (size_t)set->n_tri * 64 : 0;
  if (lds && seg_out) hipLaunchKernelGGL((k_depth_image<true, true>), dim3((unsigned)blocks), dim3(256), shm, st_, a);
  else if (lds) hipLaunchKernelGGL((k_depth_image<true, false>), dim3((unsigned)blocks), dim3(256), shm, st_, a);
  else if (seg_out) hipLaunchKernelGGL((k_depth_image<false, true>), dim3((unsigned)blocks), dim3(256), 0, st_, a);
  else hipLaunchKernelGGL((k_depth_image<false, false>), dim3((unsigned)blocks), dim3(256), 0, st_, a);
  return (int)hipGetLastError();
}

int64_t dsim_depth_image_drones_workspace(int64_t m, int32_t nx, int32_t ny) {
  return dsim_sphere_grid_workspace(m, nx, ny);
}

int dsim_depth_image_drones(dsim_ctx* ctx, void* stream, dsim_view state, const dsim_obstacles* set, const dsim_camera_params* params,
                            int64_t n_cam, const int32_t* cam_index, const float* offset, const uint8_t* type_id,
                            const dsim_camera_drones* drones, float* depth_out, int32_t* seg_out) {
  CamK a;
  int64_t blocks;
  int rc = cam_fill(ctx, state, set, params, n_cam, cam_index, offset, type_id, depth_out, seg_out, &a, &blocks);
  if (rc) return rc;
  const hipStream_t st_ = (hipStream_t)stream;
  rc = cam_drones_fill(ctx, st_, state, drones, &a.dr);
  if (rc) return rc;
  const bool tris = set != nullptr, lds = tris && set->n_tri <= OBS_LDS_TRI;
  const size_t shm = lds ? (size_t)set->n_tri * 64 : 0;
  const dim3 gr((unsigned)blocks), tb(256);
  if (lds && seg_out) hipLaunchKernelGGL((k_depth_image<true, true, true, true>), gr, tb, shm, st_, a);
  else if (lds) hipLaunchKernelGGL((k_depth_image<true, false, true, true>), gr, tb, shm, st_, a);
  else if (tris && seg_out) hipLaunchKernelGGL((k_depth_image<false, true, true, true>), gr, tb, 0, st_, a);
  else if (tris) hipLaunchKernelGGL((k_depth_image<false, false, true, true>), gr, tb, 0, st_, a);
  else if (seg_out) hipLaunchKernelGGL((k_depth_image<false, true, true, false>), gr, tb, 0, st_, a);
  else hipLaunchKernelGGL((k_depth_image<false, false, true, false>), gr, tb, 0, st_, a);
  return (int)hipGetLastError();
}

#ifdef DSIM_CAM_COUNT
// the measuring build only: triangle tests counted since the last call (synchronises the device)
int dsim_camera_tests(uint64_t* out) {
  if (!out) return DSIM_E_ARG;
  *out = 0;
  if (!g_cam_tests) return DSIM_OK;
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, g_cam_tests, sizeof(uint64_t), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemset(g_cam_tests, 0, sizeof(uint64_t));
  return (int)e;
}
#endif

}  // extern "C"
