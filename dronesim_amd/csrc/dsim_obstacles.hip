// Static-obstacle watch (dsim_obstacle_clearance): per-drone clearance between the vehicle's bounding sphere and a static soup
// of triangles, on a uniform 3-D grid of per-cell triangle lists (include/dronesim_amd.h).  Point against triangle soup; the
// drone-drone watch (dsim_downwash.hip, k_clearance_query) is point against points.  What the files this one includes share is
// stated here once: the region decision of a point against a triangle (tri_region: tri_dist2 for every watch, tri_closest for the
// witness), the tile frame with the one cell walk (obs_cell_walk: the body or the record index of the winner), the scenes' table
// as a kernel reads it (ScnK, scn_kargs), and the point kernel, which with the witness's arguments behind its own is the witness.
#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "dsim_kernels.h"
#include "dsim_obstacle_grid.h"

#define OBS_LDS_TRI 512          // sets up to this many triangles (32 KiB of records) are staged in LDS once per workgroup
#define OBS_MAX_BLOCKS 2048      // workgroups walk tiles of 256 drones grid-stride, so one staging serves many tiles

struct dsim_obstacles {
  float4* rec;                   // [n_tri][4]  (dsim_obs::records)
  int* cell_start;               // [cells + 1]
  int* cell_tri;                 // [list_len]
  int n_tri;
  dsim_obstacle_grid grid;
  // the ray grid (dsim_obstacles_enable_rays; dsim_camera.hip): null until enabled.  The soup is kept on the host for it.
  int* ray_start;
  int* ray_tri;
  dsim_obstacle_grid ray_grid;
  std::vector<float> tri_host;
  int n_bodies;                  // 1 + the largest body index (obstacle scenes number a hit g * n_bodies + body)
};

// Obstacle scenes (dsim_scenes_create; dsim_scenes.hip): K scenes of up to G placements of one prototype set.  One 64-byte record
// per slot: (c_task.xyz, r_cull) — the centre of the prototype's box placed into the task frame and the radius outside which the
// placement is out of every query's reach, -inf for a slot at or above its scene's count — then R's three columns, each
// followed by one component of t: the local point is (col_k . (q - t))_k = R^T (q - t).
struct dsim_scenes {
  const dsim_obstacles* proto;
  float4* place;                 // [K][G][4]
  long long K;
  int G;
  float box_c[3];                // the centre of the prototype's box in its own frame (what c_task is the placed image of)
  // the motion (dsim_scenes_motion_set; dsim_scene_motion.hip): both null until one is attached
  float4* motion = nullptr;      // [K][G][4]: the motion records, the `moving` flag and r_cull in their padding
  float4* base = nullptr;        // [K][G][4]: the table as dsim_scenes_create wrote it
};

// ... and as every placed kernel reads them (the point watch and the witness, the camera, the scanner), with the scene of every drone
struct ScnK {
  const float4* place;           // [K][G][4]
  const int* scene_id;           // [n_pad], storage order
  long long K;
  int G, n_bodies;
};
static int scn_kargs(const dsim_scenes* scenes, const int32_t* scene_id, ScnK* s) {
  if (!scenes || !scene_id) return DSIM_E_ARG;
  s->place = scenes->place; s->scene_id = scene_id; s->K = scenes->K; s->G = scenes->G; s->n_bodies = scenes->proto->n_bodies;
  return DSIM_OK;
}

struct ObsK {
  KView st;
  long long n, n_pad, tiles;
  const float* offset;           // SoA [3][n_pad] or null
  const uint8_t* type_id;        // or null: type 0
  const DevType* types;
  int n_types;
  const float4* rec;
  const int* cell_start;
  const int* cell_tri;
  int n_tri;
  float ox, oy, oz, inv_cell;
  int nx, ny, nz;
  float lox, loy, loz, hix, hiy, hiz;     // the grown box: outside it no triangle is within reach
  float margin;
  float* clearance;              // [n_pad]
  int* nearest;                  // [n_pad] or null
  unsigned long long* counters;  // the ctx's (DSIM_Q_OBSTACLE_CONTACTS: DSIM_OBST_SHARDS shards behind the drone watch's)
  unsigned long long* contacts_out;
};

// The whole set's records into LDS, by the 256 lanes of a workgroup (the watches, the camera and the scanner: sets of up to
// OBS_LDS_TRI triangles).  Every lane of the workgroup calls it, under a uniform condition that is the caller's: it ends in a barrier.
__device__ __forceinline__ void obs_stage(float4* s_rec, const float4* rec, int n_tri) {
  for (int k = threadIdx.x; k < 4 * n_tri; k += 256) s_rec[k] = rec[k];
  __syncthreads();
}

// The region of q against one triangle record (Ericson, Real-Time Collision Detection 5.1.5, without branches: every lane of a
// wave meets another region), decided in ONE place for the squared distance, which it returns, and for the closest point, which
// it gives with CLOSEST as the vector from q to it (`to`, else null): the witness is right because it reads the decision the
// distance was taken on.  The vertex and edge regions give barycentric (v, w) of the closest point a + v ab + w ac, and
// e = p - v ab - w ac points from it to q; in the face region the distance is |h| = |n . p| with the record's unit normal, which
// does not lose digits in the quotient vb / (va + vb + vc) of a thin triangle, and the point is q - h n.  A point that fp32
// rounding puts on the wrong side of a region border gets the neighbouring region's formula, which agrees with its own to second
// order in the distance from the border.
template <bool CLOSEST>
__device__ __forceinline__ float tri_region(const float4 r0, const float4 r1, const float4 r2, const float4 r3, float qx, float qy,
                                            float qz, float3* to) {
  const float ax = r0.x, ay = r0.y, az = r0.z, abx = r0.w, aby = r1.x, abz = r1.y, acx = r1.z, acy = r1.w, acz = r2.x;
  const float nx = r2.y, ny = r2.z, nz = r2.w, e00 = r3.x, e01 = r3.y, e11 = r3.z;
  const float px = qx - ax, py = qy - ay, pz = qz - az;
  const float d1 = abx * px + aby * py + abz * pz, d2 = acx * px + acy * py + acz * pz;
  const float d3 = d1 - e00, d4 = d2 - e01, d5 = d1 - e01, d6 = d2 - e11;
  const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  const float d43 = d4 - d3, d56 = d5 - d6;
  const bool rA = d1 <= 0.0f && d2 <= 0.0f;
  const bool rB = d3 >= 0.0f && d4 <= d3;
  const bool rAB = vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f;
  const bool rC = d6 >= 0.0f && d5 <= d6;
  const bool rAC = vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f;
  const bool rBC = va <= 0.0f && d43 >= 0.0f && d56 >= 0.0f;
  // in the order of the book: the first region that holds decides
  float num = 0.0f, den = 1.0f;        // the one quotient: AB d1 / (d1 - d3), AC d2 / (d2 - d6), BC (d4 - d3) / ((d4 - d3) + (d5 - d6))
  int mode = 6;                        // 0 A, 1 B, 2 AB, 3 C, 4 AC, 5 BC, 6 face
  if (rBC) { mode = 5; num = d43; den = d43 + d56; }
  if (rAC) { mode = 4; num = d2; den = d2 - d6; }
  if (rC) mode = 3;
  if (rAB) { mode = 2; num = d1; den = d1 - d3; }
  if (rB) mode = 1;
  if (rA) mode = 0;
  const float t = den > 0.0f ? num * DSIM_RCP(den) : 0.0f;
  const float v = mode == 1 ? 1.0f : (mode == 2 ? t : (mode == 5 ? 1.0f - t : 0.0f));
  const float w = mode == 3 ? 1.0f : (mode == 4 || mode == 5 ? t : 0.0f);
  const float ex = px - v * abx - w * acx, ey = py - v * aby - w * acy, ez = pz - v * abz - w * acz;
  const float h = nx * px + ny * py + nz * pz;
  if constexpr (CLOSEST) {
    to->x = mode == 6 ? -(h * nx) : -ex;
    to->y = mode == 6 ? -(h * ny) : -ey;
    to->z = mode == 6 ? -(h * nz) : -ez;
  }
  return mode == 6 ? h * h : ex * ex + ey * ey + ez * ez;
}

// Squared distance from q to one triangle record.
__device__ __forceinline__ float tri_dist2(const float4 r0, const float4 r1, const float4 r2, const float4 r3, float qx, float qy,
                                           float qz) {
  return tri_region<false>(r0, r1, r2, r3, qx, qy, qz, nullptr);
}

// ---- the tile frame of the three watch kernels (k_obstacle_clearance, k_obstacle_clearance_scenes, k_obstacle_sweep) ----------------
// One drone per lane, tiles of 256 drones grid-stride.  Per tile every kernel loads its lane's drone (the point kernels: obs_lane),
// decides per lane what it has to look at, stages the records once the workgroup meets a tile that needs them (obs_stage_once),
// searches, and hands the lane's answer to obs_lane_store.  The search is each kernel's own; where it walks a cell's list it is
// obs_cell_walk.

// A live lane's drone for the point kernels: the query point q = position - offset and the bounding sphere's radius.  Called
// inside the kernel's `if (live)`, beside the loads that are the kernel's own; a dead lane keeps the zeros.  (The swept kernel
// reads and writes prev between the position and the offset and keeps its own load: dsim_sweep.hip.)
struct ObsLane { float qx, qy, qz, R; };
__device__ __forceinline__ ObsLane obs_lane(const ObsK& a, long long i) {
  ObsLane l;
  const long long o = kv_off(a.st, i);
  l.qx = a.st.base[o]; l.qy = a.st.base[o + a.st.field_stride]; l.qz = a.st.base[o + 2 * a.st.field_stride];
  if (a.offset) { l.qx -= a.offset[i]; l.qy -= a.offset[a.n_pad + i]; l.qz -= a.offset[2 * a.n_pad + i]; }
  l.R = a.types[a.type_id ? min((int)a.type_id[i], a.n_types - 1) : 0].coll_sphere;
  return l;
}

// The records into LDS before the workgroup's first tile with a lane that wants them (`want` is the caller's; every lane calls).
template <bool LDS>
__device__ __forceinline__ void obs_stage_once(const ObsK& a, float4* s_rec, bool& staged, bool want) {
  if (LDS) {
    if (!staged && __syncthreads_or(want ? 1 : 0)) {
      obs_stage(s_rec, a.rec, a.n_tri);
      staged = true;
    }
  }
}

// The lane's answer — (c_i, body) within the margin, else (margin, -1) — and the wave's contacts: one ballot, one atomic per
// counter (the ctx's shard of the tile, and contacts_out).
__device__ __forceinline__ void obs_lane_store(const ObsK& a, long long tile, long long i, bool live, bool in, float c_i, int body) {
  if (live) {
    a.clearance[i] = in ? c_i : a.margin;
    if (a.nearest) a.nearest[i] = in ? body : -1;
  }
  const unsigned long long hit = __ballot(in && c_i < 0.0f);
  if (hit != 0ULL && (threadIdx.x & 63u) == 0u) {
    const unsigned long long cnt = (unsigned long long)__popcll(hit);
    atomicAdd(&a.counters[8 + DSIM_GROUND_SHARDS + DSIM_DRONE_SHARDS + (tile & (DSIM_OBST_SHARDS - 1))], cnt);
    if (a.contacts_out) atomicAdd(a.contacts_out, cnt);
  }
}

// The cell of q and the walk of its list (the set's frame, or a placement's): the least dist2(r0, r1, r2, r3) below `best` over
// the list's records and the body of the triangle that attains it — with INDEX its record index instead (the witness, which
// reads that one record again behind the walk; the watches never carry an index).  The records come from LDS when the whole set
// was staged.
template <bool LDS, bool INDEX = false, class Dist2>
__device__ __forceinline__ void obs_cell_walk(const ObsK& a, const float4* s_rec, float qx, float qy, float qz, Dist2 dist2, int& body,
                                              float& best) {
  const int cx = min(max((int)floorf((qx - a.ox) * a.inv_cell), 0), a.nx - 1);
  const int cy = min(max((int)floorf((qy - a.oy) * a.inv_cell), 0), a.ny - 1);
  const int cz = min(max((int)floorf((qz - a.oz) * a.inv_cell), 0), a.nz - 1);
  const int c = (cz * a.ny + cy) * a.nx + cx;
  const int end = a.cell_start[c + 1];
  for (int k = a.cell_start[c]; k < end; ++k) {
    const int t = a.cell_tri[k];
    const float4* r = (LDS ? s_rec : a.rec) + 4 * t;
    const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
    const float d2 = dist2(r0, r1, r2, r3);
    const bool better = d2 < best;
    best = better ? d2 : best;
    body = better ? (INDEX ? t : __float_as_int(r3.w)) : body;
  }
}

// ... for the point q itself (both point kernels, with and without the witness)
template <bool LDS, bool INDEX>
__device__ __forceinline__ void obs_point_walk(const ObsK& a, const float4* s_rec, float qx, float qy, float qz, int& body, float& best) {
  obs_cell_walk<LDS, INDEX>(a, s_rec, qx, qy, qz,
                            [=](const float4 r0, const float4 r1, const float4 r2, const float4 r3) { return tri_dist2(r0, r1, r2, r3, qx, qy, qz); },
                            body, best);
}

// The witness's tail of both point kernels (dsim_witness.hip, which this file includes behind them: its entry points launch them).
struct WitK;
template <bool LDS>
__device__ __forceinline__ int wit_point(const ObsK& a, const float4* s_rec, int tri, float lx, float ly, float lz, float& wx, float& wy,
                                         float& wz);
__device__ __forceinline__ void wit_lane_store(const ObsK& a, const WitK& w, long long i, bool live, bool in, float wx, float wy, float wz,
                                               int tri);

// The point watch.  A tile none of whose drones lies in the grown box reads its positions (and offsets) and writes (margin, -1);
// of a tile that has some, the waves that have none do the same.  The others look up their cell and walk its list: the records
// come from LDS when the whole set fits, else through L2 — the set is read-only and small next to the fleet.
// Instantiated with Wit = WitK, the witness's arguments behind the watch's, it is the witness (dsim_witness.hip; the watch itself
// has an empty Wit and its own argument only): the same frame, decisions and walk order, the walk keeping the winner's record
// index, on which the lanes within the margin evaluate tri_closest once.
template <bool LDS, class... Wit>
__global__ __launch_bounds__(256) void k_obstacle_clearance(ObsK a, Wit... w) {
  constexpr bool WIT = sizeof...(Wit) != 0;
  extern __shared__ float4 s_rec[];
  bool staged = false;
  for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const long long i = tile * 256 + threadIdx.x;
    const bool live = i < a.n;
    ObsLane l = {};
    if (live) l = obs_lane(a, i);
    const float qx = l.qx, qy = l.qy, qz = l.qz, R = l.R;
    // (a NaN position fails every comparison: not in the box, clearance = margin)
    const bool inbox = live && R > 0.0f && qx >= a.lox && qx <= a.hix && qy >= a.loy && qy <= a.hiy && qz >= a.loz && qz <= a.hiz;
    obs_stage_once<LDS>(a, s_rec, staged, inbox);
    float best = INFINITY;
    int win = -1;                        // the winner's body; with WIT its record index
    if (inbox) obs_point_walk<LDS, WIT>(a, s_rec, qx, qy, qz, win, best);   // (a wave with no such lane skips it: the per-wave reject)
    const float c_i = DSIM_SQRT(best) - R;
    const bool in = (WIT ? win >= 0 : inbox) && c_i < a.margin;           // (the same lanes: c_i < margin needs a winner)
    if constexpr (WIT) {
      float wx = 0.0f, wy = 0.0f, wz = 0.0f;
      int body = -1;
      if (in) body = wit_point<LDS>(a, s_rec, win, qx, qy, qz, wx, wy, wz);
      obs_lane_store(a, tile, i, live, in, c_i, body);
      wit_lane_store(a, w..., i, live, in, wx, wy, wz, win);
    } else {
      obs_lane_store(a, tile, i, live, in, c_i, win);
    }
  }
}

// what both queries of the set hand their kernels: the fleet, the set's records and grid, the outputs and the counters
static int obs_kargs(dsim_ctx* ctx, int64_t n, const dsim_view& state, const dsim_obstacles* set, const float* offset,
                     const uint8_t* type_id, float margin, float* clearance_out, int32_t* nearest_out, uint64_t* contacts_out, ObsK* k) {
  ObsK& a = *k;
  const int rc = make_kview(state, 3, &a.st);
  if (rc) return rc;
  const dsim_obstacle_grid& g = set->grid;
  a.n = n; a.n_pad = state.n_pad; a.tiles = (n + 255) / 256;
  a.offset = offset; a.type_id = type_id; a.types = ctx->d_types; a.n_types = ctx->n_types;
  a.rec = set->rec; a.cell_start = set->cell_start; a.cell_tri = set->cell_tri; a.n_tri = set->n_tri;
  a.ox = g.origin[0]; a.oy = g.origin[1]; a.oz = g.origin[2]; a.inv_cell = 1.0f / g.cell;
  a.nx = g.nx; a.ny = g.ny; a.nz = g.nz;
  a.lox = g.lo[0]; a.loy = g.lo[1]; a.loz = g.lo[2]; a.hix = g.hi[0]; a.hiy = g.hi[1]; a.hiz = g.hi[2];
  a.margin = margin; a.clearance = clearance_out; a.nearest = nearest_out;
  a.counters = ctx->d_counters; a.contacts_out = (unsigned long long*)contacts_out;
  return DSIM_OK;
}

// what the three watch launchers refuse alike (`extra` widens every radius: the swept watch's sag)
static int obs_refuse(const dsim_ctx* ctx, int64_t n, const dsim_view& state, const dsim_obstacles* set, const uint8_t* type_id,
                      float margin, float extra, const float* clearance_out) {
  if (!ctx || !set || !clearance_out || !(margin > 0.0f) || n <= 0 || n > state.n_pad) return DSIM_E_ARG;
  if (ctx->n_types > 1 && !type_id) return DSIM_E_ARG;
  if ((double)ctx_r_max(ctx) + (double)extra + (double)margin > (double)set->grid.reach) return DSIM_E_ARG;
  return DSIM_OK;
}

static inline unsigned obs_blocks(long long tiles) { return (unsigned)(tiles < OBS_MAX_BLOCKS ? tiles : OBS_MAX_BLOCKS); }

// one watch kernel over the fleet's tiles: the instance that stages the set in LDS when it fits, else the one that reads it through L2
template <class... Args>
static int obs_launch(void (*k_lds)(Args...), void (*k_l2)(Args...), const dsim_obstacles* set, long long tiles, void* stream,
                      const Args&... args) {
  const hipStream_t st_ = (hipStream_t)stream;
  if (set->n_tri <= OBS_LDS_TRI)
    hipLaunchKernelGGL(k_lds, dim3(obs_blocks(tiles)), dim3(256), (size_t)set->n_tri * 64, st_, args...);
  else
    hipLaunchKernelGGL(k_l2, dim3(obs_blocks(tiles)), dim3(256), 0, st_, args...);
  return (int)hipGetLastError();
}

extern "C" {

int dsim_obstacle_grid_plan(const float* tri, int64_t n_tri, float reach, dsim_obstacle_grid* out) {
  return dsim_obs::plan(tri, n_tri, reach, out);
}

int dsim_obstacle_grid_build(const float* tri, int64_t n_tri, const dsim_obstacle_grid* g, int32_t* cell_start, int32_t* cell_tri) {
  return dsim_obs::build(tri, n_tri, g, cell_start, cell_tri);
}

int dsim_obstacles_create(dsim_ctx* ctx, const float* tri_host, const int32_t* body_host, int64_t n_tri, float reach,
                          dsim_obstacles** out) {
  if (!ctx || !out) return DSIM_E_ARG;
  dsim_obstacle_grid g;
  int rc = dsim_obs::plan(tri_host, n_tri, reach, &g);
  if (rc) return rc;
  if (body_host) for (int64_t t = 0; t < n_tri; ++t) if (body_host[t] < 0) return DSIM_E_ARG;
  const int64_t cells = (int64_t)g.nx * g.ny * g.nz;
  std::vector<int32_t> start, list;
  std::vector<float> rec;
  try {
    start.resize(cells + 1); list.resize(g.list_len > 0 ? g.list_len : 1); rec.resize(DSIM_OBS_REC_FLOATS * n_tri);
  } catch (const std::bad_alloc&) { return (int)hipErrorOutOfMemory; }
  rc = dsim_obs::build(tri_host, n_tri, &g, start.data(), list.data());
  if (rc) return rc;
  dsim_obs::records(tri_host, body_host, n_tri, rec.data());
  dsim_obstacles* s = new (std::nothrow) dsim_obstacles();
  if (!s) return (int)hipErrorOutOfMemory;
  s->rec = nullptr; s->cell_start = nullptr; s->cell_tri = nullptr; s->n_tri = (int)n_tri; s->grid = g;
  s->ray_start = nullptr; s->ray_tri = nullptr; s->n_bodies = 1;
  if (body_host) for (int64_t t = 0; t < n_tri; ++t) if (body_host[t] >= s->n_bodies) s->n_bodies = body_host[t] + 1;
  try { s->tri_host.assign(tri_host, tri_host + 9 * n_tri); } catch (const std::bad_alloc&) { delete s; return (int)hipErrorOutOfMemory; }
  hipError_t e = hipSetDevice(ctx->device);           // (as dsim_dev_alloc: the set lives where the ctx's streams run)
  if (e == hipSuccess) e = hipMalloc((void**)&s->rec, rec.size() * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&s->cell_start, start.size() * sizeof(int32_t));
  if (e == hipSuccess) e = hipMalloc((void**)&s->cell_tri, list.size() * sizeof(int32_t));
  if (e == hipSuccess) e = hipMemcpy(s->rec, rec.data(), rec.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(s->cell_start, start.data(), start.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(s->cell_tri, list.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) { (void)dsim_obstacles_destroy(ctx, s); return (int)e; }
  *out = s;
  return DSIM_OK;
}

int dsim_obstacles_destroy(dsim_ctx* ctx, dsim_obstacles* set) {
  (void)ctx;                                          // (may be NULL: a set may outlive the ctx it was made through)
  if (!set) return DSIM_OK;
  hipError_t e = hipSuccess, f;                       // (hipFree waits for the work that may still read the set)
  if (set->rec && (f = hipFree(set->rec)) != hipSuccess) e = f;
  if (set->cell_start && (f = hipFree(set->cell_start)) != hipSuccess) e = f;
  if (set->cell_tri && (f = hipFree(set->cell_tri)) != hipSuccess) e = f;
  if (set->ray_start && (f = hipFree(set->ray_start)) != hipSuccess) e = f;
  if (set->ray_tri && (f = hipFree(set->ray_tri)) != hipSuccess) e = f;
  delete set;
  return (int)e;
}

int dsim_obstacle_clearance(dsim_ctx* ctx, void* stream, int64_t n, dsim_view state, const dsim_obstacles* set,
                            const float* offset, const uint8_t* type_id, float margin,
                            float* clearance_out, int32_t* nearest_out, uint64_t* contacts_out) {
  int rc = obs_refuse(ctx, n, state, set, type_id, margin, 0.0f, clearance_out);
  if (rc) return rc;
  ObsK a;
  rc = obs_kargs(ctx, n, state, set, offset, type_id, margin, clearance_out, nearest_out, contacts_out, &a);
  if (rc) return rc;
  return obs_launch(k_obstacle_clearance<true>, k_obstacle_clearance<false>, set, a.tiles, stream, a);
}

}  // extern "C"

// the depth camera: the second consumer of the set (it shares the set's private record above and the LDS threshold)
#include "dsim_camera.hip"

// the swept watch: the chord between two samples against the same set (it shares the record, tri_dist2 and the LDS threshold)
#include "dsim_sweep.hip"

// obstacle scenes: per-drone placements of one set for the watch and the camera (they share the cell walk and the camera's kernel)
#include "dsim_scenes.hip"

// the range scanner: per-drone beam fans against the set, the scenes, the plane and the drones (it shares the camera's walk and records)
#include "dsim_scan.hip"

// line of sight: per-drone segments to the neighbours a knn record names, against the set, the scenes and the plane (it shares the
// camera's walk and records and the scanner's spreading of a small fleet)
#include "dsim_sight.hip"

// the gate passage watch: the chord between two samples against one aperture per placement (it shares the tile frame and the scenes)
#include "dsim_passage.hip"

// moving scenes: per-placement motion that rewrites the scenes' table in stream order (every placed kernel above reads it per launch)
#include "dsim_scene_motion.hip"

// corridor clearance: k candidate segments per drone as swept spheres against the set, the scenes where they stand and the ground
// (it shares the swept watch's segment arithmetic and pieces, the scenes' frames and line of sight's per-slot mapping)
#include "dsim_corridor.hip"

// the obstacle witness: the point watch with the vector to the closest point (both point kernels above are its kernels too; the
// file holds the tail they call, its arguments and its entry points)
#include "dsim_witness.hip"

// obstacle witnesses: the m closest bodies per drone, each with its vector (it shares the tile frame, the scenes' cull and the
// witness's tail steps; its kernels keep a sorted list of per-body minima where the point kernels keep one)
#include "dsim_witnesses.hip"
