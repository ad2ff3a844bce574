// Static-obstacle watch, host side: the uniform 3-D grid around a triangle soup and the per-triangle records of the query.
// Plain C++ (no HIP, no device): dsim_obstacles.hip includes it, and so may a host-only program (sanitiser runs, tools).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/dronesim_amd.h"

#define DSIM_OBS_MAX_TRI 65536
#define DSIM_OBS_MAX_CELLS (1 << 18)
#define DSIM_OBS_MAX_LIST (1LL << 26)
#define DSIM_OBS_MAX_AXIS 4096
#define DSIM_OBS_MIN_AREA 1e-12
#define DSIM_OBS_REC_FLOATS 16          // one record: 64 bytes, four 16-byte loads

namespace dsim_obs {

// nothing written unless every triangle passes: finite coordinates, area >= DSIM_OBS_MIN_AREA (fp64, on the fp32 vertices)
static inline bool soup_ok(const float* tri, int64_t n_tri, float reach) {
  if (!tri || n_tri < 1 || n_tri > DSIM_OBS_MAX_TRI || !(reach > 0.0f) || !isfinite(reach)) return false;
  for (int64_t t = 0; t < n_tri; ++t) {
    const float* v = tri + 9 * t;
    for (int k = 0; k < 9; ++k) if (!isfinite(v[k])) return false;
    const double ab[3] = {(double)v[3] - v[0], (double)v[4] - v[1], (double)v[5] - v[2]};
    const double ac[3] = {(double)v[6] - v[0], (double)v[7] - v[1], (double)v[8] - v[2]};
    const double nx = ab[1] * ac[2] - ab[2] * ac[1], ny = ab[2] * ac[0] - ab[0] * ac[2], nz = ab[0] * ac[1] - ab[1] * ac[0];
    if (!(0.5 * sqrt(nx * nx + ny * ny + nz * nz) >= DSIM_OBS_MIN_AREA)) return false;
  }
  return true;
}

// The cells a triangle is listed in: those its bounding box, grown by reach and the slack, touches.  A cell with a point closer
// than reach to the triangle is closer than reach to the triangle's box on every axis, so it is among them (over-inclusive: the
// corners of the grown box are further away than reach).  The slack, a hundredth of a cell, covers the fp32 rounding of the
// device's own floor((q - origin) / cell) at a cell face: a few ulps of an index below DSIM_OBS_MAX_AXIS, 2^-11 of a cell.
struct CellRange { int lo[3], hi[3]; };
static inline CellRange cells_of(const float* v, const dsim_obstacle_grid& g) {
  const int nn[3] = {g.nx, g.ny, g.nz};
  const double grow = (double)g.reach + 1e-2 * (double)g.cell;
  CellRange r;
  for (int k = 0; k < 3; ++k) {
    const double lo = fmin(fmin(v[k], v[3 + k]), v[6 + k]) - grow, hi = fmax(fmax(v[k], v[3 + k]), v[6 + k]) + grow;
    const double a = floor((lo - (double)g.origin[k]) / (double)g.cell), b = floor((hi - (double)g.origin[k]) / (double)g.cell);
    r.lo[k] = (int)fmin(fmax(a, 0.0), (double)(nn[k] - 1));
    r.hi[k] = (int)fmin(fmax(b, 0.0), (double)(nn[k] - 1));
  }
  return r;
}
static inline int64_t cells_in(const CellRange& r) {
  return (int64_t)(r.hi[0] - r.lo[0] + 1) * (r.hi[1] - r.lo[1] + 1) * (r.hi[2] - r.lo[2] + 1);
}

// the grid for cell edge `cell`; false when it has more cells than the cap
static inline bool grid_at(const double lo[3], const double hi[3], double cell, float reach, dsim_obstacle_grid* g) {
  int n[3];
  double cells = 1.0;
  for (int k = 0; k < 3; ++k) {
    const double c = floor((hi[k] - lo[k]) / cell) + 1.0;
    cells *= c;
    if (c > (double)DSIM_OBS_MAX_AXIS) return false;
    n[k] = (int)c;
  }
  if (cells > (double)DSIM_OBS_MAX_CELLS) return false;
  for (int k = 0; k < 3; ++k) { g->origin[k] = (float)lo[k]; g->lo[k] = (float)lo[k]; g->hi[k] = (float)hi[k]; }
  g->cell = (float)cell; g->nx = n[0]; g->ny = n[1]; g->nz = n[2]; g->reach = reach; g->list_len = 0;
  return true;
}

static inline int plan(const float* tri, int64_t n_tri, float reach, dsim_obstacle_grid* out) {
  if (!out || !soup_ok(tri, n_tri, reach)) return DSIM_E_ARG;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t t = 0; t < n_tri; ++t)
    for (int k = 0; k < 9; ++k) { lo[k % 3] = fmin(lo[k % 3], tri[9 * t + k]); hi[k % 3] = fmax(hi[k % 3], tri[9 * t + k]); }
  // the grown box in fp32, rounded OUTWARDS: the device rejects against these very numbers
  for (int k = 0; k < 3; ++k) {
    lo[k] = (double)nextafterf((float)(lo[k] - (double)reach), -INFINITY);
    hi[k] = (double)nextafterf((float)(hi[k] + (double)reach), INFINITY);
    if (!isfinite(lo[k]) || !isfinite(hi[k])) return DSIM_E_ARG;
  }
  double cell = 0.5 * (double)reach;
  for (int tries = 0; tries < 64; ++tries, cell *= 2.0) {
    dsim_obstacle_grid g;
    memset(&g, 0, sizeof(g));
    if (!grid_at(lo, hi, cell, reach, &g)) continue;
    int64_t len = 0;
    for (int64_t t = 0; t < n_tri && len <= DSIM_OBS_MAX_LIST; ++t) len += cells_in(cells_of(tri + 9 * t, g));
    if (len > DSIM_OBS_MAX_LIST) continue;
    g.list_len = len;
    *out = g;
    return DSIM_OK;
  }
  return DSIM_E_ARG;
}

// count, prefix sum, fill for the grid `p` (cells_of decides where a triangle is listed): triangles ascend inside a cell because
// they are visited in order
static inline void fill_lists(const float* tri, int64_t n_tri, const dsim_obstacle_grid& p, int32_t* cell_start, int32_t* cell_tri) {
  const int64_t cells = (int64_t)p.nx * p.ny * p.nz;
  for (int64_t c = 0; c <= cells; ++c) cell_start[c] = 0;
  for (int pass = 0; pass < 2; ++pass) {
    for (int64_t t = 0; t < n_tri; ++t) {
      const CellRange r = cells_of(tri + 9 * t, p);
      for (int z = r.lo[2]; z <= r.hi[2]; ++z)
        for (int y = r.lo[1]; y <= r.hi[1]; ++y)
          for (int x = r.lo[0]; x <= r.hi[0]; ++x) {
            const int64_t c = ((int64_t)z * p.ny + y) * p.nx + x;
            if (pass == 0) ++cell_start[c + 1];
            else cell_tri[cell_start[c]++] = (int32_t)t;
          }
    }
    if (pass == 0) {
      for (int64_t c = 0; c < cells; ++c) cell_start[c + 1] += cell_start[c];
    } else {                                                   // the fill moved every start to its cell's end: shift back
      for (int64_t c = cells; c > 0; --c) cell_start[c] = cell_start[c - 1];
      cell_start[0] = 0;
    }
  }
}

static inline int build(const float* tri, int64_t n_tri, const dsim_obstacle_grid* g, int32_t* cell_start, int32_t* cell_tri) {
  dsim_obstacle_grid p;
  if (!g || !cell_start || !cell_tri) return DSIM_E_ARG;
  const int rc = plan(tri, n_tri, g->reach, &p);
  if (rc) return rc;
  if (memcmp(&p, g, sizeof(p)) != 0) return DSIM_E_ARG;        // not this soup's plan: the arrays would have another size
  fill_lists(tri, n_tri, p, cell_start, cell_tri);
  return DSIM_OK;
}

// ---- the ray grid (dsim_depth_image) ---------------------------------------------------------------------------------------------
// A second grid of the same soup for ray traversal.  The watch grid lists a triangle in every cell within `reach` of it, which
// at the size of a gate is every cell; a ray walks cells and wants each list short.  Here reach = 0: a triangle is listed in the
// cells its own bounding box touches, grown by the same hundredth of a cell (cells_of), which covers the fp32 rounding of the
// device's cell walk at a cell face.  The box [lo, hi] is the soup's, grown by that slack of the first candidate edge and rounded
// outwards; the edge starts at diagonal / (2 cbrt(n_tri)) and is doubled until the caps hold.  one_cell: the whole box as ONE
// cell that lists every triangle (the brute-force baseline a measurement compares the grid against).
static inline int ray_plan(const float* tri, int64_t n_tri, bool one_cell, dsim_obstacle_grid* out) {
  if (!out || !soup_ok(tri, n_tri, 1.0f)) return DSIM_E_ARG;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t t = 0; t < n_tri; ++t)
    for (int k = 0; k < 9; ++k) { lo[k % 3] = fmin(lo[k % 3], tri[9 * t + k]); hi[k % 3] = fmax(hi[k % 3], tri[9 * t + k]); }
  const double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
  double cell = sqrt(dx * dx + dy * dy + dz * dz) / (2.0 * cbrt((double)n_tri));
  if (!(cell > 0.0) || !isfinite(cell)) return DSIM_E_ARG;
  const double pad = 1e-2 * cell;
  for (int k = 0; k < 3; ++k) {
    lo[k] = (double)nextafterf((float)(lo[k] - pad), -INFINITY);
    hi[k] = (double)nextafterf((float)(hi[k] + pad), INFINITY);
    if (!isfinite(lo[k]) || !isfinite(hi[k])) return DSIM_E_ARG;
  }
  if (one_cell) cell = 2.0 * fmax(fmax(hi[0] - lo[0], hi[1] - lo[1]), hi[2] - lo[2]);
  for (int tries = 0; tries < 64; ++tries, cell *= 2.0) {
    dsim_obstacle_grid g;
    memset(&g, 0, sizeof(g));
    if (!grid_at(lo, hi, cell, 0.0f, &g)) continue;
    if (!((double)g.cell * 1e-2 > 0.0) || !isfinite(g.cell)) return DSIM_E_ARG;
    int64_t len = 0;
    for (int64_t t = 0; t < n_tri && len <= DSIM_OBS_MAX_LIST; ++t) len += cells_in(cells_of(tri + 9 * t, g));
    if (len > DSIM_OBS_MAX_LIST) continue;
    g.list_len = len;
    *out = g;
    return DSIM_OK;
  }
  return DSIM_E_ARG;
}

static inline int ray_build(const float* tri, int64_t n_tri, bool one_cell, const dsim_obstacle_grid* g, int32_t* cell_start,
                            int32_t* cell_tri) {
  dsim_obstacle_grid p;
  if (!g || !cell_start || !cell_tri) return DSIM_E_ARG;
  const int rc = ray_plan(tri, n_tri, one_cell, &p);
  if (rc) return rc;
  if (memcmp(&p, g, sizeof(p)) != 0) return DSIM_E_ARG;        // not this soup's ray plan
  fill_lists(tri, n_tri, p, cell_start, cell_tri);
  return DSIM_OK;
}

// One record per triangle, rounded to fp32 from fp64 arithmetic on the fp32 vertices: a, ab, ac, the unit normal, then
// ab.ab, ab.ac, ac.ac (with d1 = ab.ap and d2 = ac.ap they give the other four dot products of the region test:
// d3 = d1 - ab.ab, d4 = d2 - ab.ac, d5 = d1 - ab.ac, d6 = d2 - ac.ac) and the body index, as its bits.
static inline void records(const float* tri, const int32_t* body, int64_t n_tri, float* rec) {
  for (int64_t t = 0; t < n_tri; ++t) {
    const float* v = tri + 9 * t;
    float* r = rec + DSIM_OBS_REC_FLOATS * t;
    double ab[3], ac[3];
    for (int k = 0; k < 3; ++k) { ab[k] = (double)v[3 + k] - v[k]; ac[k] = (double)v[6 + k] - v[k]; }
    double n[3] = {ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]};
    const double len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    for (int k = 0; k < 3; ++k) { r[k] = v[k]; r[3 + k] = (float)ab[k]; r[6 + k] = (float)ac[k]; r[9 + k] = (float)(n[k] / len); }
    r[12] = (float)(ab[0] * ab[0] + ab[1] * ab[1] + ab[2] * ab[2]);
    r[13] = (float)(ab[0] * ac[0] + ab[1] * ac[1] + ab[2] * ac[2]);
    r[14] = (float)(ac[0] * ac[0] + ac[1] * ac[1] + ac[2] * ac[2]);
    const int32_t b = body ? body[t] : 0;
    memcpy(&r[15], &b, sizeof(b));
  }
}

}  // namespace dsim_obs
