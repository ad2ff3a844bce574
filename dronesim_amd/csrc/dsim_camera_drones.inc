// The walk of the drones' grid of k_depth_image<DRONES> (dsim_camera.hip) and k_range_scan<DRONES> (dsim_scan.hip), as text: as a
// function it compiled to other instruction sequences in every DRONES instance (DESIGN.md, "Range scanner").  The drones against
// the ray w + t d (w in the WORLD frame), for hits in [near, min(a.far, a.dr.range)] nearer than `best`, by a 2-D DDA over the
// grid's xy cells.  Cells are 2 R_max or more: a sphere whose centre lies in a cell reaches into adjacent cells only, so the spheres
// of the 3 x 3 block around the ray's cell are all that can be hit inside it — the whole block at the first cell, the three newly
// adjacent cells after every step — and the walk stops as soon as best is not beyond the cell's exit.  The box the ray is clipped
// to is the grid's grown by one ring of (empty) cells: a sphere of a border cell reaches outside the grid's box.  Then the outside
// list.  The includer defines CD_GATE (the lanes that cast); `a.far`, `a.dr` (CamDr), `i` (the lane's drone in storage order: it is
// never hit), `wx` .. `wz`, `dx` .. `dz`, `near`, `best` and `body` are the kernel's (and `n_tests` in the counting build).  A block
// of its own, as the triangle walk is.  The sphere test is CD_SPHERE(p, idx, k): cam_sphere on the walk's own names unless the
// includer defines another (line of sight: a solid ball and the slot's target left out, dsim_sight.hip).
#ifndef CD_SPHERE
#define CD_SPHERE(p, idx, k) cam_sphere(p, idx, k, own, wx, wy, wz, dx, dy, dz, inv_a, near, tmax, best, body)
#endif
{
  const SphereGrid& g = a.dr.g;
  const float tmax = fminf(a.far, a.dr.range);
  const float inv_a = 1.0f / (dx * dx + dy * dy + dz * dz);
  const long long i_w = i + g.local_offset;
  const int own = i_w < 0x7fffffffLL ? (int)i_w : -1;
  const float ix_ = 1.0f / dx, iy_ = 1.0f / dy;
  const float gx0 = g.xmin - g.cell, gx1 = g.xmin + (float)(g.nx + 1) * g.cell;
  const float gy0 = g.ymin - g.cell, gy1 = g.ymin + (float)(g.ny + 1) * g.cell;
  const float sx0 = (gx0 - wx) * ix_, sx1 = (gx1 - wx) * ix_;
  const float sy0 = (gy0 - wy) * iy_, sy1 = (gy1 - wy) * iy_;
  const float s_in = fmaxf(fmaxf(fminf(sx0, sx1), fminf(sy0, sy1)), near);
  const float s_out = fminf(fminf(fmaxf(sx0, sx1), fmaxf(sy0, sy1)), fminf(tmax, best));   // (starts from the triangle hit)
  const bool in_x = dx != 0.0f || (wx >= gx0 && wx <= gx1);
  const bool in_y = dy != 0.0f || (wy >= gy0 && wy <= gy1);
  if (CD_GATE && s_in <= s_out && in_x && in_y) {
    // cell indices -1 .. nx (ny): the ring included; the blocks below are clamped to the cells that exist
    const float qx = wx + s_in * dx, qy = wy + s_in * dy;
    int cx = min(max((int)floorf((qx - gx0) * g.inv_cell), 0), g.nx + 1) - 1;
    int cy = min(max((int)floorf((qy - gy0) * g.inv_cell), 0), g.ny + 1) - 1;
    const int stx = dx > 0.0f ? 1 : -1, sty = dy > 0.0f ? 1 : -1;
    const float dtx = dx != 0.0f ? g.cell * fabsf(ix_) : INFINITY;
    const float dty = dy != 0.0f ? g.cell * fabsf(iy_) : INFINITY;
    float tmx = dx != 0.0f ? (gx0 + (float)(cx + 1 + (dx > 0.0f ? 1 : 0)) * g.cell - wx) * ix_ : INFINITY;
    float tmy = dy != 0.0f ? (gy0 + (float)(cy + 1 + (dy > 0.0f ? 1 : 0)) * g.cell - wy) * iy_ : INFINITY;
    int bx0 = cx - 1, bx1 = cx + 1, by0 = cy - 1, by1 = cy + 1;           // the block to test: 3 x 3 at the first cell
    const int max_cells = g.nx + g.ny + 4;
    for (int it = 0; it < max_cells; ++it) {
      const int xlo = max(bx0, 0), xhi = min(bx1, g.nx - 1), yhi = min(by1, g.ny - 1);
      if (xlo <= xhi) {
        for (int yy = max(by0, 0); yy <= yhi; ++yy) {                      // a row of the block is one run of sorted[]
          const int end = g.cell_start[yy * g.nx + xhi + 1];
          for (int k = g.cell_start[yy * g.nx + xlo]; k < end; ++k) {
            CD_SPHERE(g.sorted[k], g.sidx, k);
#ifdef DSIM_CAM_COUNT
            ++n_tests;
#endif
          }
        }
      }
      const float t_exit = fminf(tmx, tmy);
      if (best <= t_exit || t_exit >= s_out) break;          // nothing nearer can lie in a later cell / the ray leaves the box (dx = dy = 0: at once)
      const bool gx = tmx <= tmy;
      cx += gx ? stx : 0; cy += gx ? 0 : sty;
      tmx += gx ? dtx : 0.0f; tmy += gx ? 0.0f : dty;
      if (cx < -1 || cx > g.nx || cy < -1 || cy > g.ny) break;
      bx0 = gx ? cx + stx : cx - 1; bx1 = gx ? cx + stx : cx + 1;          // the newly adjacent column or row
      by0 = gx ? cy - 1 : cy + sty; by1 = gx ? cy + 1 : cy + sty;
    }
  }
  if (CD_GATE) {                                             // drones outside the grid's box: every ray, the list is short
    const int n_out = *g.outside_n;
    for (int k = 0; k < n_out; ++k)
      CD_SPHERE(g.outside[k], g.outside_idx, k);
  }
}
#undef CD_GATE
#undef CD_SPHERE
