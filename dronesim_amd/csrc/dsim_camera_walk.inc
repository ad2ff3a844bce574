// The triangle walk of k_depth_image (dsim_camera.hip) and k_range_scan (dsim_scan.hip), as text: a kernel includes it once for the
// set in the task frame and once per placement of a scene (PLACED).  Text, not a function: as a function it compiled to other
// branch and compare sequences (DESIGN.md, "Placed camera").  The includer defines the ray CW_EX .. CW_DZ (origin and direction in
// the frame the grid lies in: t is the same in every frame), CW_GATE (the compile-time part of the walk's condition) and
// CW_BODY(rb) (what a hit reports for the triangle's body rb); `a.rg` (RayGridK), `a.far`, `live`, `near`, `best`, `body`,
// `s_cam_rec` and LDS are the kernel's (and `n_tests` in the counting build).  It is a block of its own: it declares nothing that
// outlives it, and it undefines the CW_ names.
{
  // slab clip against [o, hi]; a zero component gives +-inf (or NaN at a face, which fminf / fmaxf drop)
  const float ix_ = 1.0f / CW_DX, iy_ = 1.0f / CW_DY, iz_ = 1.0f / CW_DZ;
  const float x0 = (a.rg.ox - CW_EX) * ix_, x1 = (a.rg.hix - CW_EX) * ix_;
  const float y0 = (a.rg.oy - CW_EY) * iy_, y1 = (a.rg.hiy - CW_EY) * iy_;
  const float z0 = (a.rg.oz - CW_EZ) * iz_, z1 = (a.rg.hiz - CW_EZ) * iz_;
  const float t_in = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fmaxf(fminf(z0, z1), near));
  const float t_out = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fminf(fmaxf(z0, z1), fminf(a.far, best)));
  const bool inside_x = CW_DX != 0.0f || (CW_EX >= a.rg.ox && CW_EX <= a.rg.hix);    // a ray parallel to a slab and outside it misses
  const bool inside_y = CW_DY != 0.0f || (CW_EY >= a.rg.oy && CW_EY <= a.rg.hiy);
  const bool inside_z = CW_DZ != 0.0f || (CW_EZ >= a.rg.oz && CW_EZ <= a.rg.hiz);
  if (CW_GATE && live && t_in <= t_out && inside_x && inside_y && inside_z) {
    // the cell of the entry point, clamped; per axis the direction of travel, t at the next face and t per cell
    const float qx = CW_EX + t_in * CW_DX, qy = CW_EY + t_in * CW_DY, qz = CW_EZ + t_in * CW_DZ;
    int cx = min(max((int)floorf((qx - a.rg.ox) * a.rg.inv_cell), 0), a.rg.nx - 1);
    int cy = min(max((int)floorf((qy - a.rg.oy) * a.rg.inv_cell), 0), a.rg.ny - 1);
    int cz = min(max((int)floorf((qz - a.rg.oz) * a.rg.inv_cell), 0), a.rg.nz - 1);
    const int stx = CW_DX > 0.0f ? 1 : -1, sty = CW_DY > 0.0f ? 1 : -1, stz = CW_DZ > 0.0f ? 1 : -1;
    const float dtx = CW_DX != 0.0f ? a.rg.cell * fabsf(ix_) : INFINITY;
    const float dty = CW_DY != 0.0f ? a.rg.cell * fabsf(iy_) : INFINITY;
    const float dtz = CW_DZ != 0.0f ? a.rg.cell * fabsf(iz_) : INFINITY;
    float tmx = CW_DX != 0.0f ? (a.rg.ox + (float)(cx + (CW_DX > 0.0f ? 1 : 0)) * a.rg.cell - CW_EX) * ix_ : INFINITY;
    float tmy = CW_DY != 0.0f ? (a.rg.oy + (float)(cy + (CW_DY > 0.0f ? 1 : 0)) * a.rg.cell - CW_EY) * iy_ : INFINITY;
    float tmz = CW_DZ != 0.0f ? (a.rg.oz + (float)(cz + (CW_DZ > 0.0f ? 1 : 0)) * a.rg.cell - CW_EZ) * iz_ : INFINITY;
    const int max_cells = a.rg.nx + a.rg.ny + a.rg.nz;         // a walk visits fewer: every step moves one cell along one axis
    for (int it = 0; it < max_cells; ++it) {
      const int c = (cz * a.rg.ny + cy) * a.rg.nx + cx;
      const int end = a.rg.cell_start[c + 1];
      for (int k = a.rg.cell_start[c]; k < end; ++k) {
        const float4* r = (LDS ? s_cam_rec : a.rg.rec) + 4 * a.rg.cell_tri[k];
        const float4 r0 = r[0], r1 = r[1];
        const float acz = r[2].x;
        const int rb = __float_as_int(r[3].w);
        const float ax = r0.x, ay = r0.y, az = r0.z, abx = r0.w, aby = r1.x, abz = r1.y, acx = r1.z, acy = r1.w;
        const float pvx = CW_DY * acz - CW_DZ * acy, pvy = CW_DZ * acx - CW_DX * acz, pvz = CW_DX * acy - CW_DY * acx;      // d x ac
        const float det = abx * pvx + aby * pvy + abz * pvz;
        const float tx = CW_EX - ax, ty = CW_EY - ay, tz = CW_EZ - az;
        const float idet = DSIM_RCP(det);                      // (det = 0, a ray in the triangle's plane: inf, nothing passes)
        const float u = (tx * pvx + ty * pvy + tz * pvz) * idet;
        const float qvx = ty * abz - tz * aby, qvy = tz * abx - tx * abz, qvz = tx * aby - ty * abx;      // (e - a) x ab
        const float v = (CW_DX * qvx + CW_DY * qvy + CW_DZ * qvz) * idet;
        const float t = (acx * qvx + acy * qvy + acz * qvz) * idet;
        const bool hit = u >= 0.0f && v >= 0.0f && u + v <= 1.0f && t >= near && t <= a.far && t < best;
        best = hit ? t : best;
        body = hit ? CW_BODY(rb) : body;
#ifdef DSIM_CAM_COUNT
        ++n_tests;
#endif
      }
      const float t_exit = fminf(tmx, fminf(tmy, tmz));
      if (best <= t_exit || t_exit >= t_out) break;            // nothing nearer can lie in a later cell / the ray leaves the box
      const bool gx = tmx <= tmy && tmx <= tmz;
      const bool gy = !gx && tmy <= tmz;
      const bool gz = !gx && !gy;
      cx += gx ? stx : 0; cy += gy ? sty : 0; cz += gz ? stz : 0;
      tmx += gx ? dtx : 0.0f; tmy += gy ? dty : 0.0f; tmz += gz ? dtz : 0.0f;
      if (cx < 0 || cx >= a.rg.nx || cy < 0 || cy >= a.rg.ny || cz < 0 || cz >= a.rg.nz) break;
    }
  }
}
#undef CW_EX
#undef CW_EY
#undef CW_EZ
#undef CW_DX
#undef CW_DY
#undef CW_DZ
#undef CW_GATE
#undef CW_BODY
