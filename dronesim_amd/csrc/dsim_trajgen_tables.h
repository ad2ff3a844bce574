// dsim_trajgen_tables.h — written by tools/gen_trajgen_tables.py; do not edit.
// End values of a degree-9 segment in its own time s = t / T: e^ = (p, T p', T^2 p'', T^3 p''', T^4 p'''') at s = 0, then at s = 1.
// DSIM_TG_AINV: c^ = AINV e^, c^_j = c_j T^j (the inverse of the constant Hermite matrix; its entries are integers and 1 / k!).
// DSIM_TG_M = AINV^T Q^ AINV, Q^ the reference's Hessian at T = 1 (trajutils.py:24-36): a segment's snap cost is e^^T M e^ / T^7.
// DSIM_TG_F: 6 x 10 with F^T F = M (sqrt(D) L^T of Q^'s 6 x 6 block = L D L^T, times AINV's last six rows): the cost is |F e^|^2 / T^7.
// Exact rationals (F: to 256 bits) rounded once to fp64, written as hexadecimal floating literals.
#pragma once
__constant__ const double DSIM_TG_AINV[10][10] = {
  {0x1.0000000000000p+0, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0},
  {0x0.0p+0, 0x1.0000000000000p+0, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0},
  {0x0.0p+0, 0x0.0p+0, 0x1.0000000000000p-1, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0},
  {0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x1.5555555555555p-3, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0},
  {0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x1.5555555555555p-5, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0},
  {-0x1.f800000000000p+6, -0x1.1800000000000p+6, -0x1.1800000000000p+4, -0x1.4000000000000p+1, -0x1.aaaaaaaaaaaabp-3, 0x1.f800000000000p+6, -0x1.c000000000000p+5, 0x1.5000000000000p+3, -0x1.0000000000000p+0, 0x1.5555555555555p-5},
  {0x1.a400000000000p+8, 0x1.c000000000000p+7, 0x1.a400000000000p+5, 0x1.aaaaaaaaaaaabp+2, 0x1.aaaaaaaaaaaabp-2, -0x1.a400000000000p+8, 0x1.8800000000000p+7, -0x1.3400000000000p+5, 0x1.eaaaaaaaaaaabp+1, -0x1.5555555555555p-3},
  {-0x1.0e00000000000p+9, -0x1.1800000000000p+8, -0x1.f800000000000p+5, -0x1.e000000000000p+2, -0x1.aaaaaaaaaaaabp-2, 0x1.0e00000000000p+9, -0x1.0400000000000p+8, 0x1.a800000000000p+5, -0x1.6000000000000p+2, 0x1.0000000000000p-2},
  {0x1.3b00000000000p+8, 0x1.4000000000000p+7, 0x1.1800000000000p+5, 0x1.0000000000000p+2, 0x1.aaaaaaaaaaaabp-3, -0x1.3b00000000000p+8, 0x1.3600000000000p+7, -0x1.0400000000000p+5, 0x1.c000000000000p+1, -0x1.5555555555555p-3},
  {-0x1.1800000000000p+6, -0x1.1800000000000p+5, -0x1.e000000000000p+2, -0x1.aaaaaaaaaaaabp-1, -0x1.5555555555555p-5, 0x1.1800000000000p+6, -0x1.1800000000000p+5, 0x1.e000000000000p+2, -0x1.aaaaaaaaaaaabp-1, 0x1.5555555555555p-5}};
__constant__ const double DSIM_TG_M[10][10] = {
  {0x1.4228ba2e8ba2fp+18, 0x1.4228ba2e8ba2fp+17, 0x1.08e2e8ba2e8bap+15, 0x1.90e8ba2e8ba2fp+11, 0x1.31745d1745d17p+6, -0x1.4228ba2e8ba2fp+18, 0x1.4228ba2e8ba2fp+17, -0x1.08e2e8ba2e8bap+15, 0x1.90e8ba2e8ba2fp+11, -0x1.31745d1745d17p+6},
  {0x1.4228ba2e8ba2fp+17, 0x1.4ae8ba2e8ba2fp+16, 0x1.1a62e8ba2e8bap+14, 0x1.c2e8ba2e8ba2fp+10, 0x1.66c9b26c9b26dp+5, -0x1.4228ba2e8ba2fp+17, 0x1.3968ba2e8ba2fp+16, -0x1.eec5d1745d174p+13, 0x1.5ee8ba2e8ba2fp+10, -0x1.f83e0f83e0f84p+4},
  {0x1.08e2e8ba2e8bap+15, 0x1.1a62e8ba2e8bap+14, 0x1.fd1745d1745d1p+11, 0x1.bba2e8ba2e8bap+8, 0x1.707c1f07c1f08p+3, -0x1.08e2e8ba2e8bap+15, 0x1.eec5d1745d174p+13, -0x1.711745d1745d1p+11, 0x1.e745d1745d174p+7, -0x1.364d9364d9365p+2},
  {0x1.90e8ba2e8ba2fp+11, 0x1.c2e8ba2e8ba2fp+10, 0x1.bba2e8ba2e8bap+8, 0x1.d1745d1745d17p+5, 0x1.9364d9364d936p+0, -0x1.90e8ba2e8ba2fp+11, 0x1.5ee8ba2e8ba2fp+10, -0x1.e745d1745d174p+7, 0x1.22e8ba2e8ba2fp+4, -0x1.f07c1f07c1f08p-3},
  {0x1.31745d1745d17p+6, 0x1.66c9b26c9b26dp+5, 0x1.707c1f07c1f08p+3, 0x1.9364d9364d936p+0, 0x1.9dbcc48676f31p-4, -0x1.31745d1745d17p+6, 0x1.f83e0f83e0f84p+4, -0x1.364d9364d9365p+2, 0x1.f07c1f07c1f08p-3, 0x1.4afd6a052bf5bp-7},
  {-0x1.4228ba2e8ba2fp+18, -0x1.4228ba2e8ba2fp+17, -0x1.08e2e8ba2e8bap+15, -0x1.90e8ba2e8ba2fp+11, -0x1.31745d1745d17p+6, 0x1.4228ba2e8ba2fp+18, -0x1.4228ba2e8ba2fp+17, 0x1.08e2e8ba2e8bap+15, -0x1.90e8ba2e8ba2fp+11, 0x1.31745d1745d17p+6},
  {0x1.4228ba2e8ba2fp+17, 0x1.3968ba2e8ba2fp+16, 0x1.eec5d1745d174p+13, 0x1.5ee8ba2e8ba2fp+10, 0x1.f83e0f83e0f84p+4, -0x1.4228ba2e8ba2fp+17, 0x1.4ae8ba2e8ba2fp+16, -0x1.1a62e8ba2e8bap+14, 0x1.c2e8ba2e8ba2fp+10, -0x1.66c9b26c9b26dp+5},
  {-0x1.08e2e8ba2e8bap+15, -0x1.eec5d1745d174p+13, -0x1.711745d1745d1p+11, -0x1.e745d1745d174p+7, -0x1.364d9364d9365p+2, 0x1.08e2e8ba2e8bap+15, -0x1.1a62e8ba2e8bap+14, 0x1.fd1745d1745d1p+11, -0x1.bba2e8ba2e8bap+8, 0x1.707c1f07c1f08p+3},
  {0x1.90e8ba2e8ba2fp+11, 0x1.5ee8ba2e8ba2fp+10, 0x1.e745d1745d174p+7, 0x1.22e8ba2e8ba2fp+4, 0x1.f07c1f07c1f08p-3, -0x1.90e8ba2e8ba2fp+11, 0x1.c2e8ba2e8ba2fp+10, -0x1.bba2e8ba2e8bap+8, 0x1.d1745d1745d17p+5, -0x1.9364d9364d936p+0},
  {-0x1.31745d1745d17p+6, -0x1.f83e0f83e0f84p+4, -0x1.364d9364d9365p+2, -0x1.f07c1f07c1f08p-3, 0x1.4afd6a052bf5bp-7, 0x1.31745d1745d17p+6, -0x1.66c9b26c9b26dp+5, 0x1.707c1f07c1f08p+3, -0x1.9364d9364d936p+0, 0x1.9dbcc48676f31p-4}};
__constant__ const double DSIM_TG_F[6][10] = {
  {0x0.0p+0, 0x0.0p+0, 0x0.0p+0, -0x1.6a09e667f3bcdp+0, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x1.6a09e667f3bcdp+0, 0x0.0p+0},
  {0x0.0p+0, 0x0.0p+0, 0x1.3988e1409212ep+2, 0x1.3988e1409212ep+1, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0, -0x1.3988e1409212ep+2, 0x1.3988e1409212ep+1, 0x0.0p+0},
  {0x0.0p+0, -0x1.2f9422c23c47ep+5, -0x1.2f9422c23c47ep+4, -0x1.94c583ada5b53p+1, 0x0.0p+0, 0x0.0p+0, 0x1.2f9422c23c47ep+5, -0x1.2f9422c23c47ep+4, 0x1.94c583ada5b53p+1, 0x0.0p+0},
  {0x1.c0ffb7051bb55p+8, 0x1.c0ffb7051bb55p+7, 0x1.6732f8d0e2f77p+5, 0x1.deeea11683f49p+1, 0x0.0p+0, -0x1.c0ffb7051bb55p+8, 0x1.c0ffb7051bb55p+7, -0x1.6732f8d0e2f77p+5, 0x1.deeea11683f49p+1, 0x0.0p+0},
  {0x0.0p+0, 0x1.c48c6001f0ac0p+4, 0x1.c48c6001f0ac0p+3, 0x1.6a09e667f3bcdp+1, 0x1.e2b7dddfefa66p-3, 0x0.0p+0, -0x1.c48c6001f0ac0p+4, 0x1.c48c6001f0ac0p+3, -0x1.6a09e667f3bcdp+1, 0x1.e2b7dddfefa66p-3},
  {-0x1.662d5d350447bp+8, -0x1.662d5d350447bp+7, -0x1.33024fe44ccfcp+5, -0x1.10e59c5927d52p+2, -0x1.b4a293c1d9550p-3, 0x1.662d5d350447bp+8, -0x1.662d5d350447bp+7, 0x1.33024fe44ccfcp+5, -0x1.10e59c5927d52p+2, 0x1.b4a293c1d9550p-3}};
