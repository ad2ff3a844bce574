// Host-only self-test of the static-obstacle watch's grid builder (dronesim_amd/csrc/dsim_obstacle_grid.h): plain C++, meant to be
// compiled with -fsanitize=address,undefined.
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/obstacle_grid_selftest.cpp -o selftest && ./selftest
// Plans and builds the grid of a seeded random soup, of one triangle and of a kilometre-long soup, checks the shape of the
// lists (monotone starts, every entry a triangle, every triangle in the cell of its own centroid), makes the records, and feeds
// the builder everything it must refuse.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../dronesim_amd/csrc/dsim_obstacle_grid.h"

static unsigned long long rng_state = 88172645463325252ULL;
static double uni() {                                  // xorshift64: deterministic, no library state
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (double)(rng_state >> 11) / 9007199254740992.0;
}

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #x); exit(1); } } while (0)

static void one(const std::vector<float>& tri, float reach) {
  const int64_t n = (int64_t)tri.size() / 9;
  dsim_obstacle_grid g;
  CHECK(dsim_obs::plan(tri.data(), n, reach, &g) == DSIM_OK);
  const int64_t cells = (int64_t)g.nx * g.ny * g.nz;
  CHECK(cells >= 1 && cells <= DSIM_OBS_MAX_CELLS && g.list_len >= n);
  std::vector<int32_t> start(cells + 1), list(g.list_len);
  CHECK(dsim_obs::build(tri.data(), n, &g, start.data(), list.data()) == DSIM_OK);
  CHECK(start[0] == 0 && start[cells] == g.list_len);
  for (int64_t c = 0; c < cells; ++c) CHECK(start[c] <= start[c + 1]);
  for (int64_t k = 0; k < g.list_len; ++k) CHECK(list[k] >= 0 && list[k] < n);
  for (int64_t t = 0; t < n; ++t) {
    int c3[3];
    const int nn[3] = {g.nx, g.ny, g.nz};
    for (int k = 0; k < 3; ++k) {
      const double m = ((double)tri[9 * t + k] + tri[9 * t + 3 + k] + tri[9 * t + 6 + k]) / 3.0;
      c3[k] = (int)floor((m - g.origin[k]) / g.cell);
      CHECK(c3[k] >= 0 && c3[k] < nn[k]);
    }
    const int64_t c = ((int64_t)c3[2] * g.ny + c3[1]) * g.nx + c3[0];
    bool found = false;
    for (int32_t k = start[c]; k < start[c + 1]; ++k) found |= list[k] == t;
    CHECK(found);
  }
  std::vector<float> rec(DSIM_OBS_REC_FLOATS * n);
  std::vector<int32_t> body(n);
  for (int64_t t = 0; t < n; ++t) body[t] = (int32_t)(t % 4);
  dsim_obs::records(tri.data(), body.data(), n, rec.data());
  dsim_obs::records(tri.data(), nullptr, n, rec.data());
  dsim_obstacle_grid wrong = g;
  wrong.nz += 1;
  CHECK(dsim_obs::build(tri.data(), n, &wrong, start.data(), list.data()) == DSIM_E_ARG);
  printf("  %lld triangles, reach %.3f: %d x %d x %d cells of %.3f m, %lld list entries\n", (long long)n, reach, g.nx, g.ny, g.nz,
         g.cell, (long long)g.list_len);
}

int main() {
  std::vector<float> soup;
  for (int t = 0; t < 3000; ++t) {
    const double c[3] = {20.0 * uni() - 10.0, 20.0 * uni() - 10.0, 20.0 * uni() - 10.0};
    for (int k = 0; k < 9; ++k) soup.push_back((float)(c[k % 3] + 1.5 * uni() - 0.75));
  }
  one(soup, 0.9f);
  one(soup, 0.05f);
  one(std::vector<float>{0, 0, 1, 2, 0, 1, 0.5f, 1.5f, 1.3f}, 0.75f);
  std::vector<float> far = {0, 0, 0, 1, 0, 0, 0, 1, 0, 1000, 1000, 1000, 1001, 1000, 1000, 1000, 1001, 1000};
  one(far, 0.05f);
  dsim_obstacle_grid g;
  std::vector<float> flat = {0, 0, 0, 1, 0, 0, 2, 0, 0};
  CHECK(dsim_obs::plan(flat.data(), 1, 1.0f, &g) == DSIM_E_ARG);
  CHECK(dsim_obs::plan(soup.data(), 3000, 0.0f, &g) == DSIM_E_ARG);
  CHECK(dsim_obs::plan(soup.data(), 3000, -1.0f, &g) == DSIM_E_ARG);
  CHECK(dsim_obs::plan(soup.data(), 0, 1.0f, &g) == DSIM_E_ARG);
  CHECK(dsim_obs::plan(nullptr, 1, 1.0f, &g) == DSIM_E_ARG);
  CHECK(dsim_obs::plan(soup.data(), 3000, 1.0f, nullptr) == DSIM_E_ARG);
  std::vector<float> nan = soup;
  nan[77] = NAN;
  CHECK(dsim_obs::plan(nan.data(), 3000, 1.0f, &g) == DSIM_E_ARG);
  std::vector<float> huge = {0, 0, 0, 1, 0, 0, 0, 1, 0, 3e38f, 3e38f, 3e38f, -3e38f, 3e38f, 3e38f, 3e38f, -3e38f, 3e38f};
  (void)dsim_obs::plan(huge.data(), 2, 1.0f, &g);               // (either answer; it must not overflow an index on the way)
  printf("obstacle grid self-test: ok\n");
  return 0;
}
