// Host-only check of t2l_text_inter's launch plan (text2loc_amd/csrc/text_inter_plan.h): for every compiled width, n_desc around the
// workgroup boundaries and S across the tilings, walk the grid the way text_inter_fused2_kernel does (workgroup g, tile t: descriptions
// [g * 2 dpt + t * dpt, ... + dpt) clipped to n_desc) and assert that every description is covered exactly once, no tile exceeds 32 rows,
// whole descriptions only, and the LDS fits the 160 KiB of a gfx950 workgroup. Built and run by tests/test_text_inter_shapes_cpu.py.
#include <stdio.h>

#include <vector>

#include "text_inter_plan.h"

static int failures = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      ++failures;                   \
      printf("FAIL %s: ", #cond);   \
      printf(__VA_ARGS__);          \
      printf("\n");                 \
    }                               \
  } while (0)

int main() {
  using namespace t2l;
  // the compiled set, and its neighbours
  const int yes[][2] = {{256, 4}, {128, 4}, {128, 2}, {256, 8}};
  const int no[][2] = {{128, 8}, {256, 2}, {64, 2}, {64, 1}, {192, 6}, {192, 3}, {256, 0}, {128, 3}, {512, 8}, {0, 4}, {256, 16}, {128, 1}};
  for (auto& s : yes) CHECK(text_inter_shape_is_compiled(s[0], s[1]), "(%d, %d)", s[0], s[1]);
  for (auto& s : no) CHECK(!text_inter_shape_is_compiled(s[0], s[1]), "(%d, %d)", s[0], s[1]);

  const int widths[] = {128, 256};
  const int sents[] = {1, 5, 6, 11, 16, 17, 32};
  for (int D : widths)
    for (int S : sents) {
      const int dpt = 32 / S;
      const int counts[] = {0, 1, 2 * dpt - 1, 2 * dpt, 2 * dpt + 1};
      for (int n_desc : counts) {
        const TextInterPlan p = text_inter_plan(D, n_desc, S);
        CHECK(p.dpt == dpt && p.dpt >= 1, "D %d S %d: dpt %d", D, S, p.dpt);
        CHECK(p.rows_per_tile == dpt * S && p.rows_per_tile <= kInterTileRows, "D %d S %d: %d rows per tile", D, S, p.rows_per_tile);
        CHECK(kInterTilesPerWg == 2 && p.desc_per_wg == 2 * dpt, "D %d S %d: %d descriptions per workgroup", D, S, p.desc_per_wg);
        CHECK(p.threads == 2 * D && p.threads % 64 == 0 && p.threads <= 1024, "D %d: %d threads", D, p.threads);
        CHECK(p.lds_bytes <= 160 * 1024, "D %d: %zu bytes of LDS", D, p.lds_bytes);
        // the planes alone: 8 planes of 32 rows of D + 8 halves
        CHECK(p.lds_bytes >= (size_t)8 * 32 * (D + 8) * 2 + 32 * 4, "D %d: %zu bytes of LDS", D, p.lds_bytes);
        CHECK(p.grid == (n_desc + 2 * dpt - 1) / (2 * dpt), "D %d S %d n %d: grid %d", D, S, n_desc, p.grid);
        CHECK((n_desc == 0) == (p.grid == 0), "D %d S %d n %d: grid %d", D, S, n_desc, p.grid);
        std::vector<int> seen(n_desc, 0);
        for (int g = 0; g < p.grid; ++g) {
          int in_wg = 0;
          for (int t = 0; t < kInterTilesPerWg; ++t) {
            const int d0 = g * p.desc_per_wg + t * p.dpt;
            int nd = n_desc - d0;  // the kernel's clip: min(dpt, n_desc - d0), not below 0
            if (nd > p.dpt) nd = p.dpt;
            if (nd < 0) nd = 0;
            CHECK(nd * S <= kInterTileRows, "D %d S %d n %d: tile (%d, %d) holds %d rows", D, S, n_desc, g, t, nd * S);
            for (int d = 0; d < nd; ++d) {
              CHECK(d0 + d < n_desc, "D %d S %d n %d: description %d out of range", D, S, n_desc, d0 + d);
              if (d0 + d < n_desc) ++seen[d0 + d];
            }
            in_wg += nd;
          }
          CHECK(in_wg >= 1, "D %d S %d n %d: workgroup %d is empty", D, S, n_desc, g);
        }
        for (int d = 0; d < n_desc; ++d) CHECK(seen[d] == 1, "D %d S %d n %d: description %d covered %d times", D, S, n_desc, d, seen[d]);
      }
    }
  // the published shape's figures, as the 256-only launcher computed them
  {
    const TextInterPlan p = text_inter_plan(256, 4096, 6);
    CHECK(p.dpt == 5 && p.grid == 410 && p.threads == 512 && p.lds_bytes == (size_t)8 * 32 * 264 * 2 + 32 * 4 + 1024 * 4,
          "published: dpt %d grid %d threads %d lds %zu", p.dpt, p.grid, p.threads, p.lds_bytes);
    const TextInterPlan q = text_inter_plan(128, 4096, 6);
    CHECK(q.grid == 410 && q.threads == 256 && q.lds_bytes == (size_t)8 * 32 * 136 * 2 + 32 * 4 + 512 * 4 && 2 * q.lds_bytes <= 160 * 1024,
          "d128: grid %d threads %d lds %zu (two workgroups per CU)", q.grid, q.threads, q.lds_bytes);
  }
  if (failures) {
    printf("text_inter_plan_check: %d failure(s)\n", failures);
    return 1;
  }
  printf("text_inter_plan_check: ok\n");
  return 0;
}
