// The launch plan of t2l_text_inter (encode.hip: text_inter_fused2_kernel) as plain host code, so that a host-only program can
// walk it (tests/text_inter_plan_check.cpp): which (width, heads) pairs are compiled, and for n_desc descriptions of S sentences at
// width D the tiling, the grid and the LDS of the one launch. No HIP in here.
#pragma once
#include <stddef.h>

namespace t2l {

constexpr int kInterTileRows = 32;   // one MFMA tile of token rows
constexpr int kInterTilesPerWg = 2;  // a workgroup of D / 32 waves works on two tiles

// the compiled set: inter_mlp width D in {128, 256} with head_dim D / heads in {32, 64}; dim_feedforward = 4 D; one layer
inline bool text_inter_shape_is_compiled(int D, int heads) {
  if (D != 128 && D != 256) return false;
  if (heads <= 0 || D % heads) return false;
  return D / heads == 32 || D / heads == 64;
}
inline const char* text_inter_shapes_text() {
  return "compiled shapes of the inter layer: one layer, width 128 with 2 or 4 heads or 256 with 4 or 8 heads, dim_feedforward 4 x width";
}

struct TextInterPlan {
  int dpt = 0;            // whole descriptions per tile: floor(32 / S)
  int rows_per_tile = 0;  // live rows of a full tile: dpt * S <= 32 (the rest are zero rows, groups of their own)
  int desc_per_wg = 0;    // kInterTilesPerWg * dpt: workgroup g serves descriptions [g * desc_per_wg, ...), tile t the t-th dpt of them
  int grid = 0;           // workgroups: ceil(n_desc / desc_per_wg)
  int threads = 0;        // 64 * D / 32
  size_t lds_bytes = 0;   // 8 split-f16 planes of 32 x (D + 8) halves + the rows' group ids + the LayerNorm row sums
};

// 1 <= S <= 32, n_desc >= 0, D a compiled width
inline TextInterPlan text_inter_plan(int D, int n_desc, int S) {
  TextInterPlan p;
  p.dpt = kInterTileRows / S;
  p.rows_per_tile = p.dpt * S;
  p.desc_per_wg = kInterTilesPerWg * p.dpt;
  p.grid = (n_desc + p.desc_per_wg - 1) / p.desc_per_wg;
  p.threads = 64 * (D / 32);
  p.lds_bytes = (size_t)4 * kInterTilesPerWg * kInterTileRows * (D + 8) * 2 /* halves */ + kInterTileRows * sizeof(int) +
                (size_t)2 * kInterTilesPerWg * (D / 32) * 32 * sizeof(float);
  return p;
}

}  // namespace t2l
