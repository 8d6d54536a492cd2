// Dev-only block library (libt2l_blocks.so; never shipped, not part of include/t2l.h): the row stages of the one-cell cell encoder ONE
// call at a time, so that tests/test_gpu_encode_blocks.py can hold every element against a float64 reference (tests/encode_blocks.py).
// This translation unit IS encode_shaped.hip plus the wrapper below and is linked in encode_shaped.o's place. The stage kernel copies
// a workgroup's f32 tile [32][D] from global memory into LDS rows of D + 4 floats (the kernel's own stride), calls normalize_rows_d<D>
// or layer_norm_rows_d<D> ONCE with the kernel's four waves and copies the tile out.
//
// (The door to mm_tiles is a unit of its own, encode_shaped_products_blocks.hip: with it in this unit three instances of this unit's
// copy of encode_cells_shaped_kernel compiled to another listing than the shipped one.)
//
// Not here: encode_cells_shaped_kernel itself takes no tap (moving its body into a device function changed the shipped listing):
// its attention core, epilogues, merge loop, pool and wiring stay with the end-to-end tests (profiles/encode_blocks.md).
//
// Return: 0, -1 (refused, message through t2l_blk_last_error; nothing was launched), -2 (the HIP runtime reported an error). The
// launch is synchronised before the wrapper returns.
#include "encode_shaped.hip"
#include "blocks_common.h"

namespace t2l {
namespace {

template <int D, int OP>  // OP 0: normalize_rows_d, 1: layer_norm_rows_d
__global__ __launch_bounds__(256) void blk_encs_rows_kernel(float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b, int nvalid) {
  constexpr int LD = D + 4;
  __shared__ __attribute__((aligned(16))) float tile[kSP * LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* g = x + (size_t)blockIdx.x * kSP * D;
  for (int i = tid; i < kSP * LD; i += 256) {
    const int r = i / LD, c = i % LD;
    tile[i] = c < D ? g[r * D + c] : __builtin_nanf("");  // (the padding is never read)
  }
  __syncthreads();
  if constexpr (OP == 0) normalize_rows_d<D>(tile, LD, nvalid, wave, lane);
  else layer_norm_rows_d<D>(tile, w, b, wave, lane);
  __syncthreads();
  for (int i = tid; i < kSP * D; i += 256) g[i] = tile[(i / D) * LD + (i % D)];
}

}  // namespace
}  // namespace t2l

using namespace t2l;

extern "C" {

// op 0: F.normalize over the D columns of rows < nvalid, rows >= nvalid zeroed (w, b unused); op 1: LayerNorm(D, eps 1e-5) with gain w
// and bias b (device pointers, D floats each; nvalid unused). x: float [n_wg][32][D], in place.
int t2l_blk_encs_rows(int op, int D, int n_wg, float* x, const float* w, const float* b, int nvalid) {
  const std::string who = "t2l_blk_encs_rows";
  if ((op != 0 && op != 1) || (D != 128 && D != 256) || n_wg < 1 || n_wg > 4096) return blk_refuse(who + ": need op 0 / 1, D 128 / 256, 1 <= n_wg <= 4096");
  if (!x) return blk_refuse(who + ": null tile");
  if (op == 0 && (nvalid < 0 || nvalid > kSP)) return blk_refuse(who + ": need 0 <= nvalid <= 32");
  if (op == 1 && (!w || !b)) return blk_refuse(who + ": the LayerNorm needs gain and bias");
  if (D == 128) {
    if (op == 0) hipLaunchKernelGGL((blk_encs_rows_kernel<128, 0>), dim3(n_wg), dim3(256), 0, nullptr, x, w, b, nvalid);
    else hipLaunchKernelGGL((blk_encs_rows_kernel<128, 1>), dim3(n_wg), dim3(256), 0, nullptr, x, w, b, nvalid);
  } else {
    if (op == 0) hipLaunchKernelGGL((blk_encs_rows_kernel<256, 0>), dim3(n_wg), dim3(256), 0, nullptr, x, w, b, nvalid);
    else hipLaunchKernelGGL((blk_encs_rows_kernel<256, 1>), dim3(n_wg), dim3(256), 0, nullptr, x, w, b, nvalid);
  }
  return blk_finish("t2l_blk_encs_rows");
}

}  // extern "C"
