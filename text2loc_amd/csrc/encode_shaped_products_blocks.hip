// Dev-only block library (libt2l_blocks.so; never shipped, not part of include/t2l.h): ONE product of the one-cell cell encoder at a
// time through mm_tiles, so that tests/test_gpu_encode_blocks.py can hold every element against a float64 reference
// (tests/encode_blocks.py). mm_tiles lives in encode_shaped.hip's anonymous namespace, so this unit includes that file — as a THIRD
// copy beside encode_shaped.o (shipped) and encode_shaped_blocks.o (which stands in for it in the dev library): with this door
// in encode_shaped_blocks.hip, three instances of that unit's encode_cells_shaped_kernel compiled to another listing than the shipped
// one (tools/device_code_diff.py), so the door moved out and that unit is identical again. The copy's external names are renamed
// below; its kernels and host functions are never called.
//
// Return: 0, -1 (refused, message through t2l_blk_last_error; nothing was launched), -2 (the HIP runtime reported an error). The
// launch is synchronised before the wrapper returns.
#define shape_is_compiled blk_prodcopy_shape_is_compiled
#define compiled_shapes_text blk_prodcopy_compiled_shapes_text
#define encode_shaped_impl blk_prodcopy_encode_shaped_impl
#include "encode_shaped.hip"
#undef shape_is_compiled
#undef compiled_shapes_text
#undef encode_shaped_impl
#include "blocks_common.h"

namespace t2l {
namespace {

// ONE product of the one-cell kernel through mm_tiles<H, WA, D / 128, D == 256> (the instance its row products use; H = 0: the f32
// MFMA on the pack_half_split packing, 1: split-f16, 2: plain f16 on the pack_h fragments): out = X W_sel^T without bias, for n_tiles
// 32-row weight tiles from tile0 on, of a matrix packed for K = ktot, over the kin k-values [koff, koff + kin / 2) of each k half.
// The input tile lives in LDS with the kernel's own stride kin + 4; wave w owns tiles w, w + 4, .. of every group of 4 NT, as `own`.
// WA: the packed weights are the A operand and the tile comes out transposed (q^T / k^T), stored back straight.
struct BlkProd {
  const float4* wp;
  const uint4* hp;
  int ktot, kin, koff, tile0, n_tiles;
};
template <int D, int H, bool WA>
__global__ __launch_bounds__(256) void blk_encs_product_kernel(BlkProd P, const float* __restrict__ x, float* __restrict__ out) {
  constexpr int NT = D / 128;
  __shared__ __attribute__((aligned(16))) float tile[kSP * (256 + 4)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  const int ld = P.kin + 4, N = P.n_tiles * 32;
  const float* g = x + (size_t)blockIdx.x * kSP * P.kin;
  float* o = out + (size_t)blockIdx.x * kSP * N;
  for (int i = tid; i < kSP * ld; i += 256) {
    const int r = i / ld, c = i % ld;
    tile[i] = c < P.kin ? g[r * P.kin + c] : __builtin_nanf("");  // (the padding is never read)
  }
  __syncthreads();
  for (int g0 = 0; g0 < P.n_tiles; g0 += 4 * NT) {
    int own[NT];
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) own[t] = P.tile0 + g0 + wave + 4 * t;
    zero_tiles(acc);
    mm_tiles<H, WA, NT, D == 256>(tile + col * ld + half * (P.kin / 2), P.kin / 2, P.wp, P.hp, P.ktot, P.koff, own, acc, lane);
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n0 = (own[t] - P.tile0) * 32;
        if constexpr (WA) o[col * N + n0 + acc_row(r, half)] = acc[t][r];
        else o[acc_row(r, half) * N + n0 + col] = acc[t][r];
      }
  }
}

template <int D, int H>
void blk_product_launch(bool wa, int n_wg, const BlkProd& P, const float* x, float* out) {
  if (wa) hipLaunchKernelGGL((blk_encs_product_kernel<D, H, true>), dim3(n_wg), dim3(256), 0, nullptr, P, x, out);
  else hipLaunchKernelGGL((blk_encs_product_kernel<D, H, false>), dim3(n_wg), dim3(256), 0, nullptr, P, x, out);
}

}  // namespace
}  // namespace t2l

using namespace t2l;

extern "C" {

// One product of the loaded model (t2l_load_weights_shaped) through mm_tiles, on the packing the loader made. arm 0 f32 MFMA, 1
// split-f16, 2 plain f16 (compiled at D = 256 only, as in the product). which: 0 q^T, 1 k^T (transposed products), 2 v, 3 out_proj,
// 4 linear1 (all of layer `layer`; x [n_wg][32][D]), 5 linear2's pass sub = 0 / 1 (x = that pass's hidden tile [32][D] in the order of
// the kernel's buf), 6 slot sub of mlp_merge (the product runs it split-f16 under arm 2 too, and so does this), 7 the second
// layer of pos (sub 0) / color (1) / num (2) encoder (x [n_wg][32][64], arm 0 only). out: float [n_wg][32][N], N = D (2 D: linear1).
int t2l_blk_encs_product(t2l_ctx* ctx, int arm, int which, int layer, int sub, int n_wg, const float* x, float* out) {
  const std::string who = "t2l_blk_encs_product";
  const EncoderWeights* ew = ctx ? ctx->enc : nullptr;
  if (!ew) return blk_refuse(who + ": no context, or encoder weights not loaded");
  if (arm < 0 || arm > 2 || which < 0 || which > 7 || n_wg < 1 || n_wg > 4096 || !x || !out)
    return blk_refuse(who + ": need arm 0..2, which 0..7, 1 <= n_wg <= 4096, x and out");
  const EncParams& E = ew->p;
  const int D = ew->embed_dim, DT = D / 32;
  if (D != 128 && D != 256) return blk_refuse(who + ": width not compiled");
  if (arm == 2 && D != 256) return blk_refuse(who + ": plain f16 is compiled at width 256 only");
  if (arm != 0 && !E.split_ok) return blk_refuse(who + ": the loaded weights do not bound the f16 range (the product runs them all-f32)");
  BlkProd P{nullptr, nullptr, D, D, 0, 0, DT};
  int H = arm;
  if (which <= 5) {
    if (layer < 0 || layer >= E.num_layers) return blk_refuse(who + ": no such layer of the loaded model");
    const LayerW& L = E.layer[layer];
    if (which <= 2) { P.wp = L.in_wp; P.hp = L.in_hp; P.tile0 = which * DT; }
    else if (which == 3) { P.wp = L.out_wp; P.hp = L.out_hp; }
    else if (which == 4) { P.wp = L.ff1_wp; P.hp = L.ff1_hp; P.n_tiles = 2 * DT; }
    else {
      if (sub != 0 && sub != 1) return blk_refuse(who + ": linear2 has passes 0 and 1");
      P.wp = L.ff2_wp; P.hp = L.ff2_hp; P.ktot = 2 * D; P.koff = sub * (D / 2);
    }
  } else if (which == 6) {
    if (E.nfeat < 2 || sub < 0 || sub >= E.nfeat) return blk_refuse(who + ": no such slot of mlp_merge (a single-feature model has none)");
    P.wp = E.merge_wp + (size_t)sub * (D * D / 4);
    P.hp = E.merge_hp + (size_t)sub * (D * D / 4);
    H = arm ? 1 : 0;
  } else {
    if (arm != 0) return blk_refuse(who + ": the small encoders run on the f32 MFMA (arm 0)");
    const SmallMlp* m = sub == 0 && E.use_pos ? &E.pos : sub == 1 && E.use_color && !E.color_embed ? &E.color : sub == 2 && E.use_num ? &E.num : nullptr;
    if (!m) return blk_refuse(who + ": the loaded model has no such small encoder (sub 0 pos, 1 color MLP, 2 num)");
    P.wp = m->w2p; P.ktot = 64; P.kin = 64;
  }
  if (!P.wp || (H != 0 && !P.hp)) return blk_refuse(who + ": the loaded model has a null array there");
  if (hipSetDevice(ctx->device) != hipSuccess) {
    blk_refuse(who + ": hipSetDevice failed");
    return -2;
  }
  const bool wa = which <= 1;
  if (D == 128) {
    if (H == 0) blk_product_launch<128, 0>(wa, n_wg, P, x, out);
    else blk_product_launch<128, 1>(wa, n_wg, P, x, out);
  } else {
    if (H == 0) blk_product_launch<256, 0>(wa, n_wg, P, x, out);
    else if (H == 1) blk_product_launch<256, 1>(wa, n_wg, P, x, out);
    else blk_product_launch<256, 2>(wa, n_wg, P, x, out);
  }
  return blk_finish("t2l_blk_encs_product");
}

}  // extern "C"
