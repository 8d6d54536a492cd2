// Dev-only block library (libt2l_blocks.so; never shipped, not part of include/t2l.h): the fine match's attention block and decoder
// pass one call at a time, so that tests/test_gpu_fine_blocks.py can hold every element of a tile against a float64 reference
// (tests/fine_blocks.py). This translation unit IS fine.hip plus the wrappers below and is linked in fine.o's place: the weights are
// the ones the context's own t2l_fine_load_weights packed (FineParams), the device functions are the product's. A stage kernel here
// copies its tiles from global memory into LDS, calls ONE device function of fine.hip and copies the result out; nothing else.
//
// Tiles travel in the arm's own storage, [n_wg][32][128] each (workgroup b works on tile b of every array):
//   arm 0 (f32 MFMA on f32 tiles): `a` = float rows, `b` unused (null)
//   arm 1 (split-f16) / 2 (plain f16): `a` = the hi plane, `b` = the lo plane, _Float16 each — hi + lo re-split is not the identity
//   (fine.hip, above fp_attention), so a chain of calls that is to reproduce the product's state bit for bit passes planes as planes.
// Groups are int32[4] = TileGroups {shift, count, rows, base}: {4, c, 32, 0} and {4, c, 32, 2} (object tiles A / B, 1 <= c <= 16;
// the product builds c = 16) and {3, n_hints, 32, 0} (the hint tile, 1 <= n_hints <= 8). Anything else is refused.
//
// Return: 0, -1 (refused, message through t2l_blk_last_error; nothing was launched), -2 (the HIP runtime reported an error). The
// launch is synchronised before a wrapper returns.
#include "fine.hip"
#include "blocks_common.h"

namespace t2l {

struct BlkTiles {
  const void *x_a, *x_b, *mem_a, *mem_b, *mem2_a, *mem2_b;
  void *o_a, *o_b;
  void *t1_a, *t1_b, *t2_a, *t2_b;  // decoder: the x tile after the first / second residual + LayerNorm (null: not wanted)
  TileGroups gx, gm, gm2;
  int form;  // attention: 0 one mem tile (mem null: self-attention), 1 two mem tiles in the product's order, 2 the first pass of form 1 alone
};

// planes: raw copies, no conversion (the bits of hi and lo are the state under test)
__device__ void blk_planes_in(const FP t, const void* a, const void* b, int wg) {
  const _Float16* ga = reinterpret_cast<const _Float16*>(a) + (size_t)wg * 32 * kFD;
  const _Float16* gb = reinterpret_cast<const _Float16*>(b) + (size_t)wg * 32 * kFD;
  for (int i = threadIdx.x; i < 32 * kLdF; i += 256) {
    const int r = i / kLdF, c = i % kLdF;
    t.hi[i] = c < kFD ? ga[r * kFD + c] : (_Float16)0.f;
    t.lo[i] = c < kFD ? gb[r * kFD + c] : (_Float16)0.f;
  }
}
__device__ void blk_planes_out(const FP t, void* a, void* b, int wg) {
  _Float16* ga = reinterpret_cast<_Float16*>(a) + (size_t)wg * 32 * kFD;
  _Float16* gb = reinterpret_cast<_Float16*>(b) + (size_t)wg * 32 * kFD;
  for (int i = threadIdx.x; i < 32 * kFD; i += 256) {
    const int r = i / kFD, c = i % kFD;
    ga[i] = t.hi[r * kLdF + c];
    gb[i] = t.lo[r * kLdF + c];
  }
}
__device__ void blk_rows_in(float* t, const void* a, int wg) {
  const float* g = reinterpret_cast<const float*>(a) + (size_t)wg * 32 * kFD;
  for (int i = threadIdx.x; i < 32 * kFS; i += 256) {
    const int r = i / kFS, c = i % kFS;
    t[i] = c < kFD ? g[r * kFD + c] : 0.f;
  }
}
__device__ void blk_rows_out(const float* t, void* a, int wg) {
  float* g = reinterpret_cast<float*>(a) + (size_t)wg * 32 * kFD;
  for (int i = threadIdx.x; i < 32 * kFD; i += 256) g[i] = t[(i / kFD) * kFS + (i % kFD)];
}

// the in-layer taps (fine.hip: FNoTap): the x tile as it stands, copied out by the whole workgroup (behind the pass's own barrier)
struct BlkTapPlanes {
  BlkTiles T;
  int wg;
  __device__ __forceinline__ void operator()(int which, const FP& x) const {
    void *a = which ? T.t2_a : T.t1_a, *b = which ? T.t2_b : T.t1_b;
    if (a) blk_planes_out(x, a, b, wg);
  }
};
struct BlkTapRows {
  BlkTiles T;
  int wg;
  __device__ __forceinline__ void operator()(int which, const float* x) const {
    void* a = which ? T.t2_a : T.t1_a;
    if (a) blk_rows_out(x, a, wg);
  }
};

constexpr size_t kBlkLds = (size_t)4 * kTileBytes + 256 * sizeof(float);  // four tiles in either form + the LayerNorm row sums

// One attention block alone. The out tile is read first: the rows a call must leave alone are checked against what they held.
template <int H>
__global__ __launch_bounds__(256) void blk_fine_attention_kernel(FPacked in_proj, BlkTiles T) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int wg = blockIdx.x;
  const bool self = T.mem_a == nullptr;
  if constexpr (H != 0) {
    char* base = reinterpret_cast<char*>(sm);
    const FP x = fp_at(base), mem = fp_at(base + kTileBytes), mem2 = fp_at(base + 2 * kTileBytes), obuf = fp_at(base + 3 * kTileBytes);
    blk_planes_in(x, T.x_a, T.x_b, wg);
    if (!self) blk_planes_in(mem, T.mem_a, T.mem_b, wg);
    if (T.form == 1) blk_planes_in(mem2, T.mem2_a, T.mem2_b, wg);
    blk_planes_in(obuf, T.o_a, T.o_b, wg);
    __syncthreads();
    if (T.form == 0) {
      if (self) fp_attention<H, false>(x, T.gx, x, T.gx, true, in_proj, obuf);
      else fp_attention<H, false>(x, T.gx, mem, T.gm, false, in_proj, obuf);
    } else {
      fp_attention<H, true>(x, T.gx, mem, T.gm, false, in_proj, obuf);
      if (T.form == 1) fp_attention<H, true>(x, T.gx, mem2, T.gm2, false, in_proj, obuf);
    }
    __syncthreads();
    blk_planes_out(obuf, T.o_a, T.o_b, wg);
  } else {
    float *x = sm, *mem = x + 32 * kFS, *mem2 = mem + 32 * kFS, *obuf = mem2 + 32 * kFS;
    blk_rows_in(x, T.x_a, wg);
    if (!self) blk_rows_in(mem, T.mem_a, wg);
    if (T.form == 1) blk_rows_in(mem2, T.mem2_a, wg);
    blk_rows_in(obuf, T.o_a, wg);
    __syncthreads();
    if (T.form == 0) {
      if (self) f_attention_regs(x, T.gx, x, T.gx, in_proj, obuf);
      else f_attention_regs(x, T.gx, mem, T.gm, in_proj, obuf);
    } else {
      f_attention_regs(x, T.gx, mem, T.gm, in_proj, obuf);
      if (T.form == 1) f_attention_regs<true>(x, T.gx, mem2, T.gm2, in_proj, obuf);
    }
    __syncthreads();
    blk_rows_out(obuf, T.o_a, wg);
  }
}

// One whole decoder pass: fp_decoder<H> / f_decoder on the tiles of workgroup wg; the x tile comes back in o.
template <int H>
__global__ __launch_bounds__(256) void blk_fine_decoder_kernel(FDecoder D, BlkTiles T) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int wg = blockIdx.x;
  float* red = sm + 4 * kTileBytes / 4;
  if constexpr (H != 0) {
    char* base = reinterpret_cast<char*>(sm);
    const FP x = fp_at(base), mem = fp_at(base + kTileBytes), mem2 = fp_at(base + 2 * kTileBytes), buf = fp_at(base + 3 * kTileBytes);
    blk_planes_in(x, T.x_a, T.x_b, wg);
    blk_planes_in(mem, T.mem_a, T.mem_b, wg);
    if (T.mem2_a) blk_planes_in(mem2, T.mem2_a, T.mem2_b, wg);
    __syncthreads();
    const BlkTapPlanes tap{T, wg};
    if (T.mem2_a) fp_decoder<H>(x, T.gx, mem, T.gm, D, buf, red, &mem2, T.gm2, tap);
    else fp_decoder<H>(x, T.gx, mem, T.gm, D, buf, red, nullptr, TileGroups{0, 0, 0, 0}, tap);
    blk_planes_out(x, T.o_a, T.o_b, wg);
  } else {
    float *x = sm, *mem = x + 32 * kFS, *mem2 = mem + 32 * kFS, *buf = mem2 + 32 * kFS;
    blk_rows_in(x, T.x_a, wg);
    blk_rows_in(mem, T.mem_a, wg);
    if (T.mem2_a) blk_rows_in(mem2, T.mem2_a, wg);
    __syncthreads();
    const BlkTapRows tap{T, wg};
    if (T.mem2_a) f_decoder(x, T.gx, mem, T.gm, D, buf, mem2, T.gm2, tap);
    else f_decoder(x, T.gx, mem, T.gm, D, buf, nullptr, TileGroups{0, 0, 0, 0}, tap);
    blk_rows_out(x, T.o_a, wg);
  }
}

// the three forms whose float32 error the bounds of tests/fine_blocks.py cannot derive from the code: as fine.hip spells them
__global__ void blk_fine_probe_kernel(const float* __restrict__ in, float* __restrict__ e, float* __restrict__ rs, float* __restrict__ rc, int n) {
  blk_probe_body(in, e, rs, rc, n);
}

static bool blk_groups(const int32_t* g, TileGroups* out, int* kind) {  // kind: 0 / 1 object tile A / B, 2 the hint tile
  if (!g) return false;
  *out = TileGroups{g[0], g[1], g[2], g[3]};
  if (g[2] != 32) return false;
  if (g[0] == 4 && g[1] >= 1 && g[1] <= kFObj && (g[3] == 0 || g[3] == 2)) {
    *kind = g[3] == 0 ? 0 : 1;
    return true;
  }
  if (g[0] == 3 && g[1] >= 1 && g[1] <= kFHintMax && g[3] == 0) {
    *kind = 2;
    return true;
  }
  return false;
}
static const FDecoder* blk_layer(const std::string& who, t2l_ctx* ctx, int which, int layer) {
  FineWeights* W = ctx ? reinterpret_cast<FineWeights*>(ctx->fine) : nullptr;
  if (!W) {
    blk_refuse(who + ": no context, or fine weights not loaded (t2l_fine_load_weights)");
    return nullptr;
  }
  const FineParams& P = W->p;
  const bool ok = P.n_layers == 0 ? (which == 1 && layer == 0) : ((which == 0 || which == 1) && layer >= 0 && layer < P.n_layers);
  if (!ok) {
    blk_refuse(who + ": no such decoder (which = 0 cross_objects / 1 cross_hints, layer < n_layers; a 0-layer model has cross_hints 0 only)");
    return nullptr;
  }
  return which ? &P.hint[layer] : &P.obj[layer];
}

}  // namespace t2l

using namespace t2l;

extern "C" {

// One attention block of decoder (which, layer): ca = 0 the self-attention in-projection, 1 the cross-attention one. form as BlkTiles.
// o (the obuf tile) is read AND written: rows the block does not write keep what they held.
int t2l_blk_fine_attention(t2l_ctx* ctx, int arm, int n_wg, int which, int layer, int ca, int form, const void* x_a, const void* x_b,
                           const int32_t* gx, const void* mem_a, const void* mem_b, const int32_t* gm, const void* mem2_a,
                           const void* mem2_b, const int32_t* gm2, void* o_a, void* o_b) {
  const std::string who = "t2l_blk_fine_attention";
  const FDecoder* D = blk_layer(who, ctx, which, layer);
  if (!D) return -1;
  if (arm < 0 || arm > 2 || n_wg < 1 || n_wg > 4096 || form < 0 || form > 2 || (ca != 0 && ca != 1))
    return blk_refuse(who + ": need arm 0..2, 1 <= n_wg <= 4096, form 0..2, ca 0 / 1");
  const bool planes = arm != 0, self = mem_a == nullptr;
  if (!x_a || !o_a || (planes && (!x_b || !o_b))) return blk_refuse(who + ": null x or o tile (arms 1, 2 take two planes each)");
  if (self && form != 0) return blk_refuse(who + ": self-attention (mem null) is form 0");
  if (!self && planes && !mem_b) return blk_refuse(who + ": null mem lo plane");
  if (form == 1 && (!mem2_a || (planes && !mem2_b))) return blk_refuse(who + ": form 1 needs the mem2 tile");
  BlkTiles T{x_a, x_b, mem_a, mem_b, form == 1 ? mem2_a : nullptr, form == 1 ? mem2_b : nullptr, o_a, o_b, nullptr, nullptr, nullptr, nullptr,
             {}, {}, {}, form};
  int kx = 0, km = 0, km2 = 0;
  if (!blk_groups(gx, &T.gx, &kx)) return blk_refuse(who + ": gx is none of the tile groups the product builds");
  if (!self && !blk_groups(gm, &T.gm, &km)) return blk_refuse(who + ": gm is none of the tile groups the product builds");
  if (form == 1 && !blk_groups(gm2, &T.gm2, &km2)) return blk_refuse(who + ": gm2 is none of the tile groups the product builds");
  const FPacked in_proj = ca ? D->ca_in : D->sa_in;
  auto failed = [&](hipError_t e) {
    if (e != hipSuccess) blk_refuse(who + ": " + hipGetErrorString(e));
    return e != hipSuccess;
  };
  if (failed(hipSetDevice(ctx->device))) return -2;
#define T2L_BLK_LAUNCH(K)                                                                                                        \
  do {                                                                                                                           \
    if (failed(hipFuncSetAttribute(reinterpret_cast<const void*>(&K), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBlkLds))) \
      return -2;                                                                                                                 \
    hipLaunchKernelGGL(K, dim3(n_wg), dim3(256), kBlkLds, nullptr, in_proj, T);                                                  \
  } while (0)
  if (arm == 0) T2L_BLK_LAUNCH(blk_fine_attention_kernel<0>);
  else if (arm == 1) T2L_BLK_LAUNCH(blk_fine_attention_kernel<1>);
  else T2L_BLK_LAUNCH(blk_fine_attention_kernel<2>);
#undef T2L_BLK_LAUNCH
  return blk_finish("t2l_blk_fine_attention");
}

// One decoder pass of decoder (which, layer) in the product's two arrangements: an object tile (gx A or B) over the hint tile, or
// the hint tile over object tiles A (mem) and B (mem2). o receives the x tile; x itself is not written. t1 / t2 (optional, both planes or
// neither for arms 1, 2): the x tile after the first / second residual + LayerNorm.
int t2l_blk_fine_decoder(t2l_ctx* ctx, int arm, int n_wg, int which, int layer, const void* x_a, const void* x_b, const int32_t* gx,
                         const void* mem_a, const void* mem_b, const int32_t* gm, const void* mem2_a, const void* mem2_b,
                         const int32_t* gm2, void* o_a, void* o_b, void* t1_a, void* t1_b, void* t2_a, void* t2_b) {
  const std::string who = "t2l_blk_fine_decoder";
  const FDecoder* D = blk_layer(who, ctx, which, layer);
  if (!D) return -1;
  if (arm < 0 || arm > 2 || n_wg < 1 || n_wg > 4096) return blk_refuse(who + ": need arm 0..2, 1 <= n_wg <= 4096");
  const bool planes = arm != 0;
  if (!x_a || !o_a || !mem_a || (planes && (!x_b || !o_b || !mem_b))) return blk_refuse(who + ": null x, mem or o tile (arms 1, 2 take two planes each)");
  if (planes && ((t1_a == nullptr) != (t1_b == nullptr) || (t2_a == nullptr) != (t2_b == nullptr)))
    return blk_refuse(who + ": a tap of arms 1, 2 takes both planes or neither");
  BlkTiles T{x_a, x_b, mem_a, mem_b, mem2_a, mem2_b, o_a, o_b, t1_a, t1_b, t2_a, t2_b, {}, {}, {}, 0};
  int kx = 0, km = 0, km2 = 0;
  if (!blk_groups(gx, &T.gx, &kx) || !blk_groups(gm, &T.gm, &km)) return blk_refuse(who + ": gx / gm is none of the tile groups the product builds");
  if (kx == 2) {  // hints over the two object tiles
    if (!mem2_a || (planes && !mem2_b) || !blk_groups(gm2, &T.gm2, &km2) || km != 0 || km2 != 1)
      return blk_refuse(who + ": the hint tile attends object tile A (mem) and object tile B (mem2)");
  } else if (km != 2 || mem2_a || mem2_b) {
    return blk_refuse(who + ": an object tile attends the hint tile alone");
  }
  const FDecoder Dv = *D;
  auto failed = [&](hipError_t e) {
    if (e != hipSuccess) blk_refuse(who + ": " + hipGetErrorString(e));
    return e != hipSuccess;
  };
  if (failed(hipSetDevice(ctx->device))) return -2;
#define T2L_BLK_LAUNCH(K)                                                                                                        \
  do {                                                                                                                           \
    if (failed(hipFuncSetAttribute(reinterpret_cast<const void*>(&K), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBlkLds))) \
      return -2;                                                                                                                 \
    hipLaunchKernelGGL(K, dim3(n_wg), dim3(256), kBlkLds, nullptr, Dv, T);                                                       \
  } while (0)
  if (arm == 0) T2L_BLK_LAUNCH(blk_fine_decoder_kernel<0>);
  else if (arm == 1) T2L_BLK_LAUNCH(blk_fine_decoder_kernel<1>);
  else T2L_BLK_LAUNCH(blk_fine_decoder_kernel<2>);
#undef T2L_BLK_LAUNCH
  return blk_finish("t2l_blk_fine_decoder");
}

// e[i] = __expf(in[i]), rs[i] = 1.0f / sqrtf(in[i]), rc[i] = 1.f / in[i] as this translation unit compiles them (profiles/fine_blocks.md)
int t2l_blk_fine_probe(const float* in, float* e, float* rs, float* rc, int n) {
  const std::string who = "t2l_blk_fine_probe";
  if (!in || !e || !rs || !rc || n < 1 || n > (1 << 24)) return blk_refuse(who + ": null pointer, or n outside 1..2^24");
  hipLaunchKernelGGL(blk_fine_probe_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, in, e, rs, rc, n);
  return blk_finish("t2l_blk_fine_probe");
}

}  // extern "C"
