// Dev-only block library (libt2l_blocks.so; never shipped, not part of include/t2l.h): ONE call of planes_layer — the post-norm
// transformer layer that the two-cell cell encoder and the one-launch t2l_text_inter share — on planes the test packed, with every
// in-layer stage copied out, so that tests/test_gpu_encode_blocks.py can hold every element of every stage against a float64 reference
// (tests/encode_blocks.py). This translation unit IS encode.hip plus the wrappers below and is linked in encode.o's place: the weights
// are the ones the context's own loaders packed (t2l_load_weights: EncParams::layer; t2l_text_head_load_weights: the InterFusedW of
// the inter-sentence layer, through blk_text_inter_weights of text_head_blocks.hip), the device function is the product's.
//
// The stage kernel copies the X planes of a workgroup's two token tiles from global memory into LDS (raw _Float16 hi and lo planes
// as the test packed them, no conversion: hi + lo re-split is not the identity), fills the B planes with f16 NaN (whatever the layer
// reads there it has to have written), calls planes_layer ONCE with the tap below and copies out.
//
//   inst 0  the cell encoder's instance <SG, 256, 64, 2, false>, mask j < 28, layer `layer` of the loaded model (S must be 0)
//   inst 1  the text layer's instance <SG, D, HD, 4, true> at the loaded head's (D, heads), mask grp[i] == grp[j], grp = row / S
//   arm 1   split-f16 (SG = false), arm 2 plain f16 (SG = true)
//
// Planes travel as [n_wg][2 tiles][32][D] _Float16, hi and lo apart; the hidden tap as [n_wg][FFP passes][2][32][D]; the f32 result
// (last_to_f32) as float [n_wg][2][32][D]. Taps are optional (both planes or neither); bad is int32 [n_wg].
//
// t2l_blk_enc_normalize: normalize_rows ONCE on an f32 tile (the two-cell kernel's feature-slot normalise).
// t2l_blk_enc_small_mlp: small_mlp<IN> (hidden layer, gemm32, normalize_rows) ONCE with the loaded model's folded and packed weights.
//
// Not here: taps inside encode_cells2_kernel and encode_cells_shaped_kernel. Moving either __global__ body into a device function
// changed the shipped listing (register allocation), so those kernels keep their text (profiles/encode_blocks.md).
//
// Return: 0, -1 (refused, message through t2l_blk_last_error; nothing was launched), -2 (the HIP runtime reported an error). The
// launch is synchronised before a wrapper returns.
#include "encode.hip"
#include "blocks_common.h"

namespace t2l {

struct BlkLayerIO {
  const _Float16 *x_h, *x_l;
  _Float16 *att_h, *att_l;  // the B planes behind the attention
  _Float16 *x1_h, *x1_l;    // the X planes behind the first residual + LayerNorm
  _Float16 *hid_h, *hid_l;  // the B planes of every feed-forward pass
  _Float16 *out_h, *out_l;  // the X planes behind the second residual + LayerNorm (last_to_f32 == 0)
  float* out_f;             // ... or the f32 [32][D + 4] tiles it left in the B-plane regions, without their padding
  int32_t* bad;
  int S, last_to_f32;
};

// both tiles of a workgroup, plane pair `which` (0: X, 1: B) -> global [2][32][D]
template <int D>
__device__ __forceinline__ void blk_pl_out(_Float16* base, int which, _Float16* gh, _Float16* gl) {
  constexpr int LDP = PlaneGeo<D>::kLd;
  for (int i = threadIdx.x; i < 2 * kSP * D; i += 2 * D) {
    const int t = i / (kSP * D), r = (i / D) % kSP, c = i % D;
    const _Float16 *ph = which ? pl_bh<D>(base, t) : pl_xh<D>(base, t), *pl = which ? pl_bl<D>(base, t) : pl_xl<D>(base, t);
    gh[i] = ph[r * LDP + c];
    gl[i] = pl[r * LDP + c];
  }
}

template <int D, int FFP>
struct BlkLayerTap {
  _Float16* base;
  BlkLayerIO io;
  int wg;
  __device__ __forceinline__ void operator()(int where, int c) const {
    const size_t tile2 = (size_t)2 * kSP * D;
    if (where == 0) {
      if (io.att_h) blk_pl_out<D>(base, 1, io.att_h + wg * tile2, io.att_l + wg * tile2);
    } else if (where == 1) {
      if (io.x1_h) blk_pl_out<D>(base, 0, io.x1_h + wg * tile2, io.x1_l + wg * tile2);
    } else if (io.hid_h) {
      blk_pl_out<D>(base, 1, io.hid_h + ((size_t)wg * FFP + c) * tile2, io.hid_l + ((size_t)wg * FFP + c) * tile2);
    }
  }
};

template <int D>
constexpr size_t blk_layer_lds() {
  return (size_t)8 * PlaneGeo<D>::kSize * sizeof(_Float16) + kSP * sizeof(int) + (size_t)4 * PlaneGeo<D>::kWaves * 32 * sizeof(float);
}

template <bool SG, int D, int HD, int FFP, bool TEXT>
__global__ __launch_bounds__(2 * D, D == 256 ? 1 : 2) void blk_enc_layer_kernel(InterFusedW W, BlkLayerIO io) {
  constexpr int LDP = PlaneGeo<D>::kLd, LDX = PlaneGeo<D>::kLdF, PLANE = PlaneGeo<D>::kSize;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  _Float16* base = reinterpret_cast<_Float16*>(smem);
  int* grp = reinterpret_cast<int*>(base + (size_t)8 * PLANE);
  float* lnred = reinterpret_cast<float*>(grp + kSP);
  const int tid = threadIdx.x, wg = blockIdx.x;
  const size_t tile2 = (size_t)2 * kSP * D;
  const _Float16 nan16 = __builtin_bit_cast(_Float16, (unsigned short)0x7E00);
  for (int i = tid; i < 2 * PLANE; i += 2 * D) {
    const int t = i / PLANE, r = (i % PLANE) / LDP, c = i % LDP;
    const size_t g = wg * tile2 + ((size_t)t * kSP + r) * D + c;
    pl_xh<D>(base, t)[r * LDP + c] = c < D ? io.x_h[g] : (_Float16)0.f;
    pl_xl<D>(base, t)[r * LDP + c] = c < D ? io.x_l[g] : (_Float16)0.f;
    pl_bh<D>(base, t)[r * LDP + c] = nan16;
    pl_bl<D>(base, t)[r * LDP + c] = nan16;
  }
  if (TEXT && tid < kSP) grp[tid] = tid / io.S;
  __syncthreads();
  bool bad = false;
  const BlkLayerTap<D, FFP> tap{base, io, wg};
  if constexpr (TEXT)
    planes_layer<SG, D, HD, FFP, true>(base, W, [&](int i, int j) { return grp[i] == grp[j]; }, bad, io.last_to_f32 != 0, lnred, tap);
  else
    planes_layer<SG, D, HD, FFP, false>(base, W, [](int, int j) { return j < kS; }, bad, io.last_to_f32 != 0, lnred, tap);
  if (io.last_to_f32) {
    for (int i = tid; i < 2 * kSP * D; i += 2 * D) {
      const int t = i / (kSP * D), r = (i / D) % kSP, c = i % D;
      io.out_f[wg * tile2 + i] = reinterpret_cast<const float*>(pl_bh<D>(base, t))[r * LDX + c];
    }
  } else {
    blk_pl_out<D>(base, 0, io.out_h + wg * tile2, io.out_l + wg * tile2);
  }
  const int any = __syncthreads_or(bad ? 1 : 0);
  if (tid == 0) io.bad[wg] = any;
}

// the three forms whose float32 error the bounds of tests/encode_blocks.py cannot derive from the code: as this translation unit
// compiles them (the body is blocks_common.h's, shared with fine_blocks.hip's probe)
__global__ void blk_enc_probe_kernel(const float* __restrict__ in, float* __restrict__ e, float* __restrict__ rs, float* __restrict__ rc, int n) {
  blk_probe_body(in, e, rs, rc, n);
}

// normalize_rows (the two-cell kernel's feature-slot normalise, 256 wide, one cell's four waves) ONCE on an f32 tile [32][260] in LDS
__global__ __launch_bounds__(256) void blk_enc_normalize_kernel(float* __restrict__ x, int nvalid) {
  __shared__ __attribute__((aligned(16))) float tile[kSP * kLdX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* g = x + (size_t)blockIdx.x * kSP * kD;
  for (int i = tid; i < kSP * kLdX; i += 256) {
    const int r = i / kLdX, c = i % kLdX;
    tile[i] = c < kD ? g[r * kD + c] : __builtin_nanf("");  // (the padding is never read)
  }
  __syncthreads();
  normalize_rows(tile, kLdX, nvalid, wave, lane);
  __syncthreads();
  for (int i = tid; i < kSP * kD; i += 256) g[i] = tile[(i / kD) * kLdX + (i % kD)];
}

// small_mlp<IN> (the two-cell kernel's feature branch: hidden layer on the VALU, gemm32 on the f32 MFMA, normalize_rows) ONCE with one
// cell's four waves: in [32][IN] of this workgroup in global memory, as the product reads it; the slot comes back as f32 [32][256]
template <int IN>
__global__ __launch_bounds__(256) void blk_enc_small_mlp_kernel(SmallMlp m, const float* __restrict__ in, int is_num, int nobj, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float hbuf[kSP * kLdH];
  __shared__ __attribute__((aligned(16))) float dst[kSP * kLdX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < kSP * kLdX; i += 256) dst[i] = __builtin_nanf("");
  for (int i = tid; i < kSP * kLdH; i += 256) hbuf[i] = __builtin_nanf("");
  __syncthreads();
  small_mlp<IN>(m, in + (size_t)blockIdx.x * kSP * IN, is_num != 0, nobj, hbuf, dst, tid, wave, lane);
  __syncthreads();
  float* g = out + (size_t)blockIdx.x * kSP * kD;
  for (int i = tid; i < kSP * kD; i += 256) g[i] = dst[(i / kD) * kLdX + (i % kD)];
}

template <bool SG, int D, int HD, int FFP, bool TEXT>
static int blk_layer_launch(const std::string& who, int n_wg, const InterFusedW& W, const BlkLayerIO& io) {
  constexpr size_t lds = blk_layer_lds<D>();
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&blk_enc_layer_kernel<SG, D, HD, FFP, TEXT>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) {
    blk_refuse(who + ": " + hipGetErrorString(e));
    return -2;
  }
  hipLaunchKernelGGL((blk_enc_layer_kernel<SG, D, HD, FFP, TEXT>), dim3(n_wg), dim3(2 * D), lds, nullptr, W, io);
  return blk_finish("t2l_blk_enc_layer");
}

}  // namespace t2l

using namespace t2l;

extern "C" {

int t2l_blk_enc_layer(t2l_ctx* ctx, int inst, int arm, int n_wg, int layer, int S, int last_to_f32, const void* x_h, const void* x_l, void* att_h,
                      void* att_l, void* x1_h, void* x1_l, void* hid_h, void* hid_l, void* out_h, void* out_l, void* out_f, int32_t* bad) {
  const std::string who = "t2l_blk_enc_layer";
  if (!ctx) return blk_refuse(who + ": no context");
  if ((inst != 0 && inst != 1) || (arm != 1 && arm != 2) || n_wg < 1 || n_wg > 4096 || (last_to_f32 != 0 && last_to_f32 != 1))
    return blk_refuse(who + ": need inst 0 / 1, arm 1 (split-f16) / 2 (plain f16), 1 <= n_wg <= 4096, last_to_f32 0 / 1");
  if (!x_h || !x_l || !bad) return blk_refuse(who + ": null x planes or bad");
  if ((att_h == nullptr) != (att_l == nullptr) || (x1_h == nullptr) != (x1_l == nullptr) || (hid_h == nullptr) != (hid_l == nullptr))
    return blk_refuse(who + ": a tap takes both planes or neither");
  if (last_to_f32 ? !out_f : (!out_h || !out_l)) return blk_refuse(who + ": null result (out_f with last_to_f32, else out_h and out_l)");
  InterFusedW W;
  int D = 0, heads = 0;
  if (inst == 0) {
    const EncoderWeights* ew = ctx->enc;
    if (!ew) return blk_refuse(who + ": encoder weights not loaded (t2l_load_weights)");
    if (!ew->published() || !ew->p.split_ok)
      return blk_refuse(who + ": the two-cell kernel runs at the published shape (256, 4 heads, 28 slots) with weights that bound the f16 range only");
    if (layer < 0 || layer >= ew->p.num_layers) return blk_refuse(who + ": no such layer of the loaded model");
    if (S != 0) return blk_refuse(who + ": the cell instance has no S (pass 0)");
    const LayerW& L = ew->p.layer[layer];
    W.in_hp = L.in_hp; W.out_hp = L.out_hp; W.ff1_hp = L.ff1_hp; W.ff2_hp = L.ff2_hp;
    W.in_b = L.in_b; W.out_b = L.out_b; W.ff1_b = L.ff1_b; W.ff2_b = L.ff2_b;
    W.ln1_w = L.ln1_w; W.ln1_b = L.ln1_b; W.ln2_w = L.ln2_w; W.ln2_b = L.ln2_b;
    D = kD;
    heads = 4;
  } else {
    if (!blk_text_inter_weights(ctx, &W, &D, &heads)) return blk_refuse(who + ": no text head with an inter layer of a compiled shape loaded (t2l_text_head_load_weights)");
    if (layer != 0) return blk_refuse(who + ": the text head has one inter layer (layer 0)");
    if (S < 1 || S > kSP) return blk_refuse(who + ": need 1 <= S <= 32");
  }
  if (!W.in_hp || !W.out_hp || !W.ff1_hp || !W.ff2_hp || !W.in_b || !W.out_b || !W.ff1_b || !W.ff2_b || !W.ln1_w || !W.ln1_b || !W.ln2_w || !W.ln2_b)
    return blk_refuse(who + ": the loaded layer has a null array");
  const BlkLayerIO io{reinterpret_cast<const _Float16*>(x_h), reinterpret_cast<const _Float16*>(x_l), reinterpret_cast<_Float16*>(att_h),
                      reinterpret_cast<_Float16*>(att_l),   reinterpret_cast<_Float16*>(x1_h),      reinterpret_cast<_Float16*>(x1_l),
                      reinterpret_cast<_Float16*>(hid_h),   reinterpret_cast<_Float16*>(hid_l),     reinterpret_cast<_Float16*>(out_h),
                      reinterpret_cast<_Float16*>(out_l),   reinterpret_cast<float*>(out_f),        bad, S, last_to_f32};
  if (hipSetDevice(ctx->device) != hipSuccess) {
    blk_refuse(who + ": hipSetDevice failed");
    return -2;
  }
  const bool sg = arm == 2;
  const int hd = heads > 0 ? D / heads : 0;
  if (inst == 0) return sg ? blk_layer_launch<true, kD, 64, 2, false>(who, n_wg, W, io) : blk_layer_launch<false, kD, 64, 2, false>(who, n_wg, W, io);
#define T2L_BLK_SHAPE(DD, HH) \
  if (D == DD && hd == HH) return sg ? blk_layer_launch<true, DD, HH, 4, true>(who, n_wg, W, io) : blk_layer_launch<false, DD, HH, 4, true>(who, n_wg, W, io);
  T2L_BLK_SHAPE(256, 64)
  T2L_BLK_SHAPE(128, 32)
  T2L_BLK_SHAPE(128, 64)
  T2L_BLK_SHAPE(256, 32)
#undef T2L_BLK_SHAPE
  return blk_refuse(who + ": no kernel for the loaded inter layer");
}

// F.normalize over the 256 columns of rows < nvalid of x (float [n_wg][32][256], in place), rows >= nvalid zeroed: normalize_rows
int t2l_blk_enc_normalize(int n_wg, float* x, int nvalid) {
  const std::string who = "t2l_blk_enc_normalize";
  if (n_wg < 1 || n_wg > 4096 || !x || nvalid < 0 || nvalid > kSP) return blk_refuse(who + ": need 1 <= n_wg <= 4096, a tile, 0 <= nvalid <= 32");
  hipLaunchKernelGGL(blk_enc_normalize_kernel, dim3(n_wg), dim3(256), 0, nullptr, x, nvalid);
  return blk_finish("t2l_blk_enc_normalize");
}

// One feature branch of the loaded model (published width) through small_mlp: sub 0 pos_encoder (in [n_wg][32][3]), 1 color_encoder
// (the same; a model loaded with color_embed == 0), 2 num_encoder (in [n_wg][32][1], normalised as the kernel does). Rows >= nobj are
// zeroed. out: float [n_wg][32][256].
int t2l_blk_enc_small_mlp(t2l_ctx* ctx, int sub, int n_wg, const float* in, int nobj, float* out) {
  const std::string who = "t2l_blk_enc_small_mlp";
  const EncoderWeights* ew = ctx ? ctx->enc : nullptr;
  if (!ew) return blk_refuse(who + ": no context, or encoder weights not loaded");
  if (ew->embed_dim != kD) return blk_refuse(who + ": small_mlp is the 256-wide kernel's");
  if (n_wg < 1 || n_wg > 4096 || !in || !out || nobj < 0 || nobj > kSP) return blk_refuse(who + ": need 1 <= n_wg <= 4096, in, out, 0 <= nobj <= 32");
  const EncParams& E = ew->p;
  const SmallMlp* m = sub == 0 && E.use_pos ? &E.pos : sub == 1 && E.use_color && !E.color_embed ? &E.color : sub == 2 && E.use_num ? &E.num : nullptr;
  if (!m || !m->w1 || !m->b1 || !m->w2p || !m->b2) return blk_refuse(who + ": the loaded model has no such small encoder (sub 0 pos, 1 color MLP, 2 num)");
  if (hipSetDevice(ctx->device) != hipSuccess) {
    blk_refuse(who + ": hipSetDevice failed");
    return -2;
  }
  if (sub == 2) hipLaunchKernelGGL(blk_enc_small_mlp_kernel<1>, dim3(n_wg), dim3(256), 0, nullptr, *m, in, 1, nobj, out);
  else hipLaunchKernelGGL(blk_enc_small_mlp_kernel<3>, dim3(n_wg), dim3(256), 0, nullptr, *m, in, 0, nobj, out);
  return blk_finish("t2l_blk_enc_small_mlp");
}

// e[i] = __expf(in[i]), rs[i] = 1.0f / sqrtf(in[i]), rc[i] = 1.f / in[i] as this translation unit compiles them (profiles/encode_blocks.md)
int t2l_blk_enc_probe(const float* in, float* e, float* rs, float* rc, int n) {
  const std::string who = "t2l_blk_enc_probe";
  if (!in || !e || !rs || !rc || n < 1 || n > (1 << 24)) return blk_refuse(who + ": null pointer, or n outside 1..2^24");
  hipLaunchKernelGGL(blk_enc_probe_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, in, e, rs, rc, n);
  return blk_finish("t2l_blk_enc_probe");
}

}  // extern "C"
