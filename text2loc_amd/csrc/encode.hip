// The cell encoder at the published shape (256, 4 heads, 28 slots) in its default form, the fused t2l_text_inter layer at every compiled
// (width, heads), and the weight loader of every encoder kernel.
//
// encode_cells2_kernel: ObjectEncoder.forward (models/object_encoder.py:66-153, eval mode) +
// CellRetrievalNetwork.encode_objects (models/cell_retrieval.py:65-110) as ONE kernel, two cells per eight-wave workgroup, every
// intermediate resident in LDS. The one-cell kernel — every other compiled shape, the all-f32 arithmetic, single-feature models,
// option encoder_two_cells = 0 — is encode_shaped.hip; encode_impl below chooses.
//
//   per object (<= 28 kept, cell_retrieval.py:94-98):
//     class  = normalize(class_embedding[idx])           | normalize(mlp_pointnet(features2))
//     color  = normalize(color_embedding[idx])           | normalize(color_encoder(mean rgb))
//     pos    = normalize(pos_encoder(center)),  num = normalize(num_encoder((n-mean)/std))
//     merged = relu(BN(Linear(cat)))  -> normalize                       (trailing ReLU, language_encoder.py:15)
//   x[28,256] zero padded -> 2 x TransformerEncoderLayer (post-norm, ReLU, NO padding mask: zero slots are
//   attended to and attend) -> max over the 28 slots -> normalize.
//
// The big contractions (feature merge, q/k/v, out_proj, feed-forward: 97 % of the FLOPs) run as SPLIT-f16 on
// v_mfma_f32_32x32x16_f16: every f32 value a is used as hi + lo with hi = f16(a), lo = f16(a - hi) (22 significand bits;
// gfx950's MFMA honours f16 denormals, tools/ probe) and a product is hi*hi + hi*lo + lo*hi with f32 accumulation —
// ~5e-7 relative, well inside the 1e-3 parity budget (measured 2e-6 on the goldens) at 1/5 of the matrix-pipe time of
// v_mfma_f32_32x32x2_f32. Activations are split on the fly (20 VALU per 8 values), weights at load time. f16 overflows at
// 65504: t2l_load_weights bounds every activation that enters a split GEMM from the weights (LayerNorm gain/bias,
// row norms) and sends models that could exceed it to the all-f32 one-cell kernel (option encoder_f32 forces it).
// The attention core (S = K Q^T, P V) and the small MLPs stay on the f32 MFMA.
// M = 32 rows = the 28 slots + 4 dead rows (masked out of the softmax keys and the max-pool).
// Weights are BN-folded and re-laid out on the host into MFMA B-fragment order
// [n_tile][k_step][lane][4] so every wave-level weight load is one coalesced 1 KiB line.
// The MFMA's k-sum is order-free, so lane (col, half) owns k in [half*K/2, (half+1)*K/2): both operands
// are read as contiguous float4 (LDS rows padded by 4 floats -> conflict-free ds_read_b128).
#include <math.h>
#include <string.h>

#include <memory>

#include "t2l_internal.h"
#include "encode_shared.h"

#ifndef T2L_ENC_UNROLL
#define T2L_ENC_UNROLL 4
#endif

namespace t2l {

constexpr int kLdX = kD + 4;        // 260: row stride of every 256-wide LDS buffer
constexpr int kLdH = 64 + 4;        // 68   (hidden layer of the small MLPs)

// out[32][N] = A[32][K] @ W^T ; the 4 waves split N in 32-column tiles, two tiles at a time per wave
// (tiles w+8p and w+8p+4) sharing the A fragments. epi(t, r, row, col, value) is called for every element
// (t = which tile of the pair, r = accumulator register; both compile-time after unrolling).
template <typename Epi>
__device__ __forceinline__ void gemm32(const float* __restrict__ A, int lda, int K, const float4* __restrict__ Wp,
                                       int N, int wave, int lane, Epi epi) {
  const int col = lane & 31, half = lane >> 5;
  const int qn = K >> 3;
  const float* arow = A + col * lda + half * (K >> 1);
  for (int p = 0; p < (N >> 8); ++p) {
    const int nt0 = wave + 8 * p, nt1 = nt0 + 4;
    const float4* w0 = Wp + (size_t)nt0 * qn * 64 + lane;
    const float4* w1 = Wp + (size_t)nt1 * qn * 64 + lane;
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      acc0[r] = 0.f;
      acc1[r] = 0.f;
    }
#pragma unroll 4
    for (int q = 0; q < qn; ++q) {
      const float4 a = *reinterpret_cast<const float4*>(arow + 4 * q);
      const float4 b0 = w0[q * 64];
      const float4 b1 = w1[q * 64];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b0.x, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b1.x, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b0.y, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b1.y, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b0.z, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b1.z, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b0.w, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b1.w, acc1, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = acc_row(r, half);
      epi(0, r, row, nt0 * 32 + col, acc0[r]);
      epi(1, r, row, nt1 * 32 + col, acc1[r]);
    }
  }
}

// F.normalize over 256 columns of `rows` rows starting at buf (row stride ld); rows >= nvalid are zeroed. (One float4 per lane at the
// published width; normalize_rows_d of encode_shaped.hip and f_normalize_rows of fine.hip differ in access width and in what they zero.)
__device__ __forceinline__ void normalize_rows(float* buf, int ld, int nvalid, int wave, int lane) {
  for (int i = wave; i < kSP; i += 4) {
    float4* p = reinterpret_cast<float4*>(buf + i * ld) + lane;
    float4 v = *p;
    if (i < nvalid) {
      const float ss = wave_sum(v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w);
      const float inv = 1.f / fmaxf(sqrtf(ss), 1e-12f);
      v.x *= inv;
      v.y *= inv;
      v.z *= inv;
      v.w *= inv;
    } else {
      v = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    *p = v;
  }
}

// One feature branch through get_mlp([in,64,256]): hidden layer on the VALU (K = 1 or 3), 64->256 on MFMA.
template <int IN>
__device__ __forceinline__ void small_mlp(const SmallMlp& m, const float* __restrict__ in /* [nobj][IN] global */,
                                          bool is_num, int nobj, float* hbuf, float* dst /* [32][kLdX] */, int tid,
                                          int wave, int lane) {
  // hidden: 32 objects x 64 units, 8 per thread
  for (int e = tid; e < kSP * 64; e += 256) {
    const int o = e >> 6, u = e & 63;
    float acc = 0.f;
    if (o < nobj) {
      acc = m.b1[u];
#pragma unroll
      for (int k = 0; k < IN; ++k) {
        float v = in[o * IN + k];
        if (is_num) v = (v - kNumMean) / kNumStd;  // object_encoder.py:143
        acc += m.w1[u * IN + k] * v;
      }
      acc = fmaxf(acc, 0.f);
    }
    hbuf[o * kLdH + u] = acc;
  }
  __syncthreads();
  const float* b2 = m.b2;
  gemm32(hbuf, kLdH, 64, m.w2p, kD, wave, lane,
         [&](int, int, int row, int col, float v) { dst[row * kLdX + col] = fmaxf(v + b2[col], 0.f); });
  __syncthreads();
  normalize_rows(dst, kLdX, nobj, wave, lane);
}

// ------------------------------------------------------------------------------------------------
// t2l_text_inter as ONE launch (models/language_encoder.py:137-147): x = sent.view(B, S, D); x += TransformerEncoderLayer(D, heads,
// ff 4 D, post-norm, ReLU)(x) over the S sentences of a description; max over the sentences. Compiled for D in {128, 256} with heads of
// 32 or 64 features; (256, 4 heads) is the published model. The layer is the cell encoder's
// (encode_shaped.hip) with three differences: a 32-row tile holds floor(32 / S) whole DESCRIPTIONS and a query attends to the keys of its own
// description only (block-diagonal mask; rows past the tile's last description are zero rows that form groups of their own: every
// softmax has its own row as a key, nothing is NaN); the feed-forward hidden layer is 4 D wide = four passes through the B planes
// (pass c = hidden units [c D/2, (c + 1) D/2) and 2 D + [c D/2, (c + 1) D/2): what k-steps [c D/16, (c + 1) D/16) of W2's half-split
// packing at K = 4 D cover); and the inputs are not bounded by the weights (they come out of inter_mlp), so every value that enters a
// split-f16 product is watched against the f16 range at run time: a tile that leaves it raises *flag and the caller redoes the batch
// on the PyTorch modules (the protocol of t2l_text_head).
// (The kernel: text_inter_fused2_kernel below — two tiles per workgroup of D / 32 waves on LDS planes. The one-tile form on f32 tiles that
// this comment used to head was removed in round 5: 0.208 vs 0.179 ms for 4,096 descriptions x 6 sentences.)

// ------------------------------------------------------------------------------------------------
// The launch — the testbed for the lever the encoder family is left with (the packed-weight
// stream out of the L2 is worth 23-32 % of these kernels, the per-MFMA VALU work another third): TWO row tiles per workgroup of D / 32
// waves (EIGHT at the published width), every activation resident in LDS as split-f16 PLANES (hi | lo, rows of D + 8 halves), so that
//  * out_proj, linear1 and linear2 (3/4 of the FLOPs) load each weight fragment ONCE for both tiles — wave w owns one 32-wide tile of
//    output features and multiplies it into both token tiles (products computed transposed: A = weight fragment, B = token fragment);
//  * no operand is split in a GEMM loop: a token fragment is two ds_read_b128; the splitting happens once per produced element in the
//    epilogues, which hold 4 consecutive features per register quad (transposed C layout) and store 8-byte plane pieces;
//  * the attention runs as in the one-cell encoder, 64 / head_dim (tile, head) pairs per wave, q/k/v projected per tile (their fragments are
//    not shared), with O^T = V^T P^T so that its output has the same store-friendly layout.
// 135 KB of LDS at D = 256: one workgroup (two waves per SIMD) per CU; 70 KB at D = 128: two workgroups of four waves, the same two waves
// per SIMD, and the second workgroup covers the first one's barriers. The residual is rebuilt from hi + lo (22 significand bits).
#ifndef T2L_RING_DEPTH
#define T2L_RING_DEPTH 3
#endif
#ifndef T2L_QK_RING
#define T2L_QK_RING 2
#endif
constexpr int kQkRing = T2L_QK_RING;  // the same for the q / k projection (four weight tiles = 32 VGPRs per step; v: twice as deep)
constexpr int kRingDepth = T2L_RING_DEPTH;  // k-steps of weight fragments in flight per wave in the row-wise products (8 VGPRs per step)
// plane geometry at width D: rows of D + 8 halves (528 B at 256, 272 B at 128: rows 4 banks apart, as the f32 tiles of D + 4 floats)
template <int D>
struct PlaneGeo {
  static constexpr int kLd = D + 8;          // halves per plane row
  static constexpr int kSize = kSP * kLd;    // halves per plane
  static constexpr int kLdF = D + 4;         // floats per row of the f32 tile the last LayerNorm may leave in a tile's B planes
  static constexpr int kWaves = D / 32;      // waves of the workgroup: one per 32-wide tile of output features
};
constexpr int kLdP = PlaneGeo<kD>::kLd;   // the published width (the two-cell cell encoder below)
constexpr int kPlane = PlaneGeo<kD>::kSize;

template <int D = kD>
__device__ __forceinline__ _Float16* pl_xh(_Float16* base, int t) { return base + (size_t)(4 * t + 0) * PlaneGeo<D>::kSize; }
template <int D = kD>
__device__ __forceinline__ _Float16* pl_xl(_Float16* base, int t) { return base + (size_t)(4 * t + 1) * PlaneGeo<D>::kSize; }
template <int D = kD>
__device__ __forceinline__ _Float16* pl_bh(_Float16* base, int t) { return base + (size_t)(4 * t + 2) * PlaneGeo<D>::kSize; }
template <int D = kD>
__device__ __forceinline__ _Float16* pl_bl(_Float16* base, int t) { return base + (size_t)(4 * t + 3) * PlaneGeo<D>::kSize; }

// One post-norm TransformerEncoderLayer (d_model D, heads of HD features, ReLU, feed-forward of D * FFP units) over the TWO 32-row token
// tiles of a workgroup of D / 32 waves, in place on the tiles' X planes (B planes: scratch). mask(i, j): may query row i see key row j
// (tile-local)? WATCH: run-time f16-range watch on everything that enters a split product (`bad`). last_to_f32: the final LayerNorm
// leaves f32 [32][D + 4] tiles in the B-plane regions instead of planes (for an epilogue that needs full precision). Ends behind a
// barrier. lnred: 4 * (D / 32) * 32 floats of LDS scratch (the row sums of the fused residual + LayerNorm epilogues).
// Compiled for D in {128, 256} and HD in {32, 64}; <256, 64> is the published shape: every constant below is then what the 256-only
// form of this function spelled out, and its users return the same bits at the same speed.
//   * the 2 D / HD (tile, head) pairs go 64 / HD to a wave (pair p = tile p / NH, head p % NH): a 64-wide head is two 32-row tiles of
//     q^T, k^T and v, a 32-wide head is one (the score contraction is then two k-steps instead of four);
//   * wave w owns output-feature tile w of out_proj, linear1 and linear2 for both token tiles;
//   * pass c of the feed-forward covers k-steps [c D/16, (c + 1) D/16) of linear2's half-split packing at K = FFP D (mfma_h3.h:
//     lane half kh of step s holds k = kh K/2 + 8 s ..), i.e. hidden units [c D/2, (c + 1) D/2) in columns [0, D/2) of the B planes and
//     units K/2 + [c D/2, (c + 1) D/2) in columns [D/2, D): waves below D / 64 compute the former's tiles, the others the latter's.
// tap(where, c): an empty functor in the product; the dev block library (encode_blocks.hip) copies the planes out behind the layer's own
// barriers — where = 0 the B planes behind the attention, 1 the X planes behind the first residual + LayerNorm, 2 the B planes of
// feed-forward pass c.
struct PlNoTap {
  __device__ __forceinline__ void operator()(int, int) const {}
};
template <bool SG, int D, int HD, int FFP, bool WATCH, typename Mask, typename TAP = PlNoTap>
__device__ __forceinline__ void planes_layer(_Float16* base, const InterFusedW& W, Mask mask, bool& bad, bool last_to_f32, float* lnred,
                                             const TAP& tap = TAP()) {
  static_assert(D == 128 || D == 256, "one wave per 32-wide feature tile, four or eight waves");
  static_assert(HD == 32 || HD == 64, "a head is one or two 32-row tiles of q^T / k^T / v");
  constexpr int LDP = PlaneGeo<D>::kLd, LDX = PlaneGeo<D>::kLdF, NW = PlaneGeo<D>::kWaves;
  constexpr int KH = D / 2;       // k-values per lane half of a K = D product
  constexpr int HS = D / 16;      // k-steps of a K = D product
  constexpr int DT = D / 32;      // 32-row weight tiles per q / k / v block of in_proj
  constexpr int NH = D / HD;      // heads
  constexpr int LNH = NH == 2 ? 1 : NH == 4 ? 2 : 3;  // log2(NH)
  constexpr int TPH = HD / 32;    // weight tiles per head
  constexpr int PPW = 64 / HD;    // (tile, head) pairs per wave
  constexpr float kScale = HD == 64 ? 0.125f : 0.17677669529663687f;  // 1 / sqrt(head_dim)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 31, half = lane >> 5;
  auto watch = [&](float v) { bad = bad || !(fabsf(v) < kSplitF16Safe); };
  auto watch4 = [&](h3_f32x4 v) { watch(v[0]); watch(v[1]); watch(v[2]); watch(v[3]); };
  (void)watch4;
#pragma unroll
  for (int pp = 0; pp < PPW; ++pp) {  // ---- self-attention: wave -> (tile t, head h); q^T, k^T, v from the tile's planes, scores / softmax / O^T from registers
    const int t = (wave * PPW + pp) >> LNH, h = (wave * PPW + pp) & (NH - 1);
    const float* ib = W.in_b;
    const _Float16 *xh = pl_xh<D>(base, t) + col * LDP + half * KH, *xl = pl_xl<D>(base, t) + col * LDP + half * KH;
    f32x16 st;
    float inv;
    {
      f32x16 qT[TPH], kT[TPH];
#pragma unroll
      for (int j = 0; j < TPH; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) qT[j][r] = kT[j][r] = 0.f;
      const uint4* hqk[2 * TPH];  // the head's q tiles, then its k tiles
#pragma unroll
      for (int j = 0; j < TPH; ++j) {
        hqk[j] = W.in_hp + ((size_t)(TPH * h + j) * HS * 64 + lane) * 2;
        hqk[TPH + j] = W.in_hp + ((size_t)(DT + TPH * h + j) * HS * 64 + lane) * 2;
      }
      {  // 2 TPH weight tiles per step through a ring kQkRing steps deep (8 VGPRs per tile and step). This ring and v's below are not
         // stream_weights (several tiles per step) and not fp_attention's ring (fine.hip: opaque pointer increments, depth T2L_ATT_RING):
         // merging any two would change one kernel's schedule.
        constexpr int RD = kQkRing;
        HFrag ring[RD][2 * TPH];
        auto loadqk = [&](int s, HFrag (&f)[2 * TPH]) {
#pragma unroll
          for (int e = 0; e < 2 * TPH; ++e) f[e] = load_h1<SG>(hqk[e] + T2L_HOT(s) * 128);
        };
#pragma unroll
        for (int i = 0; i < RD; ++i) loadqk(i, ring[i]);
#pragma unroll
        for (int s = 0; s < HS; ++s) {
          HFrag f[2 * TPH];
#pragma unroll
          for (int e = 0; e < 2 * TPH; ++e) f[e] = ring[s % RD][e];
          if (s + RD < HS) loadqk(s + RD, ring[s % RD]);
          __builtin_amdgcn_sched_barrier(0);
          const HFrag xf = plane_frag<SG>(xh, xl, 8 * s);
#pragma unroll
          for (int j = 0; j < TPH; ++j) mfma_h3<SG>(qT[j], f[j], xf);
#pragma unroll
          for (int j = 0; j < TPH; ++j) mfma_h3<SG>(kT[j], f[TPH + j], xf);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int f = acc_row(r, half);
#pragma unroll
        for (int j = 0; j < TPH; ++j) qT[j][r] += ib[h * HD + 32 * j + f];
#pragma unroll
        for (int j = 0; j < TPH; ++j) kT[j][r] += ib[D + h * HD + 32 * j + f];
      }
      // S^T = K Q^T (and O^T = V^T P^T below) as split-f16 products on the accumulator registers: kT / qT (v / P) sit in the same
      // MFMA output layout, so registers 0..7 and 8..15 of the two are matching k-halves of A and B — 12 MFMAs of 32 cycles here
      // (64-wide heads) instead of 32 f32 MFMAs of 64 (the attention core was a third of a wave's matrix-pipe time in this layer).
      // Always the three-product form (the logits carry the softmax); q, k, v are inside the load-time bound of the in_proj output
      // (cell encoder) or watched here (WATCH).
      if constexpr (WATCH) {
        float wm = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float wq = fabsf(qT[0][r]), wk = fabsf(kT[0][r]);
#pragma unroll
          for (int j = 1; j < TPH; ++j) {
            wq = fmaxf(wq, fabsf(qT[j][r]));
            wk = fmaxf(wk, fabsf(kT[j][r]));
          }
          wm = fmaxf(wm, fmaxf(wq, wk));
        }
        watch(wm);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
      for (int j = 0; j < TPH; ++j)
#pragma unroll
        for (int m2 = 0; m2 < 2; ++m2) {  // (fenced: the compiler otherwise splits all the fragments first — 64 registers of temporaries)
          mfma_h3<false>(st, split_acc8<false>(kT[j], m2), split_acc8<false>(qT[j], m2));
          __builtin_amdgcn_sched_barrier(0);
        }
      float m = -__builtin_inff();
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j = acc_row(r, half);
        st[r] = mask(col, j) ? st[r] * kScale : -__builtin_inff();
        m = fmaxf(m, st[r]);
      }
      m = fmaxf(m, __shfl_xor(m, 32));
      float sum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        st[r] = __expf(st[r] - m);
        sum += st[r];
      }
      sum += __shfl_xor(sum, 32);
      inv = 1.f / sum;
    }
    {
      f32x16 v[TPH];  // v straight: lane = feature column, register = token row
#pragma unroll
      for (int j = 0; j < TPH; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) v[j][r] = 0.f;
      const uint4* hv[TPH];
#pragma unroll
      for (int j = 0; j < TPH; ++j) hv[j] = W.in_hp + ((size_t)(2 * DT + TPH * h + j) * HS * 64 + lane) * 2;
      {
        constexpr int RD = 2 * kQkRing;
        HFrag ring[RD][TPH];
#pragma unroll
        for (int i = 0; i < RD; ++i)
#pragma unroll
          for (int j = 0; j < TPH; ++j) ring[i][j] = load_h1<SG>(hv[j] + T2L_HOT(i) * 128);
#pragma unroll
        for (int s = 0; s < HS; ++s) {
          HFrag f[TPH];
#pragma unroll
          for (int j = 0; j < TPH; ++j) f[j] = ring[s % RD][j];
          if (s + RD < HS) {
#pragma unroll
            for (int j = 0; j < TPH; ++j) ring[s % RD][j] = load_h1<SG>(hv[j] + T2L_HOT(s + RD) * 128);
          }
          __builtin_amdgcn_sched_barrier(0);
          const HFrag xf = plane_frag<SG>(xh, xl, 8 * s);
#pragma unroll
          for (int j = 0; j < TPH; ++j) mfma_h3<SG>(v[j], xf, f[j]);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      float bv[TPH];
#pragma unroll
      for (int j = 0; j < TPH; ++j) bv[j] = ib[2 * D + h * HD + 32 * j + col];
      // O^T[f][i] = sum_j v[j][f] P[i][j]: A = v registers (lane = feature, lane half = the key of register r), B = P registers (lane =
      // query i, lane half = the same key) -> lane = query (token row), register quad = 4 consecutive features
      f32x16 o[TPH];
#pragma unroll
      for (int j = 0; j < TPH; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[j][r] = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        st[r] *= inv;
#pragma unroll
        for (int j = 0; j < TPH; ++j) v[j][r] += bv[j];
      }
      if constexpr (WATCH) {
        float wm = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float wv = fabsf(v[0][r]);
#pragma unroll
          for (int j = 1; j < TPH; ++j) wv = fmaxf(wv, fabsf(v[j][r]));
          wm = fmaxf(wm, wv);
        }
        watch(wm);
      }
#pragma unroll
      for (int m2 = 0; m2 < 2; ++m2) {
        const HFrag pf = split_acc8<false>(st, m2);
#pragma unroll
        for (int j = 0; j < TPH; ++j) mfma_h3<false>(o[j], split_acc8<false>(v[j], m2), pf);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        h3_f32x4 ov[TPH];
#pragma unroll
        for (int j = 0; j < TPH; ++j) ov[j] = h3_f32x4{o[j][4 * q], o[j][4 * q + 1], o[j][4 * q + 2], o[j][4 * q + 3]};
        if constexpr (WATCH) {
#pragma unroll
          for (int j = 0; j < TPH; ++j) watch4(ov[j]);
        }
#pragma unroll
        for (int j = 0; j < TPH; ++j)
          plane_put4(pl_bh<D>(base, t), pl_bl<D>(base, t), col * LDP + h * HD + 32 * j + 8 * q + 4 * half, ov[j]);
      }
    }
  }
  __syncthreads();
  tap(0, 0);
  // operand fragments of the row-wise products: token fragment of tile t at k-step s (this lane's row `col`, k half `half`)
  const int frow = col * LDP + half * KH;
  // x = LayerNorm(x + acc^T + bias) * g + be for both tiles — the residual epilogue and the LayerNorm behind it in one go (round 5; proven
  // on fine.hip first). A lane holds 16 of a token's D features per tile (its partner lane ^ 32 another 16, the other waves 32
  // each): the row sums meet in `lnred` behind two light barriers (mean, then centred squares: the two-pass form), the values stay in
  // registers in between and the normalised rows are written once. As a separate pass (8 rows per wave, two full-wave reductions per
  // row) the two LayerNorms of a layer were ~700 VALU instructions per wave and a plane round trip each.
  // Stands beside fine.hip's fp_epilogue_ln, not merged with it: the waves' row sums are added one after the other here, pairwise
  // there — another association, other bits.
  auto resid_ln = [&](const f32x16 (&acc)[2], const float* __restrict__ bias, const float* __restrict__ g, const float* __restrict__ be,
                      bool to_f32) {
    h3_f32x4 v[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      float sm = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int f0 = 32 * wave + 8 * q + 4 * half;
        const float4 bb = *reinterpret_cast<const float4*>(bias + f0);
        v[t][q] = plane_get4(pl_xh<D>(base, t), pl_xl<D>(base, t), col * LDP + f0) +
                  h3_f32x4{acc[t][4 * q] + bb.x, acc[t][4 * q + 1] + bb.y, acc[t][4 * q + 2] + bb.z, acc[t][4 * q + 3] + bb.w};
        sm += (v[t][q][0] + v[t][q][1]) + (v[t][q][2] + v[t][q][3]);
      }
      sm += __shfl_xor(sm, 32);
      if (half == 0) lnred[(t * NW + wave) * 32 + col] = sm;
    }
    __syncthreads();
    float mean[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      float m = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) m += lnred[(t * NW + w) * 32 + col];
      mean[t] = m * (1.f / D);
      float qs = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        v[t][q] -= mean[t];
        qs += (v[t][q][0] * v[t][q][0] + v[t][q][1] * v[t][q][1]) + (v[t][q][2] * v[t][q][2] + v[t][q][3] * v[t][q][3]);
      }
      qs += __shfl_xor(qs, 32);
      if (half == 0) lnred[2 * NW * 32 + (t * NW + wave) * 32 + col] = qs;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      float var = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) var += lnred[2 * NW * 32 + (t * NW + w) * 32 + col];
      const float inv = 1.f / sqrtf(var * (1.f / D) + 1e-5f);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int f0 = 32 * wave + 8 * q + 4 * half;
        const float4 gg = *reinterpret_cast<const float4*>(g + f0), bb = *reinterpret_cast<const float4*>(be + f0);
        const h3_f32x4 o = {v[t][q][0] * inv * gg.x + bb.x, v[t][q][1] * inv * gg.y + bb.y, v[t][q][2] * inv * gg.z + bb.z,
                            v[t][q][3] * inv * gg.w + bb.w};
        if (to_f32) {  // (the last LayerNorm: the tile's B planes become one f32 [32][D + 4] tile for the epilogue)
          *reinterpret_cast<h3_f32x4*>(reinterpret_cast<float*>(pl_bh<D>(base, t)) + col * LDX + f0) = o;
        } else {
          if constexpr (WATCH) watch4(o);
          plane_put4(pl_xh<D>(base, t), pl_xl<D>(base, t), col * LDP + f0, o);
        }
      }
    }
  };
  {  // ---- x = x + o @ out_proj^T + b, transposed: wave w owns output features [32 w, 32 w + 32) for BOTH tiles
    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const uint4* wp = W.out_hp + ((size_t)wave * HS * 64 + lane) * 2;
    stream_weights<SG, HS, kRingDepth>(wp, [&](int s, const HFrag& wf) {
#pragma unroll
      for (int t = 0; t < 2; ++t) mfma_h3<SG>(acc[t], wf, plane_frag<SG>(pl_bh<D>(base, t) + frow, pl_bl<D>(base, t) + frow, 8 * s));
    });
    resid_ln(acc, W.out_b, W.ln1_w, W.ln1_b, false);
  }
  __syncthreads();
  tap(1, 0);
  {  // ---- feed-forward, FFP passes of D hidden units; wave w: one hidden tile per pass and one output tile, both token tiles
    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const float* b1 = W.ff1_b;
    constexpr int FS = FFP * HS;   // k-steps of one W2 tile (K = FFP D)
    constexpr int LOW = NW / 2;    // waves whose hidden tile lies in the lower k half of W2, = 32-unit tiles per pass and k half
    const int cbase = wave < LOW ? 32 * wave : KH + 32 * (wave - LOW);  // where this wave's hidden tile lives in the B planes
    for (int c = 0; c < FFP; ++c) {
      const int tf = wave < LOW ? LOW * c + wave : LOW * FFP + LOW * c + (wave - LOW);
      f32x16 hT[2];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) hT[t][r] = 0.f;
      const uint4* w1 = W.ff1_hp + ((size_t)tf * HS * 64 + lane) * 2;
      stream_weights<SG, HS, kRingDepth>(w1, [&](int s, const HFrag& wf) {
#pragma unroll
        for (int t = 0; t < 2; ++t) mfma_h3<SG>(hT[t], wf, plane_frag<SG>(pl_xh<D>(base, t) + frow, pl_xl<D>(base, t) + frow, 8 * s));
      });
      if (c) __syncthreads();  // every wave has consumed the previous pass from the B planes
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int u0 = 8 * q + 4 * half;
          const float4 bb = *reinterpret_cast<const float4*>(b1 + tf * 32 + u0);
          const h3_f32x4 v = {fmaxf(hT[t][4 * q] + bb.x, 0.f), fmaxf(hT[t][4 * q + 1] + bb.y, 0.f), fmaxf(hT[t][4 * q + 2] + bb.z, 0.f),
                              fmaxf(hT[t][4 * q + 3] + bb.w, 0.f)};
          if constexpr (WATCH) watch4(v);
          plane_put4(pl_bh<D>(base, t), pl_bl<D>(base, t), col * LDP + cbase + u0, v);
        }
      __syncthreads();
      tap(2, c);
      const uint4* w2 = W.ff2_hp + (((size_t)wave * FS + HS * c) * 64 + lane) * 2;
      stream_weights<SG, HS, kRingDepth>(w2, [&](int s, const HFrag& wf) {
#pragma unroll
        for (int t = 0; t < 2; ++t) mfma_h3<SG>(acc[t], wf, plane_frag<SG>(pl_bh<D>(base, t) + frow, pl_bl<D>(base, t) + frow, 8 * s));
      });
    }
    resid_ln(acc, W.ff2_b, W.ln2_w, W.ln2_b, last_to_f32);  // (every wave is past its reads of the B planes and of x at the first barrier inside)
  }
  __syncthreads();
}

template <int D, int HD, int H>
__global__ __launch_bounds__(2 * D, D == 256 ? 1 : 2) void text_inter_fused2_kernel(InterFusedW W, const float* __restrict__ sent, int n_desc, int S, int dpt,
                                                                   float* __restrict__ out, int* __restrict__ flag) {
  static_assert(H == 1 || H == 2, "split-f16 or plain f16");
  constexpr bool SG = H == 2;
  constexpr int LDP = PlaneGeo<D>::kLd, LDX = PlaneGeo<D>::kLdF, PLANE = PlaneGeo<D>::kSize;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  _Float16* base = reinterpret_cast<_Float16*>(smem);
  // per tile t: X planes (token tile), B planes (attention output -> hidden pass; at the very end an f32 [32][D + 4] tile)
  auto XH = [&](int t) { return base + (size_t)(4 * t + 0) * PLANE; };
  auto XL = [&](int t) { return base + (size_t)(4 * t + 1) * PLANE; };
  auto BH = [&](int t) { return base + (size_t)(4 * t + 2) * PLANE; };
  auto BL = [&](int t) { return base + (size_t)(4 * t + 3) * PLANE; };
  int* grp = reinterpret_cast<int*>(base + (size_t)8 * PLANE);  // [32]: description of a tile-local row
  float* lnred = reinterpret_cast<float*>(grp + kSP);              // [4 NW 32]: row sums of the fused residual + LayerNorm epilogues
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 31, half = lane >> 5;
  const int d0 = blockIdx.x * 2 * dpt;
  bool bad = false;
  auto watch = [&](float v) { bad = bad || !(fabsf(v) < kSplitF16Safe); };
  auto watch4 = [&](h3_f32x4 v) { watch(v[0]); watch(v[1]); watch(v[2]); watch(v[3]); };
  int nd[2], rows[2];
  nd[0] = min(dpt, n_desc - d0);
  nd[1] = max(0, min(dpt, n_desc - d0 - dpt));
  rows[0] = nd[0] * S;
  rows[1] = nd[1] * S;
  // ---- the 64 rows -> planes (64 / NW rows per wave, 4 columns per lane: a wave takes 256 / D rows per step)
  constexpr int RPI = 256 / D, LPR = D / 4, LLPR = D == 256 ? 6 : 5;  // rows per step, lanes per row and their log2
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int r = (wave * 8 + i) * RPI + (lane >> LLPR), t = r >> 5, lr = r & 31, cl = lane & (LPR - 1);
    h3_f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (lr < rows[t]) {
      const float4 g = reinterpret_cast<const float4*>(sent + ((size_t)(d0 + t * dpt) * S + lr) * D)[cl];
      v = h3_f32x4{g.x, g.y, g.z, g.w};
    }
    watch4(v);
    plane_put4(XH(t), XL(t), lr * LDP + 4 * cl, v);
  }
  if (tid < kSP) grp[tid] = tid / S;
  __syncthreads();

  planes_layer<SG, D, HD, 4, true>(base, W, [&](int i, int j) { return grp[i] == grp[j]; }, bad, true, lnred);
  {  // x_in + layer(x_in), max over the description's S sentences: thread = (tile, column)
    const int t = tid >> (D == 256 ? 8 : 7), c = tid & (D - 1);
    const float* y = reinterpret_cast<const float*>(BH(t));
    const float* src = sent + (size_t)(d0 + t * dpt) * S * D;
    for (int d = 0; d < nd[t]; ++d) {
      float m = -__builtin_inff();
      for (int s_ = 0; s_ < S; ++s_) {
        const int r = d * S + s_;
        m = fmaxf(m, y[r * LDX + c] + src[(size_t)r * D + c]);
      }
      out[(size_t)(d0 + t * dpt + d) * D + c] = m;
    }
  }
  if (__syncthreads_or(bad ? 1 : 0) && tid == 0) atomicOr(flag, 1);
}

// ------------------------------------------------------------------------------------------------
// encode_cells, second form (option encoder_two_cells, split-f16 / plain-f16 arithmetic, at least two feature slots): the recipe that
// t2l_text_inter's second form proved — TWO cells per workgroup of EIGHT waves, activations as split-f16 planes in LDS,
// the weight fragments of the feature merge, out_proj and both feed-forward Linears loaded once for both cells and requested ahead of
// the MFMAs, nothing split inside a GEMM loop. The feature stage is the one-cell kernel's (small_mlp, gemm32, normalize_rows above): waves 4t .. 4t+3 build cell t's feature
// slot as a normalised f32 tile (in the cell's X-plane region, not live before the merge epilogue), convert it to the cell's B planes,
// and all eight waves contract both cells' slot with its slice of the merge weight.
template <int H>
__global__ __launch_bounds__(512, 1) void encode_cells2_kernel(EncParams P, t2l_packed_cells in, float* __restrict__ out) {
  static_assert(H == 1 || H == 2, "split-f16 or plain f16 (the all-f32 encoder is the one-cell kernel)");
  constexpr bool SG = H == 2;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  _Float16* base = reinterpret_cast<_Float16*>(smem);
  float* hb_all = reinterpret_cast<float*>(base + (size_t)8 * kPlane);  // [2][32][68]: hidden layer of the small MLPs
  float* red = hb_all + 2 * kSP * kLdH;                                 // [8]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 31, half = lane >> 5;
  const int tc = wave >> 2, lw = wave & 3, ltid = tid & 255;  // the cell this wave builds features for, its wave / thread index there
  int cell[2], obj0[2], nobj[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    cell[t] = min((int)blockIdx.x * 2 + t, in.n_cells - 1);  // an odd tail workgroup computes its last cell twice
    obj0[t] = in.offsets[cell[t]];
    nobj[t] = min(in.offsets[cell[t] + 1] - obj0[t], kS);
  }
  float* xf32 = reinterpret_cast<float*>(pl_xh(base, tc));  // this wave group's f32 [32][260] scratch tile (X-plane region of its cell)
  float* bf32 = reinterpret_cast<float*>(pl_bh(base, tc));  // ... and the B-plane region as one (features2 staging only)
  float* hb = hb_all + tc * kSP * kLdH;
  const int my_nobj = nobj[tc], my_obj0 = obj0[tc];
  const int frow = col * kLdP + half * 128;

  f32x16 keep[2];  // merge accumulators, transposed: wave w = output features [32 w, 32 w + 32), lane = object slot
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) keep[t][r] = 0.f;
  int slot = 0;
  auto tile_to_planes = [&]() {  // the group's normalised f32 slot (X region) -> its cell's B planes
    for (int i = lw; i < kSP; i += 4) {
      const float4 g = *(reinterpret_cast<const float4*>(xf32 + i * kLdX) + lane);
      plane_put4(pl_bh(base, tc), pl_bl(base, tc), i * kLdP + 4 * lane, h3_f32x4{g.x, g.y, g.z, g.w});
    }
  };
  auto table_to_planes = [&](const float* __restrict__ tab, const int32_t* __restrict__ idx, int n_tab) {
    for (int o = lw; o < kSP; o += 4) {
      h3_f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (o < my_nobj) {
        const int ci = min(max(idx[my_obj0 + o], 0), n_tab - 1);
        const float4 g = reinterpret_cast<const float4*>(tab + (size_t)ci * kD)[lane];
        v = h3_f32x4{g.x, g.y, g.z, g.w};
      }
      plane_put4(pl_bh(base, tc), pl_bl(base, tc), o * kLdP + 4 * lane, v);
    }
  };
  auto merge_slot = [&]() {  // both cells' B planes hold slot `slot`: keep += Wmerge[:, 256 slot : 256 slot + 256] @ slot^T
    __syncthreads();
    const uint4* wp = P.merge_hp + (size_t)slot * (kD * kD / 4) + ((size_t)wave * (kD / 16) * 64 + lane) * 2;
    stream_weights<SG, kD / 16, kRingDepth>(wp, [&](int s, const HFrag& wf) {
#pragma unroll
      for (int t = 0; t < 2; ++t) mfma_h3<SG>(keep[t], wf, plane_frag<SG>(pl_bh(base, t) + frow, pl_bl(base, t) + frow, 8 * s));
    });
    ++slot;
    __syncthreads();
  };
  if (P.use_class) {
    if (P.class_embed) {
      table_to_planes(P.class_tab, in.class_idx, P.n_class);
    } else {  // features2 -> mlp_pointnet (f32: an input, not bounded by the weights) -> normalize
      for (int o = lw; o < kSP; o += 4) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (o < my_nobj) v = reinterpret_cast<const float4*>(in.pn_feat + (size_t)(my_obj0 + o) * kD)[lane];
        reinterpret_cast<float4*>(bf32 + o * kLdX)[lane] = v;
      }
      __syncthreads();
      const float* pb = P.pn_b;
      gemm32(bf32, kLdX, kD, P.pn_wp, kD, lw, lane, [&](int, int, int row, int cc, float v) { xf32[row * kLdX + cc] = fmaxf(v + pb[cc], 0.f); });
      __syncthreads();
      normalize_rows(xf32, kLdX, my_nobj, lw, lane);
      __syncthreads();
      tile_to_planes();
    }
    merge_slot();
  }
  if (P.use_color) {
    if (P.color_embed) {
      table_to_planes(P.color_tab, in.color_idx, P.n_color);
    } else {
      small_mlp<3>(P.color, in.rgb + (size_t)my_obj0 * 3, false, my_nobj, hb, xf32, ltid, lw, lane);
      __syncthreads();
      tile_to_planes();
    }
    merge_slot();
  }
  if (P.use_pos) {
    small_mlp<3>(P.pos, in.center + (size_t)my_obj0 * 3, false, my_nobj, hb, xf32, ltid, lw, lane);
    __syncthreads();
    tile_to_planes();
    merge_slot();
  }
  if (P.use_num) {
    small_mlp<1>(P.num, in.n_pts + my_obj0, true, my_nobj, hb, xf32, ltid, lw, lane);
    __syncthreads();
    tile_to_planes();
    merge_slot();
  }
  {  // merge epilogue: relu(keep + b) -> X planes (lane = object slot, register quad = 4 consecutive features)
    const float* mb = P.merge_b;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int f0 = 32 * wave + 8 * q + 4 * half;
        const float4 bb = *reinterpret_cast<const float4*>(mb + f0);
        const h3_f32x4 v = {fmaxf(keep[t][4 * q] + bb.x, 0.f), fmaxf(keep[t][4 * q + 1] + bb.y, 0.f), fmaxf(keep[t][4 * q + 2] + bb.z, 0.f),
                            fmaxf(keep[t][4 * q + 3] + bb.w, 0.f)};
        plane_put4(pl_xh(base, t), pl_xl(base, t), col * kLdP + f0, v);
      }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 8; ++i) {  // F.normalize per object row; rows >= nobj are the zero pad slots (cell_retrieval.py:85,92)
    const int r = wave * 8 + i, t = r >> 5, lr = r & 31, off = lr * kLdP + 4 * lane;
    h3_f32x4 v = plane_get4(pl_xh(base, t), pl_xl(base, t), off);
    const float ss = wave_sum(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]);
    const float inv = lr < nobj[t] ? 1.f / fmaxf(sqrtf(ss), 1e-12f) : 0.f;
    v *= inv;
    plane_put4(pl_xh(base, t), pl_xl(base, t), off, v);
  }
  __syncthreads();
  bool bad = false;
  for (int l = 0; l < P.num_layers; ++l) {
    const LayerW& L = P.layer[l];
    InterFusedW W;
    W.in_hp = L.in_hp; W.out_hp = L.out_hp; W.ff1_hp = L.ff1_hp; W.ff2_hp = L.ff2_hp;
    W.in_b = L.in_b; W.out_b = L.out_b; W.ff1_b = L.ff1_b; W.ff2_b = L.ff2_b;
    W.ln1_w = L.ln1_w; W.ln1_b = L.ln1_b; W.ln2_w = L.ln2_w; W.ln2_b = L.ln2_b;
    // no padding mask: the 28 slots, zero pads included, attend and are attended to; the 4 dead rows of the tile are no keys
    planes_layer<SG, kD, 64, 2, false>(base, W, [](int, int j) { return j < kS; }, bad, l == P.num_layers - 1, hb_all);  // (hb_all: dead behind the feature MLPs)
  }
  {  // max over ALL 28 slots, then normalize: thread = (cell, column)
    const int t = tid >> 8, c = tid & 255;
    const float* y = reinterpret_cast<const float*>(pl_bh(base, t));
    float mx = y[c];
    for (int i = 1; i < kS; ++i) mx = fmaxf(mx, y[i * kLdX + c]);
    const float ss = wave_sum(mx * mx);
    if (lane == 0) red[wave] = ss;
    __syncthreads();
    const float nrm = sqrtf(red[4 * t] + red[4 * t + 1] + red[4 * t + 2] + red[4 * t + 3]);
    if ((int)blockIdx.x * 2 + t < in.n_cells) out[(size_t)cell[t] * kD + c] = mx / fmaxf(nrm, 1e-12f);
  }
}

template <int D, int HD>
static int text_inter_launch_shape(t2l_ctx* ctx, const InterFusedW& W, bool single, const float* sent, int n_desc, int S, float* out, int* flag,
                                   hipStream_t s) {
  const TextInterPlan plan = text_inter_plan(D, n_desc, S);
  static PerDeviceOnce once2;  // (one per instantiation)
  if (once2.need(ctx->device)) {
    T2L_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&text_inter_fused2_kernel<D, HD, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds_bytes));
    T2L_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&text_inter_fused2_kernel<D, HD, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds_bytes));
    once2.mark(ctx->device);
  }
  if (single)
    hipLaunchKernelGGL((text_inter_fused2_kernel<D, HD, 2>), dim3(plan.grid), dim3(plan.threads), plan.lds_bytes, s, W, sent, n_desc, S, plan.dpt, out, flag);
  else
    hipLaunchKernelGGL((text_inter_fused2_kernel<D, HD, 1>), dim3(plan.grid), dim3(plan.threads), plan.lds_bytes, s, W, sent, n_desc, S, plan.dpt, out, flag);
  T2L_HIP(ctx, hipGetLastError());
  return T2L_OK;
}

int text_inter_fused_launch(t2l_ctx* ctx, const InterFusedW& W, int D, int heads, bool single, const float* sent, int n_desc, int S, float* out,
                            int* flag, hipStream_t s) {
  const int hd = heads > 0 ? D / heads : 0;
#define T2L_INTER_SHAPE(DD, HH) \
  if (D == DD && hd == HH) return text_inter_launch_shape<DD, HH>(ctx, W, single, sent, n_desc, S, out, flag, s);
  T2L_INTER_SHAPE(256, 64)
  T2L_INTER_SHAPE(128, 32)
  T2L_INTER_SHAPE(128, 64)
  T2L_INTER_SHAPE(256, 32)
#undef T2L_INTER_SHAPE
  return fail(ctx, T2L_ESTATE, std::string("t2l_text_inter: no kernel for the loaded inter layer (") + text_inter_shapes_text() + ")");
}

// ---- host side: BN folding, fragment packing, upload -------------------------------------------
namespace {

std::vector<float> pack_h(const std::vector<float>& W, int N, int K) { return pack_split_f16(W.data(), nullptr, N, K, K); }
float max_abs(const float* v, size_t n) { return h3_max_abs(v, n); }
float max_row_norm(const float* W, int rows, int cols) { return h3_max_row_norm(W, rows, cols); }

std::vector<float> normalized_rows(const float* t, int rows, int D) {
  std::vector<float> o((size_t)rows * D);
  for (int r = 0; r < rows; ++r) {
    float ss = 0.f;
    for (int c = 0; c < D; ++c) ss += t[r * D + c] * t[r * D + c];
    const float inv = 1.f / fmaxf(sqrtf(ss), 1e-12f);
    for (int c = 0; c < D; ++c) o[(size_t)r * D + c] = t[r * D + c] * inv;
  }
  return o;
}

constexpr size_t kEncAlign = 16;  // the encoder's arrays sit 16-byte aligned in its blob (float4 / uint4 loads)

bool add_small(WeightTable& T, const std::string& pre, int in, int D, Staging* st, SmallMlp* m) {
  std::vector<float> W1, b1, W2, b2;
  if (!fold_linear(T, pre + ".0.0", pre + ".0.1", 64, in, &W1, &b1)) return false;
  if (!fold_linear(T, pre + ".1.0", pre + ".1.1", D, 64, &W2, &b2)) return false;
  st->place(&m->w1, W1, kEncAlign);
  st->place(&m->b1, b1, kEncAlign);
  st->place(&m->w2p, pack_half_split(W2, nullptr, D, 64, 64), kEncAlign);
  st->place(&m->b2, b2, kEncAlign);
  return true;
}

}  // namespace

void free_weights(t2l_ctx* ctx) {
  if (!ctx->enc) return;
  if (ctx->enc->blob) (void)hipFree(ctx->enc->blob);
  delete ctx->enc;
  ctx->enc = nullptr;
}

int encoder_embed_dim(const t2l_ctx* ctx) { return ctx->enc ? ctx->enc->embed_dim : kD; }

int load_weights_impl(t2l_ctx* ctx, const t2l_weight_desc* w, int n, const t2l_model_config* cfg, int D, int object_size) {
  if (!shape_is_compiled(D, cfg->num_heads, object_size))
    return fail(ctx, T2L_EINVAL, "t2l_load_weights: embed_dim " + std::to_string(D) + ", num_heads " + std::to_string(cfg->num_heads) +
                                     ", object_size " + std::to_string(object_size) + " is not built (" + compiled_shapes_text() + ")");
  if (cfg->num_layers < 1 || cfg->num_layers > 4) return fail(ctx, T2L_EINVAL, "t2l_load_weights: num_layers must be 1..4");
  const int nfeat = (cfg->use_class != 0) + (cfg->use_color != 0) + (cfg->use_position != 0) + (cfg->use_num != 0);
  if (nfeat < 1) return fail(ctx, T2L_EINVAL, "t2l_load_weights: use_features is empty");
  WeightTable T("t2l_load_weights", w, n);
  Staging blob;
  std::unique_ptr<EncoderWeights> ew(new EncoderWeights());
  EncParams& P = ew->p;
  memset(&P, 0, sizeof(P));
  auto put = [&](auto** field, const std::vector<float>& v) { blob.place(field, v, kEncAlign); };
  auto refused = [&]() { return fail(ctx, T2L_EINVAL, T.error()); };
  if (!T.ok()) return refused();
  const std::string oe = "object_encoder.";
  // an embedding table [rows][D], rows L2-normalised
  auto table = [&](const std::string& name, int* rows, const float** tab) -> bool {
    int64_t n_rows = 0;
    const float* t = T.need_rows(name, D, &n_rows);
    if (t) put(tab, normalized_rows(t, *rows = (int)n_rows, D));
    return t != nullptr;
  };
  // split-f16 safety (file header): largest weight, and an upper bound on |activation| entering a split GEMM
  float w_absmax = 0.f, act_bound = 1.f;  // merge inputs are unit rows
  if (cfg->use_class) {
    if (cfg->class_embed) {
      if (!table(oe + "class_embedding.weight", &P.n_class, &P.class_tab)) return refused();
    } else {
      std::vector<float> W, b;
      if (!fold_linear(T, oe + "mlp_pointnet.0.0", oe + "mlp_pointnet.0.1", D, 256, &W, &b)) return refused();  // features2 is 256 wide at every D
      put(&P.pn_wp, pack_half_split(W, nullptr, D, 256, 256));
      put(&P.pn_b, b);
      w_absmax = fmaxf(w_absmax, max_abs(W.data(), W.size()));
    }
  }
  if (cfg->use_color) {
    if (cfg->color_embed) {
      if (!table(oe + "color_embedding.weight", &P.n_color, &P.color_tab)) return refused();
    } else if (!add_small(T, oe + "color_encoder", 3, D, &blob, &P.color)) {
      return refused();
    }
  }
  if (cfg->use_position && !add_small(T, oe + "pos_encoder", 3, D, &blob, &P.pos)) return refused();
  if (cfg->use_num && !add_small(T, oe + "num_encoder", 1, D, &blob, &P.num)) return refused();
  if (nfeat > 1) {
    std::vector<float> W, b;
    if (!fold_linear(T, oe + "mlp_merge.0.0", oe + "mlp_merge.0.1", D, nfeat * D, &W, &b)) return refused();
    {  // one (N=256, K=256) packing per feature slot, consecutive
      std::vector<float> all, all_h;
      for (int sl = 0; sl < nfeat; ++sl) {
        std::vector<float> Ws((size_t)D * D);
        for (int n = 0; n < D; ++n)
          for (int k = 0; k < D; ++k) Ws[(size_t)n * D + k] = W[(size_t)n * nfeat * D + sl * D + k];
        const std::vector<float> ps = pack_half_split(Ws, nullptr, D, D, D);
        all.insert(all.end(), ps.begin(), ps.end());
        const std::vector<float> ph = pack_h(Ws, D, D);
        all_h.insert(all_h.end(), ph.begin(), ph.end());
      }
      put(&P.merge_wp, all);
      put(&P.merge_hp, all_h);
      w_absmax = fmaxf(w_absmax, max_abs(W.data(), W.size()));
    }
    put(&P.merge_b, b);
  }
  float x_norm = 1.f;  // bound on the 2-norm of a token row entering the layer (layer 0: unit rows or zero pads)
  for (int l = 0; l < cfg->num_layers; ++l) {
    const std::string p = "obj_inter_module." + std::to_string(l) + ".";
    LayerW& L = P.layer[l];
    auto lin = [&](const std::string& wn, const std::string& bn, int out, int in, const float4** wp, const uint4** hp, const float** bo) -> bool {
      const float* W = T.need(p + wn, (int64_t)out * in);
      const float* b = T.need(p + bn, out);
      if (!W || !b) return false;
      const std::vector<float> Wv(W, W + (size_t)out * in);
      put(wp, pack_half_split(Wv, nullptr, out, in, in));
      put(hp, pack_h(Wv, out, in));
      put(bo, std::vector<float>(b, b + out));
      w_absmax = fmaxf(w_absmax, max_abs(W, Wv.size()));
      return true;
    };
    auto vec = [&](const std::string& name, const float** o) -> bool {
      const float* v = T.need(p + name, D);
      if (!v) return false;
      put(o, std::vector<float>(v, v + D));
      return true;
    };
    if (!lin("self_attn.in_proj_weight", "self_attn.in_proj_bias", 3 * D, D, &L.in_wp, &L.in_hp, &L.in_b) ||
        !lin("self_attn.out_proj.weight", "self_attn.out_proj.bias", D, D, &L.out_wp, &L.out_hp, &L.out_b) ||
        !lin("linear1.weight", "linear1.bias", 2 * D, D, &L.ff1_wp, &L.ff1_hp, &L.ff1_b) ||
        !lin("linear2.weight", "linear2.bias", D, 2 * D, &L.ff2_wp, &L.ff2_hp, &L.ff2_b) || !vec("norm1.weight", &L.ln1_w) ||
        !vec("norm1.bias", &L.ln1_b) || !vec("norm2.weight", &L.ln2_w) || !vec("norm2.bias", &L.ln2_b))
      return refused();
    {  // bounds on what enters this layer's split GEMMs (|LayerNorm(.)| <= sqrt(255) |gain| + |bias| per element)
      const float* Wi = T.find(p + "self_attn.in_proj_weight")->data;
      const float* bi = T.find(p + "self_attn.in_proj_bias")->data;
      const float* W1 = T.find(p + "linear1.weight")->data;
      const float* b1 = T.find(p + "linear1.bias")->data;
      auto ln_elem = [&](const char* wn, const char* bn) {
        return 16.f * max_abs(T.find(p + wn)->data, D) + max_abs(T.find(p + bn)->data, D);
      };
      act_bound = fmaxf(act_bound, x_norm);                                                                   // q/k/v input
      act_bound = fmaxf(act_bound, x_norm * max_row_norm(Wi, 2 * D, D) + max_abs(bi, 2 * D));              // q, k: operands of the split S = K Q^T
      act_bound = fmaxf(act_bound, x_norm * max_row_norm(Wi + (size_t)2 * D * D, D, D) + max_abs(bi + 2 * D, D));  // v (operand of P V) and out_proj input: convex combinations of v
      const float ln1 = ln_elem("norm1.weight", "norm1.bias");
      act_bound = fmaxf(act_bound, ln1);                                                                      // linear1 input (element bound)
      act_bound = fmaxf(act_bound, 16.f * ln1 * max_row_norm(W1, 2 * D, D) + max_abs(b1, 2 * D));          // linear2 input
      x_norm = 16.f * ln_elem("norm2.weight", "norm2.bias");                                                 // next layer's rows
    }
  }
  P.split_ok = (w_absmax < kSplitF16Safe && act_bound < kSplitF16Safe) ? 1 : 0;
  P.num_layers = cfg->num_layers;
  P.class_embed = cfg->class_embed;
  P.color_embed = cfg->color_embed;
  P.use_class = cfg->use_class;
  P.use_color = cfg->use_color;
  P.use_pos = cfg->use_position;
  P.use_num = cfg->use_num;
  P.nfeat = nfeat;
  ew->embed_dim = D;
  ew->object_size = object_size;
  ew->num_heads = cfg->num_heads;
  // everything is validated and staged: one allocation, one copy, then the old set goes and the new one is published
  if (const int rc = upload_staging(ctx, "t2l_load_weights", blob, &ew->blob)) return rc;
  free_weights(ctx);
  ctx->enc = ew.release();
  return T2L_OK;
}

int encode_impl(t2l_ctx* ctx, const t2l_packed_cells* in, float* out, hipStream_t s) {
  const EncParams& P = ctx->enc->p;
  if (P.use_class && !P.class_embed && !in->pn_feat)
    return fail(ctx, T2L_EINVAL, "t2l_encode_cells: pn_feat required when class_embed == 0");
  if ((P.use_class && P.class_embed && !in->class_idx) || (P.use_color && P.color_embed && !in->color_idx) ||
      (P.use_color && !P.color_embed && !in->rgb) || (P.use_pos && !in->center) || (P.use_num && !in->n_pts))
    return fail(ctx, T2L_EINVAL, "t2l_encode_cells: a per-object input required by the loaded config is NULL");
  // the published shape with split-f16 / plain-f16 arithmetic and at least two feature slots: two cells per eight-wave workgroup on
  // planes (option encoder_two_cells, default on); everything else: the one-cell kernel of encode_shaped.hip
  if (!(ctx->enc->published() && P.split_ok && !ctx->encoder_f32 && ctx->encoder_two_cells && P.nfeat > 1))
    return encode_shaped_impl(ctx, in, out, s);
  const size_t lds2 = (size_t)8 * kPlane * sizeof(_Float16) + (size_t)(2 * kSP * kLdH + 8) * sizeof(float);
  static PerDeviceOnce attr2;
  if (attr2.need(ctx->device)) {
    T2L_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&encode_cells2_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2));
    T2L_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&encode_cells2_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2));
    attr2.mark(ctx->device);
  }
  event_begin(ctx, "encode_cells", s);
  // encoder_f16 (option, off by default): ONE f16 product per operand pair instead of the three of the split form — embeddings
  // within ~1e-4 of the reference's (the north star asks for 1e-3) instead of 2e-7, 28 % less time
  if (ctx->encoder_f16)
    hipLaunchKernelGGL(encode_cells2_kernel<2>, dim3((in->n_cells + 1) / 2), dim3(512), lds2, s, P, *in, out);
  else
    hipLaunchKernelGGL(encode_cells2_kernel<1>, dim3((in->n_cells + 1) / 2), dim3(512), lds2, s, P, *in, out);
  event_end(ctx, "encode_cells", s);
  T2L_HIP(ctx, hipGetLastError());
  return T2L_OK;
}

}  // namespace t2l
