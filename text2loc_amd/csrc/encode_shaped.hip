// The one-cell cell encoder: ObjectEncoder.forward (models/object_encoder.py:66-153) + CellRetrievalNetwork.encode_objects
// (models/cell_retrieval.py:65-110), eval mode, as ONE kernel, one workgroup of four waves per cell, for every shape the reference
// builds from `args` (models/cell_retrieval.py:22-49, training/args.py:47,60-62) that is compiled:
//
//   coarse_embed_dim D in {128, 256};  head_dim HD in {32, 64} (object_inter_module_num_heads = D / HD);
//   object_size 1..32 (a run-time value);  1..4 layers;  dim_feedforward = 2 D.
//
// The published shape (256, 4 heads, 28 slots) is the <256, 64> instance with object_size = 28. encode_impl (encode.hip) puts the
// two-cell kernel in front of it when that one applies (split-f16 or plain-f16 arithmetic, two or more feature slots, option
// encoder_two_cells); its f32 arithmetic, single-feature models and encoder_two_cells = 0 run here.
//
// Every intermediate lives in LDS as f32 rows of D + 4 floats. Arithmetic, template value H:
//   1  the big contractions (feature merge, q/k/v, out_proj, both feed-forward products) as split-f16 on
//      v_mfma_f32_32x32x16_f16 (hi*hi + hi*lo + lo*hi, f32 accumulation; mfma_h3.h);
//   2  plain f16, one product per operand pair on the high halves of the same fragments (option encoder_f16; compiled for
//      <256, 64> and offered at the published shape only). The feature merge keeps its three products;
//   0  everything on the f32 MFMA: when the weights do not bound the activations below the f16 range (EncParams::split_ok) or
//      option encoder_f32 asks for it.
// The attention core and the small MLPs are f32 MFMA in all three.
//
// Tile ownership. A D-wide output is D / 32 column tiles; wave w owns tiles w, w + 4, ... (one at D = 128, two at 256, sharing
// the A fragments). A head is HD / 32 tiles of q, k and v; wave w runs heads w, w + 4, ... from registers only: q_h^T and k_h^T
// come out transposed (A = packed weights, B = token rows), so their registers are the A / B operands of S^T = K Q^T, whose
// k-extent is HD (one pass of 16 MFMAs per 32 features: head_dim 32 halves it); v_h comes out straight and its registers are
// the B operand of P V. At D = 128 with 64-wide heads there are two heads for four waves: two waves idle through the
// attention core (a quarter of the layer's FLOPs).
// The feed-forward hidden layer (2 D wide) goes through `buf` in two halves of D units: half hf = units [hf D/2, hf D/2 + D/2)
// and [D + hf D/2, ...), what k-steps [hf D/16, (hf + 1) D/16) of the half-split packing of linear2 (K = 2 D) cover.
//
// LDS: x [32][D + 4] + buf [32][D + 4] + 8 floats = 33.8 KB at D = 128, 66.6 KB at D = 256: two workgroups per CU at 256, so
// while one sits in a barrier, a LayerNorm or a softmax, the other keeps the MFMA pipe busy. The compiler does not see the
// dynamic LDS size: at D = 256 the kernel states its two waves per SIMD itself (amdgpu_waves_per_eu), or the register
// allocator squeezes the split-f16 instance into the 168 VGPRs of a third wave that never comes and serialises every weight
// fragment load with its use; there mm_tiles asks for a step's fragments one step ahead (profiles/shapes_encoder.md).
// Row stride D + 4: a lane (col, half) reads 16 bytes at col (D + 4) + const; over the 16 lanes of a ds_read_b128 group the
// word address is 4 col + const mod 64 for D a multiple of 64 (132 = 2*64 + 4, 260 = 4*64 + 4), sixteen disjoint runs of four
// banks: conflict-free at both widths. features2 (256 wide at every D) is staged over x AND buf (32 x 260 floats <=
// 2 x 32 x 132), so mlp_pointnet keeps its output in registers until every wave is done reading the stage.
//
// object_size: rows [nobj, object_size) are the reference's zero pad slots: attended to, attending, and in the max-pool (there
// is no padding mask). Rows [object_size, 32) are dead: masked out of the softmax keys and the max-pool. object_size = 32 has
// no dead row.
#include <math.h>

#include <string>

#include "t2l_internal.h"
#include "encode_shared.h"

#ifndef T2L_ENC_UNROLL
#define T2L_ENC_UNROLL 4
#endif

namespace t2l {
namespace {

constexpr int kLdStage = 256 + 4;  // features2 staging rows
constexpr int kLdHid = 64 + 4;     // hidden layer of the small MLPs

// acc[t] += X W_t^T (WA = false: this lane's LDS row half is the A operand) or W_t X^T (WA = true: the packed weight tile is the
// A operand, the product comes out transposed), over `khalf` k-values per lane half starting at per-half offset `koff` of a
// matrix packed for K = ktot. H = 0: f32 packing (pack_half_split) on v_mfma_f32_32x32x2_f32; 1: split-f16 fragments (pack_h), three
// products; 2: plain f16, the high halves of the same fragments, one product. AHEAD (the f16 forms at D = 256, where a SIMD
// holds two waves): the NT weight fragments of the next k-step are in flight behind the MFMAs of the current one. Not stream_weights
// (tile_blocks.h): one step ahead for NT tiles at once, the activation split on the fly, a partly unrolled loop — another schedule.
template <int H, bool WA, int NT, bool AHEAD = false>
__device__ __forceinline__ void mm_tiles(const float* __restrict__ arow, int khalf, const float4* __restrict__ wp,
                                         const uint4* __restrict__ hp, int ktot, int koff, const int (&tile)[NT],
                                         f32x16 (&acc)[NT], int lane) {
  if constexpr (H == 0) {
    const int qn = ktot >> 3, q0 = koff >> 2, nq = khalf >> 2;
    const float4* w[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) w[t] = wp + ((size_t)tile[t] * qn + q0) * 64 + lane;
#pragma unroll 4
    for (int q = 0; q < nq; ++q) {
      const float4 a = *reinterpret_cast<const float4*>(arow + 4 * q);
      float4 b[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) b[t] = w[t][q * 64];
#define T2L_SH_STEP(C)                                                                            \
  _Pragma("unroll") for (int t = 0; t < NT; ++t) acc[t] =                                         \
      WA ? __builtin_amdgcn_mfma_f32_32x32x2f32(b[t].C, a.C, acc[t], 0, 0, 0)                     \
         : __builtin_amdgcn_mfma_f32_32x32x2f32(a.C, b[t].C, acc[t], 0, 0, 0);
      T2L_SH_STEP(x) T2L_SH_STEP(y) T2L_SH_STEP(z) T2L_SH_STEP(w)
#undef T2L_SH_STEP
    }
  } else {
    const int steps = ktot >> 4, s0 = koff >> 3, ns = khalf >> 3;
    const uint4* w[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) w[t] = hp + (((size_t)tile[t] * steps + s0) * 64 + lane) * 2;
    if constexpr (AHEAD) {
      // the four-tile q/k pass unrolls half as far: at most eight fragments of 8 VGPRs named per body
      constexpr int kUnroll = NT > 2 ? (T2L_ENC_UNROLL > 1 ? T2L_ENC_UNROLL / 2 : 1) : T2L_ENC_UNROLL;
      HFrag b[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) b[t] = load_h1<H == 2>(w[t]);
#pragma unroll kUnroll
      for (int s = 0; s < ns; ++s) {
        const HFrag a = split_h<H == 2>(arow + 8 * s);
        // the next step's fragments are requested before this step's MFMAs (the last step asks for its own again); the
        // scheduling barrier keeps the compiler from sinking the loads to their uses, where each would wait vmcnt(0)
        const int sn = min(s + 1, ns - 1);
        HFrag nb[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) nb[t] = load_h1<H == 2>(w[t] + sn * 128);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          if constexpr (WA) mfma_h3<H == 2>(acc[t], b[t], a);
          else mfma_h3<H == 2>(acc[t], a, b[t]);
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) b[t] = nb[t];
      }
    } else {
#pragma unroll T2L_ENC_UNROLL
      for (int s = 0; s < ns; ++s) {
        const HFrag a = split_h<H == 2>(arow + 8 * s);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const HFrag b = load_h1<H == 2>(w[t] + s * 128);
          if constexpr (WA) mfma_h3<H == 2>(acc[t], b, a);
          else mfma_h3<H == 2>(acc[t], a, b);
        }
      }
    }
  }
}

template <int NT>
__device__ __forceinline__ void zero_tiles(f32x16 (&acc)[NT]) {
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
}

// F.normalize over the D columns of the 32 rows at buf (row stride ld); rows >= nvalid are zeroed. (D / 64 scalars per lane, the
// zeroing folded into the store; encode.hip's normalize_rows reads float4 at 256 only, fine.hip's f_normalize_rows zeroes nothing.)
template <int D>
__device__ __forceinline__ void normalize_rows_d(float* buf, int ld, int nvalid, int wave, int lane) {
  constexpr int EL = D / 64;
  for (int i = wave; i < kSP; i += 4) {
    float* p = buf + i * ld + lane * EL;
    float v[EL];
#pragma unroll
    for (int e = 0; e < EL; ++e) v[e] = p[e];
    float ss = v[0] * v[0];
#pragma unroll
    for (int e = 1; e < EL; ++e) ss += v[e] * v[e];
    ss = wave_sum(ss);
    const float inv = i < nvalid ? 1.f / fmaxf(sqrtf(ss), 1e-12f) : 0.f;
#pragma unroll
    for (int e = 0; e < EL; ++e) p[e] = i < nvalid ? v[e] * inv : 0.f;
  }
}

// torch.nn.LayerNorm(D, eps=1e-5) in place over the 32 rows of x
template <int D>
__device__ __forceinline__ void layer_norm_rows_d(float* x, const float* __restrict__ w, const float* __restrict__ b, int wave,
                                                  int lane) {
  constexpr int EL = D / 64, LD = D + 4;
  float wv[EL], bv[EL];
#pragma unroll
  for (int e = 0; e < EL; ++e) {
    wv[e] = w[lane * EL + e];
    bv[e] = b[lane * EL + e];
  }
  for (int i = wave; i < kSP; i += 4) {
    float* p = x + i * LD + lane * EL;
    float v[EL];
#pragma unroll
    for (int e = 0; e < EL; ++e) v[e] = p[e];
    float sum = v[0];
#pragma unroll
    for (int e = 1; e < EL; ++e) sum += v[e];
    const float mean = wave_sum(sum) * (1.f / D);
#pragma unroll
    for (int e = 0; e < EL; ++e) v[e] -= mean;
    float sq = v[0] * v[0];
#pragma unroll
    for (int e = 1; e < EL; ++e) sq += v[e] * v[e];
    const float var = wave_sum(sq) * (1.f / D);
    const float inv = 1.f / sqrtf(var + 1e-5f);
#pragma unroll
    for (int e = 0; e < EL; ++e) p[e] = v[e] * inv * wv[e] + bv[e];
  }
}

template <int D, int HD, int H>
__global__ __launch_bounds__(256, 2) __attribute__((amdgpu_waves_per_eu(2, D == 256 ? 2 : 4))) void encode_cells_shaped_kernel(
    EncParams P, t2l_packed_cells in, int object_size, float* __restrict__ out) {
  static_assert(D == 128 || D == 256, "tile ownership is written for 4 or 8 column tiles over four waves");
  static_assert(HD == 32 || HD == 64, "a head is one or two 32-column tiles");
  constexpr int LD = D + 4;       // row stride of x and buf (see the file header for the bank arithmetic)
  constexpr int NT = D / 128;     // column tiles of a D-wide output per wave
  constexpr int TPH = HD / 32;    // tiles per head
  constexpr int NH = D / HD;      // heads
  constexpr int KH = D / 2;       // k-values per lane half of a K = D product
  constexpr int DT = D / 32;      // tiles of a D-wide matrix
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* x = smem;               // [32][LD] token buffer; scratch (small-MLP hidden / features2 staging) before it is live
  float* buf = smem + kSP * LD;  // [32][LD] feature slot -> attention output -> feed-forward hidden half
  float* red = smem + 2 * kSP * LD;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 31, half = lane >> 5;
  const int cell = blockIdx.x;  // the grid is n_cells
  const int obj0 = in.offsets[cell];
  const int nobj = max(min(in.offsets[cell + 1] - obj0, object_size), 0);  // objects beyond object_size are dropped (cell_retrieval.py:94-98)
  int own[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) own[t] = wave + 4 * t;

  // ------------------------------------------------------------------ per-object features, merged slot by slot
  f32x16 keep[NT];
  zero_tiles(keep);
  int slot = 0;
  auto merge_slot = [&]() {  // buf holds slot `slot` (normalised rows): keep += buf @ Wmerge[:, D*slot : D*slot + D]^T
    __syncthreads();
    if (P.nfeat > 1) {  // (split-f16 also under plain f16)
      mm_tiles<(H ? 1 : 0), false, NT, D == 256>(buf + col * LD + half * KH, KH, P.merge_wp + (size_t)slot * (D * D / 4),
                               P.merge_hp + (size_t)slot * (D * D / 4), D, 0, own, keep, lane);
    } else {
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) keep[t][r] = buf[acc_row(r, half) * LD + own[t] * 32 + col];
    }
    ++slot;
    __syncthreads();  // every wave is done reading buf (and the x-region scratch) before the next slot rewrites them
  };
  auto table_rows = [&](const float* __restrict__ tab, const int* __restrict__ idx, int n_rows) {
    for (int e = tid; e < kSP * D; e += 256) {
      const int o = e / D, c = e % D;
      float v = 0.f;
      if (o < nobj) v = tab[(size_t)min(max(idx[obj0 + o], 0), n_rows - 1) * D + c];
      buf[o * LD + c] = v;
    }
  };
  // one feature branch through get_mlp([IN, 64, D]): hidden layer on the VALU, 64 -> D on the f32 MFMA
  auto small_mlp = [&](const SmallMlp& m, const float* __restrict__ src, int IN, bool is_num) {
    float* hbuf = x;
    for (int e = tid; e < kSP * 64; e += 256) {
      const int o = e >> 6, u = e & 63;
      float acc = 0.f;
      if (o < nobj) {
        acc = m.b1[u];
        for (int k = 0; k < IN; ++k) {
          float v = src[o * IN + k];
          if (is_num) v = (v - kNumMean) / kNumStd;  // object_encoder.py:143
          acc += m.w1[u * IN + k] * v;
        }
        acc = fmaxf(acc, 0.f);
      }
      hbuf[o * kLdHid + u] = acc;
    }
    __syncthreads();
    f32x16 acc[NT];
    zero_tiles(acc);
    mm_tiles<0, false, NT>(hbuf + col * kLdHid + half * 32, 32, m.w2p, nullptr, 64, 0, own, acc, lane);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int c = own[t] * 32 + col;
      const float b2 = m.b2[c];
#pragma unroll
      for (int r = 0; r < 16; ++r) buf[acc_row(r, half) * LD + c] = fmaxf(acc[t][r] + b2, 0.f);
    }
    __syncthreads();
    normalize_rows_d<D>(buf, LD, nobj, wave, lane);
  };

  if (P.use_class) {
    if (P.class_embed) {  // object_encoder.py:103-110 (table rows pre-normalised on the host)
      table_rows(P.class_tab, in.class_idx, P.n_class);
    } else {  // object_encoder.py:86-99,112: features2 [256] -> mlp_pointnet -> normalize
      float* stage = smem;  // 32 x 260 floats over x and (at D = 128) most of buf
      for (int o = wave; o < kSP; o += 4) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (o < nobj) v = reinterpret_cast<const float4*>(in.pn_feat + (size_t)(obj0 + o) * 256)[lane];
        reinterpret_cast<float4*>(stage + o * kLdStage)[lane] = v;
      }
      __syncthreads();
      f32x16 acc[NT];
      zero_tiles(acc);
      // (features2 is an input: its magnitude is not bounded by the weights, so this product stays f32)
      mm_tiles<0, false, NT>(stage + col * kLdStage + half * 128, 128, P.pn_wp, nullptr, 256, 0, own, acc, lane);
      __syncthreads();  // the stage overlaps buf
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int c = own[t] * 32 + col;
        const float pb = P.pn_b[c];
#pragma unroll
        for (int r = 0; r < 16; ++r) buf[acc_row(r, half) * LD + c] = fmaxf(acc[t][r] + pb, 0.f);
      }
      __syncthreads();
      normalize_rows_d<D>(buf, LD, nobj, wave, lane);
    }
    merge_slot();
  }
  if (P.use_color) {
    if (P.color_embed) table_rows(P.color_tab, in.color_idx, P.n_color);  // object_encoder.py:116-120
    else small_mlp(P.color, in.rgb + (size_t)obj0 * 3, 3, false);         // object_encoder.py:121-128
    merge_slot();
  }
  if (P.use_pos) {  // object_encoder.py:130-136
    small_mlp(P.pos, in.center + (size_t)obj0 * 3, 3, false);
    merge_slot();
  }
  if (P.use_num) {  // object_encoder.py:138-145
    small_mlp(P.num, in.n_pts + obj0, 1, true);
    merge_slot();
  }
  // merge epilogue (object_encoder.py:148-149: Linear+BN folded, ReLU) + normalize (cell_retrieval.py:92)
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int c = own[t] * 32 + col;
    const float mb = P.nfeat > 1 ? P.merge_b[c] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) x[acc_row(r, half) * LD + c] = P.nfeat > 1 ? fmaxf(keep[t][r] + mb, 0.f) : keep[t][r];
  }
  __syncthreads();
  normalize_rows_d<D>(x, LD, nobj, wave, lane);  // rows >= nobj: the zero pad slots (cell_retrieval.py:85) and the dead rows
  __syncthreads();

  // ------------------------------------------------------------------ set transformer (cell_retrieval.py:101-103)
  const float* xrow = x + col * LD + half * KH;
  for (int l = 0; l < P.num_layers; ++l) {
    const LayerW& W = P.layer[l];
    const float* ib = W.in_b;
    for (int h = wave; h < NH; h += 4) {  // registers only; no barrier inside (waves without a head skip the loop)
      f32x16 st;  // S^T, then the unnormalised probabilities
      float inv;
      {
        // q_h^T and k_h^T in one pass over x: tiles [q_0 .. q_TPH-1, k_0 .. k_TPH-1] share every token fragment
        int qk[2 * TPH];
        f32x16 qkT[2 * TPH];
#pragma unroll
        for (int t = 0; t < TPH; ++t) {
          qk[t] = h * TPH + t;
          qk[TPH + t] = DT + h * TPH + t;
        }
        zero_tiles(qkT);
        mm_tiles<H, true, 2 * TPH, D == 256>(xrow, KH, W.in_wp, W.in_hp, D, 0, qk, qkT, lane);
        // in_proj bias: q^T / k^T rows are features (register index)
#pragma unroll
        for (int t = 0; t < TPH; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int f = h * HD + t * 32 + acc_row(r, half);
            qkT[t][r] += ib[f];
            qkT[TPH + t][r] += ib[D + f];
          }
        // S^T[j][i] = k_j . q_i: k_h^T (token j = lane col, feature pair = the two lane halves) is the A operand, q_h^T the B
        // operand, one MFMA per register: 16 TPH MFMAs cover the HD features
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
        for (int t = 0; t < TPH; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) st = __builtin_amdgcn_mfma_f32_32x32x2f32(qkT[TPH + t][r], qkT[t][r], st, 0, 0, 0);
        // lane: query i = col, keys j = acc_row(r, half); keys >= object_size are the dead rows
        constexpr float scale = HD == 64 ? 0.125f : 0.17677669529663687f;  // 1/sqrt(head_dim)
        float m = -__builtin_inff();
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          st[r] = (acc_row(r, half) < object_size) ? st[r] * scale : -__builtin_inff();
          m = fmaxf(m, st[r]);
        }
        m = fmaxf(m, __shfl_xor(m, 32));  // key 0 is never masked (object_size >= 1): m is finite
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          st[r] = __expf(st[r] - m);
          sum += st[r];
        }
        sum += __shfl_xor(sum, 32);
        inv = 1.f / sum;
      }
      {  // v_h straight (A = token rows, B = packed weights), then o = P V from registers
        int vt[TPH];
        f32x16 v[TPH];
#pragma unroll
        for (int t = 0; t < TPH; ++t) vt[t] = 2 * DT + h * TPH + t;
        zero_tiles(v);
        mm_tiles<H, false, TPH, D == 256>(xrow, KH, W.in_wp, W.in_hp, D, 0, vt, v, lane);
#pragma unroll
        for (int t = 0; t < TPH; ++t) {
          const float bv = ib[2 * D + h * HD + t * 32 + col];  // v columns are features (lane)
          // o[i][n] = sum_j P[i][j] v[j][n]: P (lane = query i, register = key j) is the A operand, v_h registers (lane =
          // column n, register = key j) the B operand
          f32x16 o;
#pragma unroll
          for (int r = 0; r < 16; ++r) o[r] = 0.f;
#pragma unroll
          for (int r = 0; r < 16; ++r) o = __builtin_amdgcn_mfma_f32_32x32x2f32(st[r] * inv, v[t][r] + bv, o, 0, 0, 0);
#pragma unroll
          for (int r = 0; r < 16; ++r) buf[acc_row(r, half) * LD + h * HD + t * 32 + col] = o[r];
        }
      }
    }
    __syncthreads();
    {  // x = LN1(x + o @ out_proj^T + b)
      f32x16 acc[NT];
      zero_tiles(acc);
      mm_tiles<H, false, NT, D == 256>(buf + col * LD + half * KH, KH, W.out_wp, W.out_hp, D, 0, own, acc, lane);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int c = own[t] * 32 + col;
        const float b = W.out_b[c];
#pragma unroll
        for (int r = 0; r < 16; ++r) x[acc_row(r, half) * LD + c] += acc[t][r] + b;
      }
    }
    __syncthreads();
    layer_norm_rows_d<D>(x, W.ln1_w, W.ln1_b, wave, lane);
    __syncthreads();
    {  // x = LN2(x + relu(x W1^T + b1) W2^T + b2), hidden units in two halves through buf
      f32x16 acc[NT];
      zero_tiles(acc);
      for (int hf = 0; hf < 2; ++hf) {
        // buf column tile j of this half = hidden tile hf D/64 + j (j < D/64) or D/32 + hf D/64 + (j - D/64)
        int ht[NT];
        f32x16 hh[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) ht[t] = own[t] < DT / 2 ? hf * (DT / 2) + own[t] : DT + hf * (DT / 2) + own[t] - DT / 2;
        zero_tiles(hh);
        mm_tiles<H, false, NT, D == 256>(xrow, KH, W.ff1_wp, W.ff1_hp, D, 0, ht, hh, lane);
        if (hf) __syncthreads();  // every wave has consumed the first half from buf
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const float b1 = W.ff1_b[ht[t] * 32 + col];
#pragma unroll
          for (int r = 0; r < 16; ++r) buf[acc_row(r, half) * LD + own[t] * 32 + col] = fmaxf(hh[t][r] + b1, 0.f);
        }
        __syncthreads();
        mm_tiles<H, false, NT, D == 256>(buf + col * LD + half * KH, KH, W.ff2_wp, W.ff2_hp, 2 * D, hf * KH, own, acc, lane);
      }
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int c = own[t] * 32 + col;
        const float b2 = W.ff2_b[c];
#pragma unroll
        for (int r = 0; r < 16; ++r) x[acc_row(r, half) * LD + c] += acc[t][r] + b2;
      }
    }
    __syncthreads();
    layer_norm_rows_d<D>(x, W.ln2_w, W.ln2_b, wave, lane);
    __syncthreads();
  }

  // ------------------------------------------------------------------ max over ALL object_size slots, pads included (cell_retrieval.py:107-108)
  float mx = 0.f;
  if (tid < D) {
    mx = x[tid];
    for (int i = 1; i < object_size; ++i) mx = fmaxf(mx, x[i * LD + tid]);
  }
  const float ss = wave_sum(mx * mx);
  if (lane == 0) red[wave] = ss;
  __syncthreads();
  const float nrm = sqrtf(red[0] + red[1] + red[2] + red[3]);
  if (tid < D) out[(size_t)cell * D + tid] = mx / fmaxf(nrm, 1e-12f);
}

template <int D, int HD, int H>
int launch_shaped(t2l_ctx* ctx, const EncParams& P, const t2l_packed_cells* in, int object_size, float* out, hipStream_t s) {
  const size_t lds = (size_t)(2 * kSP * (D + 4) + 8) * sizeof(float);
  static PerDeviceOnce attr_done;
  if (attr_done.need(ctx->device)) {
    T2L_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&encode_cells_shaped_kernel<D, HD, H>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr_done.mark(ctx->device);
  }
  event_begin(ctx, "encode_cells", s);
  hipLaunchKernelGGL((encode_cells_shaped_kernel<D, HD, H>), dim3(in->n_cells), dim3(256), lds, s, P, *in, object_size, out);
  event_end(ctx, "encode_cells", s);
  T2L_HIP(ctx, hipGetLastError());
  return T2L_OK;
}

}  // namespace

bool shape_is_compiled(int embed_dim, int num_heads, int object_size) {
  if (embed_dim != 128 && embed_dim != 256) return false;
  if (num_heads <= 0 || embed_dim % num_heads) return false;
  const int hd = embed_dim / num_heads;
  return (hd == 32 || hd == 64) && object_size >= 1 && object_size <= kSP;
}

const char* compiled_shapes_text() {
  return "compiled shapes: coarse_embed_dim 128 or 256, head_dim 32 or 64 (num_heads 2 or 4 at 128, 4 or 8 at 256), object_size 1..32, "
         "1..4 layers";
}

int encode_shaped_impl(t2l_ctx* ctx, const t2l_packed_cells* in, float* out, hipStream_t s) {
  const EncoderWeights& ew = *ctx->enc;
  const EncParams& P = ew.p;
  // 0: everything on the f32 MFMA; 1: split-f16; 2: plain f16 (option encoder_f16: the published shape only, as encoder_two_cells)
  const int H = (!P.split_ok || ctx->encoder_f32) ? 0 : (ctx->encoder_f16 && ew.published()) ? 2 : 1;
  const int D = ew.embed_dim, hd = ew.embed_dim / ew.num_heads, S = ew.object_size;
  if (H == 2) return launch_shaped<256, 64, 2>(ctx, P, in, S, out, s);
#define T2L_SHAPED(DD, HH)                                                        \
  if (D == DD && hd == HH)                                                        \
    return H ? launch_shaped<DD, HH, 1>(ctx, P, in, S, out, s) : launch_shaped<DD, HH, 0>(ctx, P, in, S, out, s);
  T2L_SHAPED(128, 32)
  T2L_SHAPED(128, 64)
  T2L_SHAPED(256, 32)
  T2L_SHAPED(256, 64)
#undef T2L_SHAPED
  return fail(ctx, T2L_ESTATE, std::string("t2l_encode_cells: no kernel for the loaded shape (") + compiled_shapes_text() + ")");
}

}  // namespace t2l
