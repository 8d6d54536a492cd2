// Device kernels of the object-branch TRAINING step: forward in model.train() mode with saved
// activations, backward, Adam. gfx950 only. The row kernels (LayerNorm, F.normalize, element-wise dropout, max over a group's rows) also
// serve the fine step (fine_train.hip, through train.hip's launchers in train_common.h): row widths 128, 256 and 1024. All arithmetic is f32 (the reference trains in f32); contractions run on
// v_mfma_f32_32x32x2_f32. The step is small (B=64 cells -> 1,792 tokens, ~12 GFLOP fwd+bwd) and latency-bound, so the
// kernels are modular (one per op of the autograd graph) rather than fused per cell like the eval encoder.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "gemm_f32.h"
#include "train_common.h"

namespace t2l {
namespace train {

constexpr int kTD = 256;    // embed dim
constexpr int kTS = 28;     // object slots (tokens) per cell
constexpr int kTH = 4;      // heads
constexpr int kTHd = 64;    // head dim
constexpr float kBnEps = 1e-5f, kLnEps = 1e-5f, kNormEps = 1e-12f;

// all-reduce sum over the 64 lanes on the VALU (DPP + v_permlane swaps): __shfl_xor lowers to ds_bpermute_b32 — six dependent
// LDS round trips per sum
template <int CTRL>
__device__ __forceinline__ float wsum_dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float wsum(float v) {
  v += wsum_dpp<0xB1>(v);   // quad_perm [1,0,3,2]
  v += wsum_dpp<0x4E>(v);   // quad_perm [2,3,0,1]
  v += wsum_dpp<0x141>(v);  // row_half_mirror
  v += wsum_dpp<0x140>(v);  // row_mirror
  {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  }
  {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  }
  return v;
}

// A lane's share of a row, for the row kernels below (F.normalize, LayerNorm) at every width they serve — 128 (the fine step), 256 and
// 1024: VW = min(4, D / 64) consecutive floats of each 64 VW-column chunk, so float4 at `chunk * 256 + lane * 4` from D = 256 up and
// float2 at `lane * 2` at D = 128. vmap: f over the components of one or more vectors; vacc: s += a; vatomic_add: p[0 .. VW) += a with
// float atomics; vsum, vdot_pair: LayerNorm's pairwise lane sums; vdot: the sequential one of F.normalize; vdrop: the dropout rule on
// the VW elements from index o on. (Spelled so that the 256 and 1024 instances keep the code they had with float4 written out:
// profiles/fine_train_rows.md.)
template <int D>
struct RowVec {
  static_assert(D == 128 || (D >= 256 && D % 256 == 0), "row width: 128 or a multiple of 256");
  static constexpr int VW = D < 256 ? D / 64 : 4, CW = 64 * VW, NV = D / CW;
  using type = typename std::conditional<VW == 2, float2, float4>::type;
};
template <typename F, typename... R>
__device__ __forceinline__ float2 vmap(F f, float2 a, R... r) {
  return make_float2(f(a.x, r.x...), f(a.y, r.y...));
}
template <typename F, typename... R>
__device__ __forceinline__ float4 vmap(F f, float4 a, R... r) {
  return make_float4(f(a.x, r.x...), f(a.y, r.y...), f(a.z, r.z...), f(a.w, r.w...));
}
__device__ __forceinline__ void vacc(float2& s, float2 a) { s.x += a.x; s.y += a.y; }
__device__ __forceinline__ void vacc(float4& s, float4 a) { s.x += a.x; s.y += a.y; s.z += a.z; s.w += a.w; }
__device__ __forceinline__ void vatomic_add(float* p, float2 a) { unsafeAtomicAdd(p + 0, a.x); unsafeAtomicAdd(p + 1, a.y); }
__device__ __forceinline__ void vatomic_add(float* p, float4 a) {
  unsafeAtomicAdd(p + 0, a.x); unsafeAtomicAdd(p + 1, a.y); unsafeAtomicAdd(p + 2, a.z); unsafeAtomicAdd(p + 3, a.w);
}
__device__ __forceinline__ float vsum(float2 a) { return a.x + a.y; }
__device__ __forceinline__ float vsum(float4 a) { return (a.x + a.y) + (a.z + a.w); }
__device__ __forceinline__ float vdot_pair(float2 a, float2 b) { return a.x * b.x + a.y * b.y; }
__device__ __forceinline__ float vdot_pair(float4 a, float4 b) { return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w); }
__device__ __forceinline__ float vdot(float2 a, float2 b) { return a.x * b.x + a.y * b.y; }
__device__ __forceinline__ float vdot(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
__device__ __forceinline__ float drop1(float v, const Drop& dr, uint32_t i) { return keep_bit(dr.key, i, dr.thr) ? v * dr.scale : 0.f; }
__device__ __forceinline__ float2 vdrop(float2 v, const Drop& dr, uint32_t o) { return make_float2(drop1(v.x, dr, o), drop1(v.y, dr, o + 1)); }
__device__ __forceinline__ float4 vdrop(float4 v, const Drop& dr, uint32_t o) {
  return make_float4(drop1(v.x, dr, o), drop1(v.y, dr, o + 1), drop1(v.z, dr, o + 2), drop1(v.w, dr, o + 3));
}

// ---------------------------------------------------------------------------------------------------------------
// first Linear of the small branches (K = 1 or 3 inputs -> 64): y[m][c] = b[c] + sum_k x[m][k] w[c][k]
// standardize: x = (n_pts - mean)/std evaluated in f32 exactly as the reference's tensor expression
// (models/object_encoder.py:141-144).
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float small_in(const float* x, int m, int K, int k, int standardize, float mean, float stdv) {
  float v = x[(size_t)m * K + k];
  return standardize ? (v - mean) / stdv : v;
}
// Every op of the feature branches is ONE kernel over a job list (<= kMaxJobs jobs, the job in an extra grid dimension): the two or three
// small branches — position, point count, colour — are independent chains of identical shape, so each stage of all of them is one
// launch (a dependent launch costs ~5 us whatever it does); a layer that is alone (mlp_merge, mlp_pointnet) is a list of one.
constexpr int kMaxJobs = 3;
__device__ __forceinline__ void smallk_fwd_body(const float* __restrict__ x, int M, int K, const float* __restrict__ w,
                                                const float* __restrict__ b, int standardize, float mean, float stdv,
                                                float* __restrict__ y, unsigned bx) {
  const int i = bx * blockDim.x + threadIdx.x;
  if (i >= M * 64) return;
  const int m = i >> 6, c = i & 63;
  float s = b[c];
  for (int k = 0; k < K; ++k) s += small_in(x, m, K, k, standardize, mean, stdv) * w[c * K + k];
  y[i] = s;
}
struct SmallkJob {
  const float* x;
  int K, standardize;
  const float *w, *b;   // forward
  float* y;             // forward
  const float* dy;      // backward
  float *dW, *db;       // backward
};
struct SmallkMulti {
  SmallkJob j[kMaxJobs];
  int M, rows_per_block;
  float mean, stdv;
};
__global__ void smallk_fwd_kernel(SmallkMulti m) {
  const SmallkJob& j = m.j[blockIdx.y];
  smallk_fwd_body(j.x, m.M, j.K, j.w, j.b, j.standardize, m.mean, m.stdv, j.y, blockIdx.x);
}
// dW[c][k] += sum_m dy[m][c] x[m][k]   grid = row chunks, 256 threads = 64 channels x 4 row lanes
__device__ __forceinline__ void smallk_bwd_body(const float* __restrict__ x, int M, int K, const float* __restrict__ dy, int standardize,
                                                float mean, float stdv, int rows_per_block, float* __restrict__ dW,
                                                float* __restrict__ db, unsigned bx) {
  __shared__ float red[4][256];
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int lo = bx * rows_per_block, hi = min(M, lo + rows_per_block);
  float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
  for (int m = lo + g; m < hi; m += 4) {
    const float d = dy[(size_t)m * 64 + c];
    s[3] += d;
    for (int k = 0; k < K; ++k) s[k] += d * small_in(x, m, K, k, standardize, mean, stdv);
  }
  for (int k = 0; k < 4; ++k) red[k][threadIdx.x] = s[k];
  __syncthreads();
  if (g == 0) {
    for (int k = 0; k < K; ++k)
      unsafeAtomicAdd(dW + c * K + k, red[k][c] + red[k][c + 64] + red[k][c + 128] + red[k][c + 192]);
    unsafeAtomicAdd(db + c, red[3][c] + red[3][c + 64] + red[3][c + 128] + red[3][c + 192]);
  }
}
__global__ __launch_bounds__(256) void smallk_bwd_kernel(SmallkMulti m) {
  const SmallkJob& j = m.j[blockIdx.y];
  smallk_bwd_body(j.x, m.M, j.K, j.dy, j.standardize, m.mean, m.stdv, m.rows_per_block, j.dW, j.db, blockIdx.x);
}

// ---------------------------------------------------------------------------------------------------------------
// BatchNorm1d in training mode (+ ReLU). Two stages so that the whole chip takes part although there are only 64-1024
// channels: (1) per (64 channels x 64 rows) workgroup partial sums, float64 atomics into acc[2*C]; (2) elementwise apply.
// var = E[x^2] - mean^2 in float64 (inputs are f32; the cancellation is harmless there). Running statistics get the
// unbiased variance (momentum 0.1), as torch does.
// ---------------------------------------------------------------------------------------------------------------
constexpr int kBnRows = 64;
// (the accumulator slot's layout, kBnCount / kBnStride: train_common.h)
// MODE 0: acc[c] += sum y, acc[C+c] += sum y^2.  MODE 1: dv = out>0 ? d : 0; acc[c] += sum dv, acc[C+c] += sum dv*xhat
template <int MODE>
__device__ __forceinline__ void bn_stats_body(const float* __restrict__ y, const float* __restrict__ d, const float* __restrict__ out, int M,
                                              int C, const float* __restrict__ save_mean, const float* __restrict__ save_rstd,
                                              double* __restrict__ acc, unsigned bx, unsigned by, int sync,
                                              float* __restrict__ dgamma, float* __restrict__ dbeta) {
  __shared__ float r1[256], r2[256];
  const int c = bx * 64 + (threadIdx.x & 63), g = threadIdx.x >> 6;
  const int lo = by * kBnRows, hi = min(M, lo + kBnRows);
  float mean = 0.f, rstd = 0.f;
  if (MODE == 1) {
    mean = save_mean[c];
    rstd = save_rstd[c];
  }
  float s1 = 0.f, s2 = 0.f;
#pragma unroll 8  // 16 rows per thread: the loads of eight of them in flight (each row's loads otherwise wait for the previous row's)
  for (int m = lo + g; m < hi; m += 4) {
    const size_t i = (size_t)m * C + c;
    if (MODE == 0) {
      const float v = y[i];
      s1 += v;
      s2 += v * v;
    } else {
      const float dv = out[i] > 0.f ? d[i] : 0.f;
      s1 += dv;
      s2 += dv * (y[i] - mean) * rstd;
    }
  }
  r1[threadIdx.x] = s1;
  r2[threadIdx.x] = s2;
  __syncthreads();
  if (g == 0) {
    const int t = threadIdx.x;
    const double t1 = (double)r1[t] + (double)r1[t + 64] + (double)r1[t + 128] + (double)r1[t + 192];
    const double t2 = (double)r2[t] + (double)r2[t + 64] + (double)r2[t + 128] + (double)r2[t + 192];
    atomicAdd(acc + c, t1);
    atomicAdd(acc + C + c, t2);
    if (sync) {
      // cross-rank statistics: the slot will hold GLOBAL sums when the apply launch reads it, and the parameter gradients are this
      // rank's own sums (the gradient all_reduce adds the ranks' up) — so they are taken here, not in the apply launch
      if (MODE == 1) {
        unsafeAtomicAdd(dgamma + c, (float)t2);
        unsafeAtomicAdd(dbeta + c, (float)t1);
      }
      if (bx == 0 && by == 0 && t == 0) atomicAdd(acc + kBnCount, (double)M);
    }
  }
}
// one BatchNorm layer of one branch: everything the statistics / apply kernels of either direction need
struct BnJob {
  const float* y;       // pre-BatchNorm Linear output
  float* out;           // forward: post-ReLU output (written); backward: the same (read: ReLU mask)
  float* d;             // backward: gradient w.r.t. out, overwritten with the gradient w.r.t. y
  double* acc;
  const float *gamma, *beta;
  float *run_mean, *run_var, *save_mean, *save_rstd, *dgamma, *dbeta;
};
struct BnMulti {
  BnJob j[kMaxJobs];
  int M, C;
  float momentum;
  int sync;
};
template <int MODE>
__global__ __launch_bounds__(256) void bn_stats_kernel(BnMulti m) {
  const BnJob& j = m.j[blockIdx.z];
  bn_stats_body<MODE>(j.y, j.d, j.out, m.M, m.C, j.save_mean, j.save_rstd, j.acc, blockIdx.x, blockIdx.y, m.sync, j.dgamma, j.dbeta);
}
__device__ __forceinline__ void bn_apply_fwd_body(const float* __restrict__ y, int M, int C, const double* __restrict__ acc,
                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                  float* __restrict__ run_mean, float* __restrict__ run_var, float momentum,
                                                  float* __restrict__ out, float* __restrict__ save_mean, float* __restrict__ save_rstd,
                                                  unsigned bx, int sync) {
  const size_t i = (size_t)bx * 256 + threadIdx.x;
  const double Mg = sync ? acc[kBnCount] : (double)M;  // rows behind the sums: this rank's, or every rank's
  if (i < (size_t)M * C) {
    const int c = (int)(i % C);
    const double mean = acc[c] / Mg;
    const double var = fmax(acc[C + c] / Mg - mean * mean, 0.0);
    const float rstd = 1.0f / sqrtf((float)var + kBnEps);
    out[i] = fmaxf((y[i] - (float)mean) * rstd * gamma[c] + beta[c], 0.f);
  }
  if (bx == 0)
    for (int c = threadIdx.x; c < C; c += 256) {
      const double mean = acc[c] / Mg;
      const double var = fmax(acc[C + c] / Mg - mean * mean, 0.0);
      save_mean[c] = (float)mean;
      save_rstd[c] = 1.0f / sqrtf((float)var + kBnEps);
      run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * (float)mean;
      run_var[c] = (1.f - momentum) * run_var[c] + momentum * (float)(var * (Mg / fmax(Mg - 1.0, 1.0)));
    }
}
__global__ __launch_bounds__(256) void bn_apply_fwd_kernel(BnMulti m) {
  const BnJob& j = m.j[blockIdx.y];
  bn_apply_fwd_body(j.y, m.M, m.C, j.acc, j.gamma, j.beta, j.run_mean, j.run_var, m.momentum, j.out, j.save_mean, j.save_rstd, blockIdx.x, m.sync);
}
// d: gradient w.r.t. the ReLU output (in), overwritten with the gradient w.r.t. the Linear output y.
__device__ __forceinline__ void bn_apply_bwd_body(float* __restrict__ d, const float* __restrict__ out, const float* __restrict__ y, int M,
                                                  int C, const double* __restrict__ acc, const float* __restrict__ gamma,
                                                  const float* __restrict__ save_mean, const float* __restrict__ save_rstd,
                                                  float* __restrict__ dgamma, float* __restrict__ dbeta, unsigned bx, int sync) {
  const size_t i = (size_t)bx * 256 + threadIdx.x;
  if (i < (size_t)M * C) {
    const int c = (int)(i % C);
    const float Mg = sync ? (float)acc[kBnCount] : (float)M;
    const float rstd = save_rstd[c], s1 = (float)acc[c], s2 = (float)acc[C + c];
    const float dv = out[i] > 0.f ? d[i] : 0.f;
    d[i] = gamma[c] * rstd / Mg * (Mg * dv - s1 - (y[i] - save_mean[c]) * rstd * s2);
  }
  if (bx == 0 && !sync)  // (sync: the statistics launch took this rank's own sums)
    for (int c = threadIdx.x; c < C; c += 256) {
      unsafeAtomicAdd(dgamma + c, (float)acc[C + c]);
      unsafeAtomicAdd(dbeta + c, (float)acc[c]);
    }
}
__global__ __launch_bounds__(256) void bn_apply_bwd_kernel(BnMulti m) {
  const BnJob& j = m.j[blockIdx.y];
  bn_apply_bwd_body(j.d, j.out, j.y, m.M, m.C, j.acc, j.gamma, j.save_mean, j.save_rstd, j.dgamma, j.dbeta, blockIdx.x, m.sync);
}

// ---------------------------------------------------------------------------------------------------------------
// F.normalize over D-wide rows (D = 256: the coarse step, 128: the fine step): one wave per row, D / 64 floats per lane.
// ---------------------------------------------------------------------------------------------------------------
template <typename V>
__device__ __forceinline__ V norm_fwd(V v, float& n) {
  n = fmaxf(sqrtf(wsum(vdot(v, v))), kNormEps);
  const float nn = n;
  return vmap([nn](float a) { return a / nn; }, v);
}
template <typename V>
__device__ __forceinline__ V norm_bwd(V dy, V y, float n) {
  if (n <= kNormEps) return vmap([](float d) { return d / kNormEps; }, dy);
  const float t = wsum(vdot(dy, y));
  return vmap([t, n](float d, float yy) { return (d - yy * t) / n; }, dy, y);
}
// src row = table[idx[m]] when idx != nullptr (embedding lookup: the coarse step's, the index is not tested) else src[m]; dst row stride
// ldd (a D-wide slot of cat)
template <int D>
__device__ __forceinline__ void rownorm_fwd_body(const float* __restrict__ src, const int32_t* __restrict__ idx, int M, float* __restrict__ dst,
                                                 int ldd, float* __restrict__ save_n, unsigned bx) {
  using V = typename RowVec<D>::type;
  constexpr int VW = RowVec<D>::VW;
  const int m = (bx * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (m >= M) return;
  const size_t row = idx ? (size_t)idx[m] : (size_t)m;
  const V v = *reinterpret_cast<const V*>(src + row * D + lane * VW);
  float n;
  const V y = norm_fwd(v, n);
  *reinterpret_cast<V*>(dst + (size_t)m * ldd + lane * VW) = y;
  if (lane == 0) save_n[m] = n;
}
struct RownormJob {
  const float* src;      // forward: rows to normalise (or the embedding table); backward: dy (a slot of dcat)
  const int32_t* idx;    // forward: embedding lookup or nullptr
  float* dst;            // forward: slot of cat; backward: dx [M][D]
  const float* y;        // backward: the normalised rows (slot of cat)
  float* save_n;
};
struct RownormMulti {
  RownormJob j[kMaxJobs];
  int M, ld;
};
template <int D>
__global__ void rownorm_fwd_kernel(RownormMulti m) {
  const RownormJob& j = m.j[blockIdx.y];
  rownorm_fwd_body<D>(j.src, j.idx, m.M, j.dst, m.ld, j.save_n, blockIdx.x);
}
// dx[m] = normalize_bwd(dy[m], y[m], n[m])
template <int D>
__device__ __forceinline__ void rownorm_bwd_body(const float* __restrict__ dy, const float* __restrict__ y, int ld,
                                                 const float* __restrict__ save_n, int M, float* __restrict__ dx, unsigned bx) {
  using V = typename RowVec<D>::type;
  constexpr int VW = RowVec<D>::VW;
  const int m = (bx * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (m >= M) return;
  const V d = *reinterpret_cast<const V*>(dy + (size_t)m * ld + lane * VW);
  const V yy = *reinterpret_cast<const V*>(y + (size_t)m * ld + lane * VW);
  *reinterpret_cast<V*>(dx + (size_t)m * D + lane * VW) = norm_bwd(d, yy, save_n[m]);
}
template <int D>
__global__ void rownorm_bwd_kernel(RownormMulti m) {
  const RownormJob& j = m.j[blockIdx.y];
  rownorm_bwd_body<D>(j.src, j.y, m.ld, j.save_n, m.M, j.dst, blockIdx.x);
}
// Embedding-table gradient, stage 2 (stage 1 = rownorm_bwd_kernel writing g[M,256] = normalize_bwd per object):
// dtable[r] += sum over the objects with idx == r of g[m]. grid (table rows - 1, kEmbSplit): row 0 = padding_idx never
// receives gradient (models/object_encoder.py:33,37). Each workgroup lists in LDS the matching objects with
// m % kEmbSplit == blockIdx.y, its 4 waves add their rows (independent coalesced 1 KiB loads), then 256 float atomics.
constexpr int kEmbSplit = 8;
__device__ __forceinline__ void embed_sum_body(const float* __restrict__ g, const int32_t* __restrict__ idx, int M, float* __restrict__ dtable,
                                               unsigned bx, unsigned by) {
  __shared__ float4 red[256];
  __shared__ int list[2048];
  __shared__ int cnt;
  const int r = bx + 1, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int base = 0; base < M; base += 2048) {
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    for (int m = base + threadIdx.x; m < min(M, base + 2048); m += 256)
      if (idx[m] == r && (m % kEmbSplit) == (int)by) list[atomicAdd(&cnt, 1)] = m;  // this workgroup's share
    __syncthreads();
    const int n = cnt;
#pragma unroll 4
    for (int i = w; i < n; i += 4) {
      const float4 v = *reinterpret_cast<const float4*>(g + (size_t)list[i] * kTD + lane * 4);
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
    __syncthreads();
  }
  red[threadIdx.x] = a;
  __syncthreads();
  if (w == 0) {
    for (int i = 1; i < 4; ++i) {
      const float4 b = red[lane + 64 * i];
      a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    float* t = dtable + (size_t)r * kTD + lane * 4;
    unsafeAtomicAdd(t + 0, a.x); unsafeAtomicAdd(t + 1, a.y); unsafeAtomicAdd(t + 2, a.z); unsafeAtomicAdd(t + 3, a.w);
  }
}
struct EmbedSumMulti {
  const float* g[kMaxJobs];
  const int32_t* idx[kMaxJobs];
  float* dtable[kMaxJobs];
  int rows[kMaxJobs];  // table rows (row 0 = padding_idx receives nothing); grid.x = max(rows) - 1
  int M;
};
__global__ __launch_bounds__(256) void embed_sum_kernel(EmbedSumMulti m) {
  const int j = blockIdx.z;
  if ((int)blockIdx.x + 1 >= m.rows[j]) return;  // (workgroup-uniform: the barriers inside are not reached by anyone)
  embed_sum_body(m.g[j], m.idx[j], m.M, m.dtable[j], blockIdx.x, blockIdx.y);
}
// tokens: X0[b*28+s] = normalize(feats[offsets[b]+s]) for s < min(count,28), zeros otherwise (cell_retrieval.py:85-98)
__global__ void scatter_norm_fwd_kernel(const float* __restrict__ feats, const int32_t* __restrict__ offsets, int B,
                                        float* __restrict__ X0, float* __restrict__ save_n) {
  const int t = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (t >= B * kTS) return;
  const int b = t / kTS, s = t - b * kTS;
  const int lo = offsets[b], cnt = offsets[b + 1] - lo;
  float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
  if (s < cnt) {
    float n;
    y = norm_fwd(*reinterpret_cast<const float4*>(feats + (size_t)(lo + s) * kTD + lane * 4), n);
    if (lane == 0) save_n[lo + s] = n;
  }
  *reinterpret_cast<float4*>(X0 + (size_t)t * kTD + lane * 4) = y;
}
// dfeats[o] = normalize_bwd(dX0[token of o]) for the kept objects, 0 for objects beyond slot 27
__global__ void scatter_norm_bwd_kernel(const float* __restrict__ dX0, const float* __restrict__ X0,
                                        const float* __restrict__ save_n, const int32_t* __restrict__ offsets, int B,
                                        int M, float* __restrict__ dfeats) {
  const int o = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (o >= M) return;
  int lo = 0, hi = B;  // largest b with offsets[b] <= o
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offsets[mid] <= o) lo = mid; else hi = mid;
  }
  const int s = o - offsets[lo];
  float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
  if (s < kTS) {
    const size_t t = (size_t)lo * kTS + s;
    g = norm_bwd(*reinterpret_cast<const float4*>(dX0 + t * kTD + lane * 4),
                 *reinterpret_cast<const float4*>(X0 + t * kTD + lane * 4), save_n[o]);
  }
  *reinterpret_cast<float4*>(dfeats + (size_t)o * kTD + lane * 4) = g;
}

// ---------------------------------------------------------------------------------------------------------------
// The kernels of one nn.TransformerEncoderLayer, for every caller (train.hip: enc_layer_fwd / enc_layer_bwd): the object branch's
// obj_inter_module.* (D 256, 28 slots per cell) and the text head's intra_module.0 (D 1024 over L <= 32 tokens per sentence) and
// inter_module.0 (D 256 over S <= 32 sentences per description; models/language_encoder.py:97-101,127-147).
// ---------------------------------------------------------------------------------------------------------------
// self-attention over the S rows of one group (cell / sentence / description), one workgroup per (group, head); qkv [rows][3 D],
// D = 4 HD. No padding mask (cell_retrieval.py:102). Dynamic LDS (train.hip: attn_lds): q, k, v tiles [S][HD + 1] + p [S][S + 1]
// (forward), + go and two more [S][S + 1] (backward).
// CS: S at compile time, 0 = the run-time argument. The object branch instantiates its 28 (every trip count known: its step is
// latency-bound, and with S at run time its forward and backward measured 4-5 % slower, profiles/train_layer.md); same arithmetic.
template <int HD, int CS>
__global__ __launch_bounds__(256) void attn_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ P, float* __restrict__ O,
                                                       int S_rt, Drop dr) {
  extern __shared__ float sm[];
  constexpr int AS = HD + 1, D = 4 * HD;
  // (S known: the tile's load loop unrolled whole, every global load issued before the first LDS write waits for one)
  constexpr int kLoadTrips = CS ? (CS * HD + 255) / 256 : 1;
  const int S = CS ? CS : S_rt;
  float *q = sm, *k = q + S * AS, *v = k + S * AS, *p = v + S * AS;
  const int b = blockIdx.x >> 2, h = blockIdx.x & 3, tid = threadIdx.x, SP = S + 1;
  const float scale = 1.0f / sqrtf((float)HD);
#pragma unroll kLoadTrips
  for (int i = tid; i < S * HD; i += 256) {
    const int s = i / HD, d = i - s * HD;
    const float* base = qkv + (size_t)(b * S + s) * (3 * D) + h * HD + d;
    q[s * AS + d] = base[0];
    k[s * AS + d] = base[D];
    v[s * AS + d] = base[2 * D];
  }
  __syncthreads();
  for (int e = tid; e < S * S; e += 256) {
    const int i = e / S, j = e - i * S;
    float s = 0.f;
#pragma unroll 8
    for (int d = 0; d < HD; ++d) s += q[i * AS + d] * k[j * AS + d];
    p[i * SP + j] = s * scale;
  }
  __syncthreads();
  if (tid < S) {
    float* row = p + tid * SP;
    float mx = row[0];
    for (int j = 1; j < S; ++j) mx = fmaxf(mx, row[j]);
    float sum = 0.f;
    for (int j = 0; j < S; ++j) {
      row[j] = expf(row[j] - mx);
      sum += row[j];
    }
    for (int j = 0; j < S; ++j) row[j] /= sum;
  }
  __syncthreads();
  const size_t pbase = (size_t)blockIdx.x * S * S;
  for (int e = tid; e < S * S; e += 256) {
    const int i = e / S, j = e - i * S;
    float pv = p[i * SP + j];
    P[pbase + e] = pv;  // probabilities BEFORE dropout (softmax backward needs them)
    if (dr.thr) pv = keep_bit(dr.key, (uint32_t)(pbase + e), dr.thr) ? pv * dr.scale : 0.f;
    p[i * SP + j] = pv;
  }
  __syncthreads();
  for (int e = tid; e < S * HD; e += 256) {
    const int i = e / HD, d = e - i * HD;
    float s = 0.f;
    for (int j = 0; j < S; ++j) s += p[i * SP + j] * v[j * AS + d];
    O[(size_t)(b * S + i) * D + h * HD + d] = s;
  }
}
template <int HD, int CS>
__global__ __launch_bounds__(256) void attn_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ P,
                                                       const float* __restrict__ dO, float* __restrict__ dqkv, int S_rt, Drop dr) {
  extern __shared__ float sm[];
  constexpr int AS = HD + 1, D = 4 * HD;
  // (S known: the tile's load loop unrolled whole, every global load issued before the first LDS write waits for one)
  constexpr int kLoadTrips = CS ? (CS * HD + 255) / 256 : 1;
  const int S = CS ? CS : S_rt;
  const int SP = S + 1;
  float *q = sm, *k = q + S * AS, *v = k + S * AS, *go = v + S * AS, *p = go + S * AS, *pd = p + S * SP, *ds = pd + S * SP;
  const int b = blockIdx.x >> 2, h = blockIdx.x & 3, tid = threadIdx.x;
  const float scale = 1.0f / sqrtf((float)HD);
#pragma unroll kLoadTrips
  for (int i = tid; i < S * HD; i += 256) {
    const int s = i / HD, d = i - s * HD;
    const float* base = qkv + (size_t)(b * S + s) * (3 * D) + h * HD + d;
    q[s * AS + d] = base[0];
    k[s * AS + d] = base[D];
    v[s * AS + d] = base[2 * D];
    go[s * AS + d] = dO[(size_t)(b * S + s) * D + h * HD + d];
  }
  const size_t pbase = (size_t)blockIdx.x * S * S;
  for (int e = tid; e < S * S; e += 256) {
    const int i = e / S, j = e - i * S;
    const float pv = P[pbase + e];
    const float m = dr.thr ? (keep_bit(dr.key, (uint32_t)(pbase + e), dr.thr) ? dr.scale : 0.f) : 1.f;
    p[i * SP + j] = pv;
    pd[i * SP + j] = pv * m;
    ds[i * SP + j] = m;  // mask factor for now
  }
  __syncthreads();
  for (int e = tid; e < S * HD; e += 256) {  // dV[j][d] = sum_i Pd[i][j] dO[i][d]
    const int j = e / HD, d = e - j * HD;
    float s = 0.f;
    for (int i = 0; i < S; ++i) s += pd[i * SP + j] * go[i * AS + d];
    dqkv[(size_t)(b * S + j) * (3 * D) + 2 * D + h * HD + d] = s;
  }
  for (int e = tid; e < S * S; e += 256) {  // dP[i][j] = mask * sum_d dO[i][d] V[j][d]
    const int i = e / S, j = e - i * S;
    float s = 0.f;
#pragma unroll 8
    for (int d = 0; d < HD; ++d) s += go[i * AS + d] * v[j * AS + d];
    ds[i * SP + j] *= s;
  }
  __syncthreads();
  if (tid < S) {  // dS = P * (dP - sum_j dP*P) / sqrt(hd)
    float t = 0.f;
    for (int j = 0; j < S; ++j) t += ds[tid * SP + j] * p[tid * SP + j];
    for (int j = 0; j < S; ++j) ds[tid * SP + j] = p[tid * SP + j] * (ds[tid * SP + j] - t) * scale;
  }
  __syncthreads();
  for (int e = tid; e < S * HD; e += 256) {
    const int i = e / HD, d = e - i * HD;
    float sq = 0.f, sk = 0.f;
    for (int j = 0; j < S; ++j) {
      sq += ds[i * SP + j] * k[j * AS + d];
      sk += ds[j * SP + i] * q[j * AS + d];
    }
    float* base = dqkv + (size_t)(b * S + i) * (3 * D) + h * HD + d;
    base[0] = sq;
    base[D] = sk;
  }
}

// out = LayerNorm(x + dropout(y)) over D columns (128, 256, 1024), one wave per row (RowVec<D>: D / 256 float4 per lane, each wave-load
// 1 KiB contiguous; one float2 at D = 128). Saves xhat and rstd.
template <int D>
__global__ void ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, int T, const float* __restrict__ gamma,
                              const float* __restrict__ beta, Drop dr, float* __restrict__ out, float* __restrict__ xhat,
                              float* __restrict__ save_rstd) {
  using V = typename RowVec<D>::type;
  constexpr int VW = RowVec<D>::VW, CW = RowVec<D>::CW, NV = RowVec<D>::NV;
  const int t = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (t >= T) return;
  V a[NV];
  float s1 = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const size_t o = (size_t)t * D + j * CW + lane * VW;
    a[j] = *reinterpret_cast<const V*>(x + o);
    V f = *reinterpret_cast<const V*>(y + o);
    if (dr.thr) f = vdrop(f, dr, (uint32_t)o);
    vacc(a[j], f);
    s1 += vsum(a[j]);
  }
  const float mu = wsum(s1) * (1.f / D);
  float s2 = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    a[j] = vmap([mu](float p) { return p - mu; }, a[j]);
    s2 += vdot_pair(a[j], a[j]);
  }
  const float rstd = 1.0f / sqrtf(wsum(s2) * (1.f / D) + kLnEps);
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const size_t o = (size_t)t * D + j * CW + lane * VW;
    const V h = vmap([rstd](float p) { return p * rstd; }, a[j]);
    const V g = *reinterpret_cast<const V*>(gamma + j * CW + lane * VW);
    const V be = *reinterpret_cast<const V*>(beta + j * CW + lane * VW);
    *reinterpret_cast<V*>(xhat + o) = h;
    *reinterpret_cast<V*>(out + o) = vmap([](float p, float q, float r) { return p * q + r; }, h, g, be);
  }
  if (lane == 0) save_rstd[t] = rstd;
}
// dz = LN backward of dout; d_res = dz (gradient of the residual input), d_y = dz * dropout mask (gradient of y).
// dgamma/dbeta: per-workgroup column partials, then atomics. grid = any; each of a workgroup's WAVES waves strides over rows.
// The dgamma / dbeta atomics of a workgroup land on the same 2 D addresses as everybody else's (~75 ns per same-address atomic: at
// D = 256, 64 workgroups of 4 waves spent ~5 of their 10.7 us there, 128 workgroups took 15.5 us), so the object branch spreads its
// rows over MORE WAVES per workgroup (16) instead of more workgroups. The partials take WAVES * D * 8 bytes of LDS: 4 waves at D = 1024.
template <int D, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void ln_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ xhat,
                                                            const float* __restrict__ save_rstd, int T, const float* __restrict__ gamma,
                                                            Drop dr, float* __restrict__ d_res, float* __restrict__ d_y,
                                                            float* __restrict__ dgamma, float* __restrict__ dbeta) {
  using V = typename RowVec<D>::type;
  constexpr int VW = RowVec<D>::VW, CW = RowVec<D>::CW, NV = RowVec<D>::NV;
  __shared__ V rg[WAVES * 64 * NV], rb[WAVES * 64 * NV];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  V g[NV], ag[NV], ab[NV], d[NV], h[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    g[j] = *reinterpret_cast<const V*>(gamma + j * CW + lane * VW);
    ag[j] = ab[j] = d[j] = h[j] = V{};
  }
  // a wave walks several rows: the next row's operands are loaded before the current row is reduced and stored (written as
  // load -> reduce -> store per row, every row paid its own L2 round trip behind the previous row's stores: 11.4 us per launch
  // at the object branch's shape)
  const int stride = gridDim.x * WAVES;
  int t = blockIdx.x * WAVES + w;
  float rstd = 0.f;
  if (t < T) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const size_t o = (size_t)t * D + j * CW + lane * VW;
      d[j] = *reinterpret_cast<const V*>(dout + o);
      h[j] = *reinterpret_cast<const V*>(xhat + o);
    }
    rstd = save_rstd[t];
  }
  while (t < T) {
    const int tn = min(t + stride, T - 1);  // (clamped: the last prefetch re-reads a valid row and is dropped)
    V nd[NV], nh[NV], dh[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const size_t on = (size_t)tn * D + j * CW + lane * VW;
      nd[j] = *reinterpret_cast<const V*>(dout + on);
      nh[j] = *reinterpret_cast<const V*>(xhat + on);
    }
    const float nrstd = save_rstd[tn];
    float m1 = 0.f, m2 = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      ag[j] = vmap([](float acc, float p, float q) { return acc + p * q; }, ag[j], d[j], h[j]);
      vacc(ab[j], d[j]);
      dh[j] = vmap([](float p, float q) { return p * q; }, d[j], g[j]);
      m1 += vsum(dh[j]);
      m2 += vdot_pair(dh[j], h[j]);
    }
    m1 = wsum(m1) * (1.f / D);
    m2 = wsum(m2) * (1.f / D);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const size_t o = (size_t)t * D + j * CW + lane * VW;
      V dz = vmap([rstd, m1, m2](float p, float q) { return rstd * (p - m1 - q * m2); }, dh[j], h[j]);
      *reinterpret_cast<V*>(d_res + o) = dz;
      if (dr.thr) dz = vdrop(dz, dr, (uint32_t)o);
      *reinterpret_cast<V*>(d_y + o) = dz;
      d[j] = nd[j];
      h[j] = nh[j];
    }
    rstd = nrstd;
    t += stride;
  }
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    rg[threadIdx.x * NV + j] = ag[j];
    rb[threadIdx.x * NV + j] = ab[j];
  }
  __syncthreads();
  if (w == 0) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      V sg = ag[j], sb = ab[j];
      for (int i = 1; i < WAVES; ++i) {
        const V a = rg[(lane + 64 * i) * NV + j], c = rb[(lane + 64 * i) * NV + j];
        vacc(sg, a);
        vacc(sb, c);
      }
      vatomic_add(dgamma + j * CW + lane * VW, sg);
      vatomic_add(dbeta + j * CW + lane * VW, sb);
    }
  }
}

// feed-forward hidden dropout: hd = h * mask (forward); dh = dhd * mask * (h > 0) (backward, in place)
__global__ void drop_fwd_kernel(const float* __restrict__ h, size_t n, Drop dr, float* __restrict__ hd) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) hd[i] = keep_bit(dr.key, (uint32_t)i, dr.thr) ? h[i] * dr.scale : 0.f;
}
__global__ void relu_drop_bwd_kernel(float* __restrict__ d, const float* __restrict__ h, size_t n, Drop dr) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float v = h[i] > 0.f ? d[i] : 0.f;
  if (dr.thr) v = keep_bit(dr.key, (uint32_t)i, dr.thr) ? v * dr.scale : 0.f;
  d[i] = v;
}

// ---------------------------------------------------------------------------------------------------------------
// max over the 28 slots (first maximal slot wins) + F.normalize: one workgroup (256 threads = columns) per cell
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float block_sum256(float v, float* red) {
  v = wsum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}
__global__ __launch_bounds__(256) void pool_norm_fwd_kernel(const float* __restrict__ X, float* __restrict__ out,
                                                            int32_t* __restrict__ arg, float* __restrict__ save_n,
                                                            float* __restrict__ out2,  // out2: the caller's copy (no memcpy launch)
                                                            double* __restrict__ zero, int zero_n) {
  __shared__ float red[4];
  const int b = blockIdx.x, c = threadIdx.x;
  // the forward's last launch clears the BatchNorm accumulators of this step's backward and of the next forward (every
  // forward-side reader is behind it on the stream): no memset launch in the step
  for (int i = b * 256 + c; i < zero_n; i += gridDim.x * 256) zero[i] = 0.0;
  float mx = X[(size_t)b * kTS * kTD + c];
  int am = 0;
#pragma unroll
  for (int s = 1; s < kTS; ++s) {
    const float v = X[((size_t)b * kTS + s) * kTD + c];
    if (v > mx) { mx = v; am = s; }
  }
  const float n = fmaxf(sqrtf(block_sum256(mx * mx, red)), kNormEps);
  out[(size_t)b * kTD + c] = mx / n;
  out2[(size_t)b * kTD + c] = mx / n;
  arg[(size_t)b * kTD + c] = am;
  if (c == 0) save_n[b] = n;
}
__global__ __launch_bounds__(256) void pool_norm_bwd_kernel(const float* __restrict__ gout, const float* __restrict__ out,
                                                            const int32_t* __restrict__ arg,
                                                            const float* __restrict__ save_n, float* __restrict__ dX) {
  __shared__ float red[4];
  const int b = blockIdx.x, c = threadIdx.x;
  const float g = gout[(size_t)b * kTD + c], y = out[(size_t)b * kTD + c], n = save_n[b];
  const float t = block_sum256(g * y, red);
  const float d = n <= kNormEps ? g / kNormEps : (g - y * t) / n;
  const int am = arg[(size_t)b * kTD + c];
  for (int s = 0; s < kTS; ++s) dX[((size_t)b * kTS + s) * kTD + c] = (s == am) ? d : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------
// torch.optim.Adam (defaults: no weight decay, no amsgrad) over all bound tensors in ONE launch:
// chunk table entry = (tensor, first element); 1,024 elements per workgroup.
// ---------------------------------------------------------------------------------------------------------------
struct AdamTensor {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t numel;
};
struct AdamChunk {
  int32_t tensor;
  int32_t first;  // element offset / 1024
};
__global__ __launch_bounds__(256) void adam_kernel(const AdamTensor* __restrict__ ts, const AdamChunk* __restrict__ cs,
                                                   float lr, float b1, float b2, float eps, float bc1, float bc2_sqrt) {
  const AdamChunk c = cs[blockIdx.x];
  const AdamTensor t = ts[c.tensor];
  const int64_t base = (int64_t)c.first * 1024;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t i = base + j * 256 + threadIdx.x;
    if (i < t.numel) {
      const float g = t.g[i];
      const float m = b1 * t.m[i] + (1.f - b1) * g;
      const float v = b2 * t.v[i] + (1.f - b2) * g * g;
      t.m[i] = m;
      t.v[i] = v;
      t.p[i] -= (lr / bc1) * m / (sqrtf(v) / bc2_sqrt + eps);
    }
  }
}
__global__ void zero_kernel(const AdamTensor* __restrict__ ts, const AdamChunk* __restrict__ cs) {
  const AdamChunk c = cs[blockIdx.x];
  const AdamTensor t = ts[c.tensor];
  float* g = const_cast<float*>(t.g);
  const int64_t base = (int64_t)c.first * 1024;
  for (int j = 0; j < 4; ++j) {
    const int64_t i = base + j * 256 + threadIdx.x;
    if (i < t.numel) g[i] = 0.f;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// The text head's own ops (train.hip: text_train_*)
// ---------------------------------------------------------------------------------------------------------------
// out[b][c] = max over the S rows of group b of (X + R) (R optional: the residual AROUND the inter-sentence layer); first maximal
// row wins, as torch.max does. arg keeps the row for the backward scatter.
__global__ __launch_bounds__(256) void seq_max_fwd_kernel(const float* __restrict__ X, const float* __restrict__ R, int B, int S, int D,
                                                          float* __restrict__ out, int32_t* __restrict__ arg) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)B * D) return;
  const int b = (int)(i / D), c = (int)(i - (size_t)b * D);
  float mx = 0.f;
  int am = 0;
  for (int s = 0; s < S; ++s) {
    const size_t o = ((size_t)b * S + s) * D + c;
    const float v = R ? X[o] + R[o] : X[o];
    if (s == 0 || v > mx) { mx = v; am = s; }
  }
  out[i] = mx;
  arg[i] = am;
}
// dX[b][s][c] = g[b][c] at s = arg, else 0 (the gradient of X and, with a residual, of R alike)
__global__ __launch_bounds__(256) void seq_max_bwd_kernel(const float* __restrict__ g, const int32_t* __restrict__ arg, int B, int S, int D,
                                                          float* __restrict__ dX) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)B * S * D) return;
  const int c = (int)(i % D);
  const size_t bs = i / D;
  const int s = (int)(bs % S);
  const size_t b = bs / S;
  dX[i] = arg[b * D + c] == s ? g[b * D + c] : 0.f;
}

// BatchNorm1d in training mode WITHOUT a ReLU behind it (inter_mlp = get_mlp2([1024, D]): Linear + BatchNorm1d,
// models/language_encoder.py:43-74,99) over M rows (a few hundred sentences) x C <= 256 columns: one workgroup per 4 columns, 64 row
// lanes each (one thread per column looping over all rows was 150 us per pass: a third of a millisecond per step).
__device__ __forceinline__ void bn4_reduce(double s1, double s2, double (*red)[4][2], int cl, int rl, double& t1, double& t2) {
  red[rl][cl][0] = s1;
  red[rl][cl][1] = s2;
  __syncthreads();
  t1 = t2 = 0.0;
  for (int i = 0; i < 64; ++i) {
    t1 += red[i][cl][0];
    t2 += red[i][cl][1];
  }
  __syncthreads();
}
// PHASE 0: statistics + apply in one launch. Cross-rank statistics (t2l_train_sync_bn) split it: PHASE 1 stores this rank's sums and row
// count into the slot `acc` (plain stores: a column has one owner), the host sums the slot over the ranks, PHASE 2 applies from it.
template <int PHASE = 0>
__global__ __launch_bounds__(256) void bn_plain_fwd_kernel(const float* __restrict__ y, int M, int C, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float* __restrict__ run_mean,
                                                           float* __restrict__ run_var, float momentum, float* __restrict__ out,
                                                           float* __restrict__ save_mean, float* __restrict__ save_rstd,
                                                           double* __restrict__ acc = nullptr) {
  __shared__ double red[64][4][2];
  const int cl = threadIdx.x & 3, rl = threadIdx.x >> 2, c = blockIdx.x * 4 + cl;
  double t1, t2, Mg = (double)M;
  if (PHASE != 2) {
    double s1 = 0.0, s2 = 0.0;
    if (c < C)
      for (int m = rl; m < M; m += 64) {
        const double v = y[(size_t)m * C + c];
        s1 += v;
        s2 += v * v;
      }
    bn4_reduce(s1, s2, red, cl, rl, t1, t2);
  }
  if (PHASE == 1) {
    if (c < C && rl == 0) {
      acc[c] = t1;
      acc[C + c] = t2;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) acc[kBnCount] = (double)M;
    return;
  }
  if (c >= C) return;
  if (PHASE == 2) {
    t1 = acc[c];
    t2 = acc[C + c];
    Mg = acc[kBnCount];
  }
  const double mean = t1 / Mg, var = fmax(t2 / Mg - mean * mean, 0.0);
  const float rstd = 1.0f / sqrtf((float)var + kBnEps), g = gamma[c], be = beta[c];
  for (int m = rl; m < M; m += 64) out[(size_t)m * C + c] = (y[(size_t)m * C + c] - (float)mean) * rstd * g + be;
  if (rl == 0) {
    save_mean[c] = (float)mean;
    save_rstd[c] = rstd;
    run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * (float)mean;
    run_var[c] = (1.f - momentum) * run_var[c] + momentum * (float)(var * (Mg / fmax(Mg - 1.0, 1.0)));
  }
}
// d: gradient w.r.t. the BatchNorm output (in), overwritten with the gradient w.r.t. its input y. PHASE as above; the parameter
// gradients are this rank's own sums in every phase form (the gradient all_reduce adds the ranks' up).
template <int PHASE = 0>
__global__ __launch_bounds__(256) void bn_plain_bwd_kernel(float* __restrict__ d, const float* __restrict__ y, int M, int C,
                                                           const float* __restrict__ gamma, const float* __restrict__ save_mean,
                                                           const float* __restrict__ save_rstd, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta, double* __restrict__ acc = nullptr) {
  __shared__ double red[64][4][2];
  const int cl = threadIdx.x & 3, rl = threadIdx.x >> 2, c = blockIdx.x * 4 + cl;
  const float mean = c < C ? save_mean[c] : 0.f, rstd = c < C ? save_rstd[c] : 0.f;
  double t1, t2;
  float Mg = (float)M;
  if (PHASE != 2) {
    double s1 = 0.0, s2 = 0.0;
    if (c < C)
      for (int m = rl; m < M; m += 64) {
        const float dv = d[(size_t)m * C + c];
        s1 += dv;
        s2 += dv * (y[(size_t)m * C + c] - mean) * rstd;
      }
    bn4_reduce(s1, s2, red, cl, rl, t1, t2);
    if (c < C && rl == 0) {
      dgamma[c] += (float)t2;
      dbeta[c] += (float)t1;
    }
  }
  if (PHASE == 1) {
    if (c < C && rl == 0) {
      acc[c] = t1;
      acc[C + c] = t2;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) acc[kBnCount] = (double)M;
    return;
  }
  if (c >= C) return;
  if (PHASE == 2) {
    t1 = acc[c];
    t2 = acc[C + c];
    Mg = (float)acc[kBnCount];
  }
  const float f1 = (float)t1, f2 = (float)t2, g = gamma[c];
  for (int m = rl; m < M; m += 64) {
    const size_t i = (size_t)m * C + c;
    d[i] = g * rstd / Mg * (Mg * d[i] - f1 - (y[i] - mean) * rstd * f2);
  }
}

}  // namespace train
}  // namespace t2l
