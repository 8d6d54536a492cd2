// Fine stage under model.train(): one training step of CrossMatch downstream of the text branch
// (models/cross_matcher.py:86-135, training/fine.py:38-91) —
//   t2l_fine_train_bind     : live data / grad pointers of object_encoder.* (optionally with the PointNet++ backbone's
//                             object_encoder.pointnet.* group, class_embed == 0), cross_objects.*, cross_hints.*, mlp_offsets.*
//   t2l_fine_train_forward  : ObjectEncoder at d = 128 with batch-statistics BatchNorm (running buffers updated in place) +
//                             F.normalize, the CCAT cascade with the six dropout sites of every nn.TransformerDecoderLayer, max over
//                             the hints (arg-max kept), mlp_offsets
//   t2l_fine_train_forward_points : the same, with features2 from the backbone's training-mode forward on the pairs' point
//                             batches (one cell = one pair = 16 objects: pointnet_train.h, the coarse step's backbone code on a
//                             state of this context's own)
//   t2l_fine_train_backward : d offsets -> parameter gradients ADDED into the bound .grad buffers, d hint encodings, d features2,
//                             and on through the backbone after a points forward when it is bound with gradients
//   t2l_fine_zero_grad / t2l_fine_adam_step / t2l_fine_adam_state : optimizer.zero_grad() / Adam over the tensors bound with a gradient
//                             buffer (train.hip's AdamSet through train_common.h), one launch each
// With t2l_train_sync_bn set, the ObjectEncoder's BatchNorms take their statistics over every rank's rows: k_bn_stats_* / k_bn_apply_*
// around the caller's sum, the branches' layers side by side (one exchange per layer index, one for mlp_merge).
// Everything is f32 on the vector ALU. Residual + dropout + LayerNorm, F.normalize, the feed-forward dropout with its ReLU backward
// and the max over the hints are the coarse step's row kernels (train_kernels.h) at width 128, reached through train.hip's launchers
// (train_common.h). The kernels below are the ones the coarse step has no counterpart for:
//   k_gemm / k_colsum        a row-major tiled GEMM (64x64 tiles) over STRIDED operands, so one kernel serves X·Wᵀ, dY·W and the weight
//                            gradients dYᵀ·X (split over the rows with float atomics), at K = 1 or 3 and N = 2 too (gemm_f32.h wants
//                            N % 32 == 0 and K % 16 == 0)
//   k_attn_fwd / k_attn_bwd  one workgroup per (pair, head), CROSS-attention: Tq != Tk, separate Q / K / V strides (the coarse kernel
//                            is self-attention on packed qkv, its S = 28 instance latency-tuned); dmask is their dropout factor
//   k_bn_fwd / k_bn_bwd      BatchNorm + ReLU over plain rows, one workgroup per column (the coarse forms are per-job accumulators or
//                            have no ReLU)
//   k_gather / k_scatter_add / k_num_in   the embedding lookup that answers an out-of-range index with a zero row, its backward,
//                            num_encoder's input
// Moving one of these would change arithmetic or speed, not spelling. Activations of the last forward stay in a context-owned arena
// until the next forward (backward may run again on them: it reads the saved activations only). DESIGN.md §3.7b.
#include <math.h>
#include <string.h>

#include "t2l_internal.h"
#include "train_common.h"

namespace t2l {
namespace ft {

constexpr int kW = 128, kObj = 16, kHintMax = 8, kHeads = 4, kHd = 32, kFF = 512;
constexpr float kBnEps = 1e-5f, kBnMom = 0.1f;
constexpr int kLnWaves = 4;  // waves per workgroup of the LayerNorm backward (train.hip: ln_bwd_launch)

// shared with the coarse step (train_common.h): the a9 dropout rule — Drop, keep_bit, make_drop(seed, site, p) —, num_encoder's
// constants, the arena and the row kernels' launchers
using train::Arena;
using train::Drop;
using train::keep_bit;
using train::make_drop;

__device__ __forceinline__ float dmask(const Drop& d, uint32_t idx) {
  return d.thr ? (keep_bit(d.key, idx, d.thr) ? d.scale : 0.f) : 1.f;
}

// ---- C[M,N] (=|+=) A[M,K]·B[K,N] (+ bias[n]) (ReLU); A(m,k) = A[m*sam + k*sak], B(k,n) = B[k*sbk + n*sbn] -------------
struct Gemm {
  const float* A;
  int64_t sam, sak;
  const float* B;
  int64_t sbk, sbn;
  float* C;
  int64_t ldc;
  const float* bias;
  int M, N, K, acc, relu, kchunk;  // kchunk < K: blockIdx.z takes rows [z*kchunk, (z+1)*kchunk) of K and adds atomically
};

__global__ __launch_bounds__(256) void k_gemm(Gemm g) {
  __shared__ float As[16][68];
  __shared__ float Bs[16][68];
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
  const int kb = blockIdx.z * g.kchunk, ke = min(g.K, kb + g.kchunk);
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  for (int k0 = kb; k0 < ke; k0 += 16) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = t + i * 256;
      // consecutive lanes walk the operand's contiguous dimension (k for X and W in X·Wᵀ, m / n for dYᵀ·X and dY·W)
      const bool ak_fast = g.sak == 1, bn_fast = g.sbn == 1;
      const int ak = ak_fast ? (e & 15) : (e >> 6), am = ak_fast ? (e >> 4) : (e & 63);
      const int gm = m0 + am, gk = k0 + ak;
      As[ak][am] = (gm < g.M && gk < ke) ? g.A[(int64_t)gm * g.sam + (int64_t)gk * g.sak] : 0.f;
      const int bn = bn_fast ? (e & 63) : (e >> 4), bk = bn_fast ? (e >> 6) : (e & 15);
      const int gn = n0 + bn, gk2 = k0 + bk;
      Bs[bk][bn] = (gn < g.N && gk2 < ke) ? g.B[(int64_t)gk2 * g.sbk + (int64_t)gn * g.sbn] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      float a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        a[i] = As[kk][ty * 4 + i];
        b[i] = Bs[kk][tx * 4 + i];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
    }
    __syncthreads();
  }
  const bool split = gridDim.z > 1;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + ty * 4 + i;
    if (m >= g.M) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + tx * 4 + j;
      if (n >= g.N) continue;
      float* c = g.C + (int64_t)m * g.ldc + n;
      if (split) {
        atomicAdd(c, acc[i][j]);
        continue;
      }
      float v = acc[i][j];
      if (g.bias) v += g.bias[n];
      if (g.acc) v += *c;
      if (g.relu) v = fmaxf(v, 0.f);
      *c = v;
    }
  }
}

// out[n] += Σ_m X[m*ldx + n]
__global__ __launch_bounds__(256) void k_colsum(const float* X, int64_t ldx, int M, int N, float* out) {
  __shared__ float red[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), r = threadIdx.x >> 6;
  const int r0 = blockIdx.y * 256, r1 = min(M, r0 + 256);
  float s = 0.f;
  if (c < N)
    for (int m = r0 + r; m < r1; m += 4) s += X[(int64_t)m * ldx + c];
  red[r][threadIdx.x & 63] = s;
  __syncthreads();
  if (r == 0 && c < N) atomicAdd(&out[c], red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
}

__device__ double block_sum_d(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// BatchNorm1d (batch statistics) + ReLU over the M rows of column blockIdx.x. Y: pre-BN in, x̂ out (in place).
__global__ __launch_bounds__(256) void k_bn_fwd(float* Y, int M, int N, const float* g, const float* b, float* rm, float* rv,
                                                float* rstd_out, float* out) {
  __shared__ double red[256];
  const int n = blockIdx.x;
  double s = 0.0;
  for (int m = threadIdx.x; m < M; m += 256) s += Y[(int64_t)m * N + n];
  const double mean = block_sum_d(s, red) / M;
  double q = 0.0;
  for (int m = threadIdx.x; m < M; m += 256) {
    const double d = Y[(int64_t)m * N + n] - mean;
    q += d * d;
  }
  const double var = block_sum_d(q, red) / M;
  const float rstd = 1.f / sqrtf((float)var + kBnEps);
  const float mf = (float)mean, gn = g[n], bn = b[n];
  for (int m = threadIdx.x; m < M; m += 256) {
    const int64_t i = (int64_t)m * N + n;
    const float xh = (Y[i] - mf) * rstd;
    Y[i] = xh;
    out[i] = fmaxf(fmaf(xh, gn, bn), 0.f);
  }
  if (threadIdx.x == 0) {
    rstd_out[n] = rstd;
    if (rm) rm[n] = (1.f - kBnMom) * rm[n] + kBnMom * mf;
    if (rv) rv[n] = (1.f - kBnMom) * rv[n] + kBnMom * (float)(var * M / (M > 1 ? M - 1 : 1));
  }
}

// backward of k_bn_fwd: dout -> dy (pre-BN), dg / db added (one workgroup per column: no race)
__global__ __launch_bounds__(256) void k_bn_bwd(const float* dout, const float* out, const float* xhat, const float* rstd,
                                                const float* g, int M, int N, float* dg, float* db, float* dy) {
  __shared__ double red[256];
  const int n = blockIdx.x;
  double s = 0.0, sx = 0.0;
  for (int m = threadIdx.x; m < M; m += 256) {
    const int64_t i = (int64_t)m * N + n;
    const float dz = out[i] > 0.f ? dout[i] : 0.f;
    s += dz;
    sx += (double)dz * xhat[i];
  }
  const double sd = block_sum_d(s, red), sdx = block_sum_d(sx, red);
  const float k = g[n] * rstd[n] / M, sdf = (float)sd, sdxf = (float)sdx;
  for (int m = threadIdx.x; m < M; m += 256) {
    const int64_t i = (int64_t)m * N + n;
    const float dz = out[i] > 0.f ? dout[i] : 0.f;
    dy[i] = k * (M * dz - sdf - xhat[i] * sdxf);
  }
  if (threadIdx.x == 0) {
    if (dg) dg[n] += sdxf;
    if (db) db[n] += sdf;
  }
}

// ---- the same two in PHASES, for BatchNorm statistics over the rows of ALL ranks (t2l_train_sync_bn): a statistics launch leaves this
// rank's float64 column sums and its row count in an accumulator slot (train_common.h; plain stores — a column has one owner, so a slot
// needs no clearing and carries nothing from one launch to the next), the host sums the slot over the ranks, and an apply launch
// normalises by the global sums and the global row count at kBnCount. The scheme and the parameter-gradient rule are the coarse step's
// (train_kernels.h: bn_stats_body / bn_apply_*): dgamma / dbeta are this rank's OWN sums, taken in the statistics launch — the gradient
// all_reduce adds the ranks' up. The variance is E[y²] - mean² in float64 (the operands are float32, their squares exact in float64:
// the cancellation costs M 2^-52 (mean² + var), nothing beside the float32 rounding of mean and rstd), clamped at 0.
using train::kBnCount;
using train::kBnStride;

__global__ __launch_bounds__(256) void k_bn_stats_fwd(const float* Y, int M, int N, double* acc) {
  __shared__ double red[256];
  const int n = blockIdx.x;
  double s = 0.0, q = 0.0;
  for (int m = threadIdx.x; m < M; m += 256) {
    const double y = Y[(int64_t)m * N + n];
    s += y;
    q += y * y;
  }
  const double st = block_sum_d(s, red), qt = block_sum_d(q, red);
  if (threadIdx.x == 0) {
    acc[n] = st;
    acc[N + n] = qt;
    if (n == 0) acc[kBnCount] = (double)M;
  }
}

// Y: pre-BN in, x̂ out (in place), as k_bn_fwd; acc: the summed slot
__global__ __launch_bounds__(256) void k_bn_apply_fwd(float* Y, int M, int N, const float* g, const float* b, float* rm, float* rv,
                                                      float* rstd_out, float* out, const double* acc) {
  const int n = blockIdx.x;
  const double Mg = acc[kBnCount];
  const double mean = acc[n] / Mg;
  const double var = fmax(acc[N + n] / Mg - mean * mean, 0.0);
  const float rstd = 1.f / sqrtf((float)var + kBnEps);
  const float mf = (float)mean, gn = g[n], bn = b[n];
  for (int m = threadIdx.x; m < M; m += 256) {
    const int64_t i = (int64_t)m * N + n;
    const float xh = (Y[i] - mf) * rstd;
    Y[i] = xh;
    out[i] = fmaxf(fmaf(xh, gn, bn), 0.f);
  }
  if (threadIdx.x == 0) {
    rstd_out[n] = rstd;
    if (rm) rm[n] = (1.f - kBnMom) * rm[n] + kBnMom * mf;
    if (rv) rv[n] = (1.f - kBnMom) * rv[n] + kBnMom * (float)(var * Mg / (Mg > 1.0 ? Mg - 1.0 : 1.0));
  }
}

__global__ __launch_bounds__(256) void k_bn_stats_bwd(const float* dout, const float* out, const float* xhat, int M, int N, float* dg,
                                                      float* db, double* acc) {
  __shared__ double red[256];
  const int n = blockIdx.x;
  double s = 0.0, sx = 0.0;
  for (int m = threadIdx.x; m < M; m += 256) {
    const int64_t i = (int64_t)m * N + n;
    const float dz = out[i] > 0.f ? dout[i] : 0.f;
    s += dz;
    sx += (double)dz * xhat[i];
  }
  const double sd = block_sum_d(s, red), sdx = block_sum_d(sx, red);
  if (threadIdx.x == 0) {
    acc[n] = sd;
    acc[N + n] = sdx;
    if (n == 0) acc[kBnCount] = (double)M;
    if (dg) dg[n] += (float)sdx;
    if (db) db[n] += (float)sd;
  }
}

__global__ __launch_bounds__(256) void k_bn_apply_bwd(const float* dout, const float* out, const float* xhat, const float* rstd,
                                                      const float* g, int M, int N, const double* acc, float* dy) {
  const int n = blockIdx.x;
  const float Mg = (float)acc[kBnCount];
  const float k = g[n] * rstd[n] / Mg, sdf = (float)acc[n], sdxf = (float)acc[N + n];
  for (int m = threadIdx.x; m < M; m += 256) {
    const int64_t i = (int64_t)m * N + n;
    const float dz = out[i] > 0.f ? dout[i] : 0.f;
    dy[i] = k * (Mg * dz - sdf - xhat[i] * sdxf);
  }
}

// nn.Embedding lookup and its backward (padding_idx = 0 gets no gradient; out-of-range rows read zero and get nothing)
__global__ void k_gather(const float* table, int rows, const int32_t* idx, int M, float* out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)M * kW) return;
  const int r = idx[e / kW];
  out[e] = (r >= 0 && r < rows) ? table[(int64_t)r * kW + e % kW] : 0.f;
}

__global__ void k_scatter_add(const float* dY, int rows, const int32_t* idx, int M, float* grad) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)M * kW) return;
  const int r = idx[e / kW];
  if (r > 0 && r < rows) atomicAdd(&grad[(int64_t)r * kW + e % kW], dY[e]);
}

__global__ void k_num_in(const float* n_pts, int M, float* out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < M) out[i] = (n_pts[i] - train::kNumPtsMean) / train::kNumPtsStd;
}

// attention of one (pair, head): probabilities (before dropout) to P[pair, head, query, key], output to O[:, head*32 : +32]
__global__ __launch_bounds__(256) void k_attn_fwd(const float* Q, int64_t ldq, const float* K, int64_t ldk, const float* V,
                                                  int64_t ldv, int Tq, int Tk, float* P, float* O, int64_t ldo, Drop dr) {
  __shared__ float q[kObj][kHd + 1], k[kObj][kHd + 1], v[kObj][kHd + 1], s[kObj][kObj + 1];
  const int pair = blockIdx.x / kHeads, h = blockIdx.x % kHeads, t = threadIdx.x;
  for (int e = t; e < Tq * kHd; e += 256) q[e / kHd][e % kHd] = Q[((int64_t)pair * Tq + e / kHd) * ldq + h * kHd + e % kHd];
  for (int e = t; e < Tk * kHd; e += 256) {
    k[e / kHd][e % kHd] = K[((int64_t)pair * Tk + e / kHd) * ldk + h * kHd + e % kHd];
    v[e / kHd][e % kHd] = V[((int64_t)pair * Tk + e / kHd) * ldv + h * kHd + e % kHd];
  }
  __syncthreads();
  const float sc = 0.17677669529663687f;  // 1/sqrt(head_dim)
  if (t < Tq * Tk) {
    const int i = t / Tk, j = t % Tk;
    float a = 0.f;
#pragma unroll
    for (int d = 0; d < kHd; ++d) a = fmaf(q[i][d], k[j][d], a);
    s[i][j] = a * sc;
  }
  __syncthreads();
  if (t < Tq) {
    float mx = -INFINITY;
    for (int j = 0; j < Tk; ++j) mx = fmaxf(mx, s[t][j]);
    float sum = 0.f;
    for (int j = 0; j < Tk; ++j) {
      const float e = __expf(s[t][j] - mx);
      s[t][j] = e;
      sum += e;
    }
    const int64_t base = (((int64_t)pair * kHeads + h) * Tq + t) * Tk;
    for (int j = 0; j < Tk; ++j) {
      const float p = s[t][j] / sum;
      P[base + j] = p;
      s[t][j] = p * dmask(dr, (uint32_t)(base + j));
    }
  }
  __syncthreads();
  for (int e = t; e < Tq * kHd; e += 256) {
    const int i = e / kHd, d = e % kHd;
    float a = 0.f;
    for (int j = 0; j < Tk; ++j) a = fmaf(s[i][j], v[j][d], a);
    O[((int64_t)pair * Tq + i) * ldo + h * kHd + d] = a;
  }
}

__global__ __launch_bounds__(256) void k_attn_bwd(const float* Q, int64_t ldq, const float* K, int64_t ldk, const float* V,
                                                  int64_t ldv, const float* P, const float* dO, int64_t lddo, float* dQ,
                                                  int64_t lddq, float* dK, int64_t lddk, float* dV, int64_t lddv, int Tq, int Tk,
                                                  Drop dr) {
  __shared__ float q[kObj][kHd + 1], k[kObj][kHd + 1], v[kObj][kHd + 1], go[kObj][kHd + 1];
  __shared__ float p[kObj][kObj + 1], pd[kObj][kObj + 1], ds[kObj][kObj + 1];
  const int pair = blockIdx.x / kHeads, h = blockIdx.x % kHeads, t = threadIdx.x;
  for (int e = t; e < Tq * kHd; e += 256) {
    const int64_t r = (int64_t)pair * Tq + e / kHd;
    q[e / kHd][e % kHd] = Q[r * ldq + h * kHd + e % kHd];
    go[e / kHd][e % kHd] = dO[r * lddo + h * kHd + e % kHd];
  }
  for (int e = t; e < Tk * kHd; e += 256) {
    const int64_t r = (int64_t)pair * Tk + e / kHd;
    k[e / kHd][e % kHd] = K[r * ldk + h * kHd + e % kHd];
    v[e / kHd][e % kHd] = V[r * ldv + h * kHd + e % kHd];
  }
  const int64_t base = ((int64_t)pair * kHeads + h) * Tq * Tk;
  if (t < Tq * Tk) {
    const int i = t / Tk, j = t % Tk;
    const float m = dmask(dr, (uint32_t)(base + t));
    p[i][j] = P[base + t];
    pd[i][j] = p[i][j] * m;
    ds[i][j] = m;  // the mask, until the next step
  }
  __syncthreads();
  if (t < Tq * Tk) {
    const int i = t / Tk, j = t % Tk;
    float a = 0.f;
#pragma unroll
    for (int d = 0; d < kHd; ++d) a = fmaf(go[i][d], v[j][d], a);
    ds[i][j] *= a;  // d loss / d probabilities (before dropout)
  }
  __syncthreads();
  if (t < Tq) {
    float r = 0.f;
    for (int j = 0; j < Tk; ++j) r += p[t][j] * ds[t][j];
    for (int j = 0; j < Tk; ++j) ds[t][j] = p[t][j] * (ds[t][j] - r) * 0.17677669529663687f;
  }
  __syncthreads();
  for (int e = t; e < Tq * kHd; e += 256) {
    const int i = e / kHd, d = e % kHd;
    float a = 0.f;
    for (int j = 0; j < Tk; ++j) a = fmaf(ds[i][j], k[j][d], a);
    dQ[((int64_t)pair * Tq + i) * lddq + h * kHd + d] = a;
  }
  for (int e = t; e < Tk * kHd; e += 256) {
    const int j = e / kHd, d = e % kHd;
    float a = 0.f, b = 0.f;
    for (int i = 0; i < Tq; ++i) {
      a = fmaf(ds[i][j], q[i][d], a);
      b = fmaf(pd[i][j], go[i][d], b);
    }
    dK[((int64_t)pair * Tk + j) * lddk + h * kHd + d] = a;
    dV[((int64_t)pair * Tk + j) * lddv + h * kHd + d] = b;
  }
}

// ------------------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------------------
struct Ten {
  float* d = nullptr;  // live parameter / buffer
  float* g = nullptr;  // its .grad, or null (frozen parameter, or a buffer)
  int64_t n = 0;
};
struct BnLayer {  // get_mlp block: Linear(K -> N), BatchNorm1d(N), ReLU
  Ten w, b, bw, bb, rm, rv;
  int K = 0, N = 0;
  // saved by the forward
  const float* x = nullptr;
  float *xhat = nullptr, *rstd = nullptr, *out = nullptr;
};
struct Branch {
  bool used = false, embed = false;
  Ten table;  // nn.Embedding [rows,128]
  std::vector<BnLayer> mlp;
  float *raw = nullptr, *nrm = nullptr, *in = nullptr;  // embedding rows / F.normalize norms / num-encoder input
  // cross-rank statistics only: the backward runs the branches' layers side by side (one exchange per layer index), so each MLP branch
  // keeps its own d output [M0,128], d pre-BN of the last layer [M0,128], and for a two-layer branch d hidden / d pre-BN [M0,64]
  float *s_draw = nullptr, *s_dy = nullptr, *s_d0 = nullptr, *s_dy0 = nullptr;
};
struct DecLayer {
  Ten in_w, in_b, out_w, out_b, cin_w, cin_b, cout_w, cout_b, l1_w, l1_b, l2_w, l2_b, n1_w, n1_b, n2_w, n2_b, n3_w, n3_b;
  bool obj = false;  // cross_objects.* (tgt = the 16 objects) or cross_hints.*
  int Tq = 0, Tk = 0, site = 0;
  const float *x = nullptr, *mem = nullptr;
  float *qkv, *Ps, *os, *xh1, *r1, *x1, *q2, *kv2, *Pc, *oc, *xh2, *r2, *x2, *h1, *h1d, *xh3, *r3, *out;
};

struct FineTrain {
  int class_embed = 0, color_embed = 0, n_layers = 0, n_feat = 0;
  Branch br[4];  // class, color, position, num (object_encoder.py:102-145 code order)
  BnLayer merge;
  bool pn_stats = false;  // class_embed off without "class" in use_features: mlp_pointnet still runs (object_encoder.py:86-99)
  BnLayer pn_only;        // ... for its BatchNorm running statistics only (its output is unused: no gradient)
  std::vector<DecLayer> dec;  // cascade order: cross_objects.0, cross_hints.0, cross_objects.1, ... (or cross_hints alone)
  Ten o0w, o0b, o2w, o2b;
  PnTrain* pn = nullptr;  // the PointNet++ backbone's training state (object_encoder.pointnet.* bound), or null
  // the optimizer (t2l_fine_adam_step): every tensor bound with a gradient buffer, in bind order with the backbone's group behind the
  // rest — tensors [0, n_own) step on every call, [n_own, n_adam) only when the backward went through the backbone since the last
  // t2l_fine_zero_grad (torch.optim.Adam skips a .grad of None and counts steps per parameter: the coarse step's rule, train.hip)
  AdamSet* adam = nullptr;  // null: nothing is trained
  size_t n_own = 0, n_adam = 0;
  int64_t step = 0, step_pn = 0;
  bool pn_touched = false;
  // the last forward
  bool have_fwd = false;
  bool sync = false;      // ... exchanged its BatchNorm statistics across the ranks (ctx->sync_fn was set): the backward does too
  bool pn_fwd = false;    // ... took features2 from the backbone (t2l_fine_train_forward_points)
  int P = 0, H = 0;
  float p = 0.f;
  uint32_t seed = 0;
  const int32_t *class_idx = nullptr, *color_idx = nullptr;
  const float *rgb = nullptr, *center = nullptr, *n_pts = nullptr, *pn_feat = nullptr, *hint = nullptr;
  float *E = nullptr, *D0 = nullptr, *nrm0 = nullptr, *pool = nullptr, *a1 = nullptr;
  int32_t* arg = nullptr;
  // backward scratch
  float *gA0, *gB0, *gA1, *gB1, *t_dx1, *t_dx2, *t_ds, *t_do, *t_dq, *t_dkv, *t_dh, *dE, *ta, *tb, *dpool, *da1;
  float* dpn = nullptr;  // d features2 on its way into the backbone's backward (when the caller passes no grad_pn_feat)
  float* sink = nullptr;  // [2][128], never read: where the LayerNorm backward adds d weight / d bias of a frozen norm
  Arena ws;               // one allocation for all of the above
};

static void free_ft(FineTrain* st) {
  if (!st) return;
  if (st->ws.base) (void)hipFree(st->ws.base);
  pn_train_release(st->pn);
  adam_set_free(st->adam);
  delete st;
}

static inline unsigned nblk(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

static void gemm(hipStream_t s, const float* A, int64_t sam, int64_t sak, const float* B, int64_t sbk, int64_t sbn, float* C, int64_t ldc,
                 const float* bias, int M, int N, int K, int acc, int relu) {
  if (M <= 0 || N <= 0) return;
  Gemm g{A, sam, sak, B, sbk, sbn, C, ldc, bias, M, N, K, acc, relu, K};
  hipLaunchKernelGGL(k_gemm, dim3(nblk(N, 64), nblk(M, 64), 1), dim3(256), 0, s, g);
}
// Y[M,N] = X[M,K]·Wᵀ + b (W row-major [N,K] with row stride ldw)
static void lin_fwd(hipStream_t s, const float* X, int64_t ldx, int M, int K, const float* W, int64_t ldw, const float* b, int N, float* Y,
                    int64_t ldy, int relu = 0) {
  gemm(s, X, ldx, 1, W, 1, ldw, Y, ldy, b, M, N, K, 0, relu);
}
// dX[M,K] (+)= dY[M,N]·W
static void lin_dx(hipStream_t s, const float* dY, int64_t ldd, int M, int N, const float* W, int64_t ldw, int K, float* dX, int64_t ldx,
                   int acc) {
  gemm(s, dY, ldd, 1, W, ldw, 1, dX, ldx, nullptr, M, K, N, acc, 0);
}
// dW[N,K] += dYᵀ·X, db[N] += Σ rows of dY (skipped for frozen tensors)
static void lin_dw(hipStream_t s, const float* dY, int64_t ldd, const float* X, int64_t ldx, int M, int N, int K, float* dW, int64_t ldw,
                   float* db) {
  if (M <= 0) return;
  if (dW) {  // few output tiles, many rows: slices of 256 rows, added atomically
    Gemm g{dY, 1, ldd, X, ldx, 1, dW, ldw, nullptr, N, K, M, 1, 0, M};
    unsigned z = 1;
    if (M > 256) {
      g.kchunk = 256;
      z = nblk(M, 256);
    }
    hipLaunchKernelGGL(k_gemm, dim3(nblk(K, 64), nblk(N, 64), z), dim3(256), 0, s, g);
  }
  if (db) hipLaunchKernelGGL(k_colsum, dim3(nblk(N, 64), nblk(M, 256)), dim3(256), 0, s, dY, ldd, M, N, db);
}

// every pointer of the step inside one arena (count pass with base == null, then the real pass)
static void plan(FineTrain* st, Arena& a, int P, int H, float p, bool sync) {
  const int M0 = P * kObj, M1 = P * H, Mx = M0 > M1 ? M0 : M1;
  for (auto& b : st->br) {
    if (!b.used) continue;
    if (b.embed) b.raw = a.take<float>((int64_t)M0 * kW);
    for (auto& l : b.mlp) {
      l.xhat = a.take<float>((int64_t)M0 * l.N);
      l.out = a.take<float>((int64_t)M0 * l.N);
      l.rstd = a.take<float>(l.N);
    }
    b.nrm = a.take<float>(M0);
    b.in = a.take<float>(M0);
    if (sync && !b.embed) {
      b.s_draw = a.take<float>((int64_t)M0 * kW);
      b.s_dy = a.take<float>((int64_t)M0 * kW);
      if (b.mlp.size() > 1) {
        b.s_d0 = a.take<float>((int64_t)M0 * 64);
        b.s_dy0 = a.take<float>((int64_t)M0 * 64);
      }
    }
  }
  st->E = a.take<float>((int64_t)M0 * kW * st->n_feat);
  if (st->n_feat > 1) {
    st->merge.xhat = a.take<float>((int64_t)M0 * kW);
    st->merge.out = a.take<float>((int64_t)M0 * kW);
    st->merge.rstd = a.take<float>(kW);
  }
  if (st->pn_stats) {
    st->pn_only.xhat = a.take<float>((int64_t)M0 * kW);
    st->pn_only.out = a.take<float>((int64_t)M0 * kW);
    st->pn_only.rstd = a.take<float>(kW);
  }
  st->D0 = a.take<float>((int64_t)M0 * kW);
  st->nrm0 = a.take<float>(M0);
  for (auto& L : st->dec) {
    const int M = L.obj ? M0 : M1, Mm = L.obj ? M1 : M0;
    L.qkv = a.take<float>((int64_t)M * 3 * kW);
    L.Ps = a.take<float>((int64_t)P * kHeads * L.Tq * L.Tq);
    L.os = a.take<float>((int64_t)M * kW);
    L.xh1 = a.take<float>((int64_t)M * kW);
    L.r1 = a.take<float>(M);
    L.x1 = a.take<float>((int64_t)M * kW);
    L.q2 = a.take<float>((int64_t)M * kW);
    L.kv2 = a.take<float>((int64_t)Mm * 2 * kW);
    L.Pc = a.take<float>((int64_t)P * kHeads * L.Tq * L.Tk);
    L.oc = a.take<float>((int64_t)M * kW);
    L.xh2 = a.take<float>((int64_t)M * kW);
    L.r2 = a.take<float>(M);
    L.x2 = a.take<float>((int64_t)M * kW);
    L.h1 = a.take<float>((int64_t)M * kFF);
    L.h1d = p > 0.f ? a.take<float>((int64_t)M * kFF) : L.h1;
    L.xh3 = a.take<float>((int64_t)M * kW);
    L.r3 = a.take<float>(M);
    L.out = a.take<float>((int64_t)M * kW);
  }
  st->pool = a.take<float>((int64_t)P * kW);
  st->arg = a.take<int32_t>((int64_t)P * kW);
  st->a1 = a.take<float>((int64_t)P * 64);
  st->gA0 = a.take<float>((int64_t)M0 * kW);
  st->gB0 = a.take<float>((int64_t)M0 * kW);
  st->gA1 = a.take<float>((int64_t)M1 * kW);
  st->gB1 = a.take<float>((int64_t)M1 * kW);
  st->t_dx1 = a.take<float>((int64_t)Mx * kW);
  st->t_dx2 = a.take<float>((int64_t)Mx * kW);
  st->t_ds = a.take<float>((int64_t)Mx * kW);
  st->t_do = a.take<float>((int64_t)Mx * kW);
  st->t_dq = a.take<float>((int64_t)Mx * 3 * kW);
  st->t_dkv = a.take<float>((int64_t)Mx * 2 * kW);
  st->t_dh = a.take<float>((int64_t)Mx * kFF);
  st->dE = a.take<float>((int64_t)M0 * kW * st->n_feat);
  st->ta = a.take<float>((int64_t)M0 * 256);
  st->tb = a.take<float>((int64_t)M0 * 256);
  st->dpool = a.take<float>((int64_t)P * kW);
  st->da1 = a.take<float>((int64_t)P * 64);
  st->dpn = st->pn ? a.take<float>((int64_t)M0 * 256) : nullptr;
  st->sink = a.take<float>(2 * kW);
}

// one nn.TransformerDecoderLayer (post-norm, ReLU, no masks) in training mode: L.x [P*Tq,128] attends itself, then L.mem.
// false (here and in dec_bwd): a row kernel has no instance of width 128
static bool dec_fwd(FineTrain* st, DecLayer& L, float p, uint32_t seed, float* tmp, hipStream_t s) {
  const int P = st->P, M = P * L.Tq, Mm = P * L.Tk;
  // Y = LayerNorm(X + dropout(S)); x̂ and 1/σ saved
  auto ln_fwd = [&](const float* X, const float* S, const Ten& g, const Ten& b, int site, float* xh, float* r, float* Y) {
    return ln_fwd_rows(kW, X, S, M, g.d, b.d, make_drop(seed, site, p), Y, xh, r, s);
  };
  // self-attention block + dropout1 + norm1
  lin_fwd(s, L.x, kW, M, kW, L.in_w.d, kW, L.in_b.d, 3 * kW, L.qkv, 3 * kW);
  hipLaunchKernelGGL(k_attn_fwd, dim3(P * kHeads), dim3(256), 0, s, L.qkv, (int64_t)3 * kW, L.qkv + kW, (int64_t)3 * kW, L.qkv + 2 * kW,
                     (int64_t)3 * kW, L.Tq, L.Tq, L.Ps, L.os, (int64_t)kW, make_drop(seed, L.site + 0, p));
  lin_fwd(s, L.os, kW, M, kW, L.out_w.d, kW, L.out_b.d, kW, tmp, kW);
  bool ok = ln_fwd(L.x, tmp, L.n1_w, L.n1_b, L.site + 1, L.xh1, L.r1, L.x1);
  // cross-attention block + dropout2 + norm2
  lin_fwd(s, L.x1, kW, M, kW, L.cin_w.d, kW, L.cin_b.d, kW, L.q2, kW);
  lin_fwd(s, L.mem, kW, Mm, kW, L.cin_w.d + kW * kW, kW, L.cin_b.d + kW, 2 * kW, L.kv2, 2 * kW);
  hipLaunchKernelGGL(k_attn_fwd, dim3(P * kHeads), dim3(256), 0, s, L.q2, (int64_t)kW, L.kv2, (int64_t)2 * kW, L.kv2 + kW, (int64_t)2 * kW,
                     L.Tq, L.Tk, L.Pc, L.oc, (int64_t)kW, make_drop(seed, L.site + 2, p));
  lin_fwd(s, L.oc, kW, M, kW, L.cout_w.d, kW, L.cout_b.d, kW, tmp, kW);
  ok = ln_fwd(L.x1, tmp, L.n2_w, L.n2_b, L.site + 3, L.xh2, L.r2, L.x2) && ok;
  // feed-forward block + dropout3 + norm3
  lin_fwd(s, L.x2, kW, M, kW, L.l1_w.d, kW, L.l1_b.d, kFF, L.h1, kFF, 1);
  if (L.h1d != L.h1) drop_fwd_launch(L.h1, (size_t)M * kFF, make_drop(seed, L.site + 4, p), L.h1d, s);
  lin_fwd(s, L.h1d, kFF, M, kFF, L.l2_w.d, kFF, L.l2_b.d, kW, tmp, kW);
  return ln_fwd(L.x2, tmp, L.n3_w, L.n3_b, L.site + 5, L.xh3, L.r3, L.out) && ok;
}

// backward of dec_fwd: dout -> dx (written), d mem ADDED to dmem
static bool dec_bwd(FineTrain* st, DecLayer& L, float p, uint32_t seed, const float* dout, float* dx, float* dmem, hipStream_t s) {
  const int P = st->P, M = P * L.Tq, Mm = P * L.Tk;
  float *dx2 = st->t_dx2, *dx1 = st->t_dx1, *ds = st->t_ds, *dob = st->t_do, *dq = st->t_dq, *dkv = st->t_dkv, *dh = st->t_dh;
  // dZ = d loss / d (X + dropout(S)) (the residual's gradient), dS = dZ through the dropout mask; d weight / d bias added
  auto ln_bwd = [&](const float* dY, const float* xh, const float* r, const Ten& g, const Ten& b, int site, float* dZ) {
    return ln_bwd_rows(kW, kLnWaves, dY, xh, r, M, g.d, make_drop(seed, site, p), dZ, ds, g.g ? g.g : st->sink, b.g ? b.g : st->sink + kW, s);
  };
  // norm3 / dropout3 / feed-forward
  bool ok = ln_bwd(dout, L.xh3, L.r3, L.n3_w, L.n3_b, L.site + 5, dx2);
  lin_dw(s, ds, kW, L.h1d, kFF, M, kW, kFF, L.l2_w.g, kFF, L.l2_b.g);
  lin_dx(s, ds, kW, M, kW, L.l2_w.d, kFF, kFF, dh, kFF, 0);
  relu_drop_bwd_launch(dh, L.h1, (size_t)M * kFF, make_drop(seed, L.site + 4, p), s);
  lin_dw(s, dh, kFF, L.x2, kW, M, kFF, kW, L.l1_w.g, kW, L.l1_b.g);
  lin_dx(s, dh, kFF, M, kFF, L.l1_w.d, kW, kW, dx2, kW, 1);
  // norm2 / dropout2 / cross-attention
  ok = ln_bwd(dx2, L.xh2, L.r2, L.n2_w, L.n2_b, L.site + 3, dx1) && ok;
  lin_dw(s, ds, kW, L.oc, kW, M, kW, kW, L.cout_w.g, kW, L.cout_b.g);
  lin_dx(s, ds, kW, M, kW, L.cout_w.d, kW, kW, dob, kW, 0);
  hipLaunchKernelGGL(k_attn_bwd, dim3(P * kHeads), dim3(256), 0, s, L.q2, (int64_t)kW, L.kv2, (int64_t)2 * kW, L.kv2 + kW, (int64_t)2 * kW,
                     L.Pc, dob, (int64_t)kW, dq, (int64_t)kW, dkv, (int64_t)2 * kW, dkv + kW, (int64_t)2 * kW, L.Tq, L.Tk,
                     make_drop(seed, L.site + 2, p));
  lin_dw(s, dq, kW, L.x1, kW, M, kW, kW, L.cin_w.g, kW, L.cin_b.g);
  lin_dx(s, dq, kW, M, kW, L.cin_w.d, kW, kW, dx1, kW, 1);
  lin_dw(s, dkv, 2 * kW, L.mem, kW, Mm, 2 * kW, kW, L.cin_w.g ? L.cin_w.g + kW * kW : nullptr, kW, L.cin_b.g ? L.cin_b.g + kW : nullptr);
  lin_dx(s, dkv, 2 * kW, Mm, 2 * kW, L.cin_w.d + kW * kW, kW, kW, dmem, kW, 1);
  // norm1 / dropout1 / self-attention
  ok = ln_bwd(dx1, L.xh1, L.r1, L.n1_w, L.n1_b, L.site + 1, dx) && ok;
  lin_dw(s, ds, kW, L.os, kW, M, kW, kW, L.out_w.g, kW, L.out_b.g);
  lin_dx(s, ds, kW, M, kW, L.out_w.d, kW, kW, dob, kW, 0);
  hipLaunchKernelGGL(k_attn_bwd, dim3(P * kHeads), dim3(256), 0, s, L.qkv, (int64_t)3 * kW, L.qkv + kW, (int64_t)3 * kW, L.qkv + 2 * kW,
                     (int64_t)3 * kW, L.Ps, dob, (int64_t)kW, dq, (int64_t)3 * kW, dq + kW, (int64_t)3 * kW, dq + 2 * kW, (int64_t)3 * kW,
                     L.Tq, L.Tq, make_drop(seed, L.site + 0, p));
  lin_dw(s, dq, 3 * kW, L.x, kW, M, 3 * kW, kW, L.in_w.g, kW, L.in_b.g);
  lin_dx(s, dq, 3 * kW, M, 3 * kW, L.in_w.d, kW, kW, dx, kW, 1);
  return ok;
}

// ---- launchers of the phased BatchNorm (the dev library's wrapper goes through them too)
static void bn_stats_fwd_launch(const float* Y, int M, int N, double* acc, hipStream_t s) {
  hipLaunchKernelGGL(k_bn_stats_fwd, dim3(N), dim3(256), 0, s, Y, M, N, acc);
}
static void bn_apply_fwd_launch(float* Y, int M, int N, const float* g, const float* b, float* rm, float* rv, float* rstd, float* out,
                                const double* acc, hipStream_t s) {
  hipLaunchKernelGGL(k_bn_apply_fwd, dim3(N), dim3(256), 0, s, Y, M, N, g, b, rm, rv, rstd, out, acc);
}
static void bn_stats_bwd_launch(const float* dout, const float* out, const float* xhat, int M, int N, float* dg, float* db, double* acc,
                                hipStream_t s) {
  hipLaunchKernelGGL(k_bn_stats_bwd, dim3(N), dim3(256), 0, s, dout, out, xhat, M, N, dg, db, acc);
}
static void bn_apply_bwd_launch(const float* dout, const float* out, const float* xhat, const float* rstd, const float* g, int M, int N,
                                const double* acc, float* dy, hipStream_t s) {
  hipLaunchKernelGGL(k_bn_apply_bwd, dim3(N), dim3(256), 0, s, dout, out, xhat, rstd, g, M, N, acc, dy);
}

// One exchange of the cross-rank statistics: up to kFineBnSlots independent layers of the same row count, slot i for layer i — every
// statistics launch, ONE call of the caller's sum over the slots in use, every apply launch.
struct BnJob {
  BnLayer* l;
  const float* x;     // forward: the layer's input
  const float* dout;  // backward: d of the layer's output
  float *dy, *dx;     // backward: d pre-BN (scratch [M,N]); d input [M,K] or null
};
static double* sync_slot(t2l_ctx* ctx, size_t i) { return ctx->sync_buf + (size_t)(train::kFineBnSlot0 + i) * kBnStride; }
static void sync_sum(t2l_ctx* ctx, size_t slots, hipStream_t s) {
  if (ctx->sync_failed) return;  // (no further collective from a rank whose last one failed)
  if (ctx->sync_fn(ctx->sync_user, sync_slot(ctx, 0), (int64_t)slots * kBnStride, (void*)s) != 0) ctx->sync_failed = true;
}
// false (here and in bn_stage_bwd): more layers than slots, or the callback failed — nothing more of the step should run
static bool bn_stage_fwd(t2l_ctx* ctx, const std::vector<BnJob>& jobs, int M, hipStream_t s) {
  if (jobs.empty()) return true;
  if (jobs.size() > (size_t)train::kFineBnSlots) return false;  // (at most class, color, position, num side by side)
  for (size_t i = 0; i < jobs.size(); ++i) {
    BnLayer& l = *jobs[i].l;
    l.x = jobs[i].x;
    lin_fwd(s, l.x, l.K, M, l.K, l.w.d, l.K, l.b.d, l.N, l.xhat, l.N);
    bn_stats_fwd_launch(l.xhat, M, l.N, sync_slot(ctx, i), s);
  }
  sync_sum(ctx, jobs.size(), s);
  if (ctx->sync_failed) return false;
  for (size_t i = 0; i < jobs.size(); ++i) {
    BnLayer& l = *jobs[i].l;
    bn_apply_fwd_launch(l.xhat, M, l.N, l.bw.d, l.bb.d, l.rm.d, l.rv.d, l.rstd, l.out, sync_slot(ctx, i), s);
  }
  return true;
}
static bool bn_stage_bwd(t2l_ctx* ctx, const std::vector<BnJob>& jobs, int M, hipStream_t s) {
  if (jobs.empty()) return true;
  if (jobs.size() > (size_t)train::kFineBnSlots) return false;
  for (size_t i = 0; i < jobs.size(); ++i) {
    BnLayer& l = *jobs[i].l;
    bn_stats_bwd_launch(jobs[i].dout, l.out, l.xhat, M, l.N, l.bw.g, l.bb.g, sync_slot(ctx, i), s);
  }
  sync_sum(ctx, jobs.size(), s);
  if (ctx->sync_failed) return false;
  for (size_t i = 0; i < jobs.size(); ++i) {
    BnLayer& l = *jobs[i].l;
    bn_apply_bwd_launch(jobs[i].dout, l.out, l.xhat, l.rstd, l.bw.d, M, l.N, sync_slot(ctx, i), jobs[i].dy, s);
    lin_dw(s, jobs[i].dy, l.N, l.x, l.K, M, l.N, l.K, l.w.g, l.K, l.b.g);
    if (jobs[i].dx) lin_dx(s, jobs[i].dy, l.N, M, l.N, l.w.d, l.K, l.K, jobs[i].dx, l.K, 0);
  }
  return true;
}
// what a step answers when a stage returned false
static int stage_failed(t2l_ctx* ctx, const char* who) {
  (void)hipGetLastError();
  if (ctx->sync_failed) return fail(ctx, T2L_ESTATE, std::string(who) + ": the cross-rank sum callback (t2l_train_sync_bn) failed");
  return fail(ctx, T2L_ESTATE, std::string(who) + ": more BatchNorm layers in one exchange than the fine step has slots");
}

static void bn_layer_fwd(BnLayer& l, const float* x, int M, hipStream_t s) {
  l.x = x;
  lin_fwd(s, x, l.K, M, l.K, l.w.d, l.K, l.b.d, l.N, l.xhat, l.N);
  hipLaunchKernelGGL(k_bn_fwd, dim3(l.N), dim3(256), 0, s, l.xhat, M, l.N, l.bw.d, l.bb.d, l.rm.d, l.rv.d, l.rstd, l.out);
}

// dout [M,N] of the block's output -> parameter gradients, and d input [M,K] into dx when non-null (dy: scratch [M,N])
static void bn_layer_bwd(BnLayer& l, const float* dout, int M, float* dy, float* dx, hipStream_t s) {
  hipLaunchKernelGGL(k_bn_bwd, dim3(l.N), dim3(256), 0, s, dout, l.out, l.xhat, l.rstd, l.bw.d, M, l.N, l.bw.g, l.bb.g, dy);
  lin_dw(s, dy, l.N, l.x, l.K, M, l.N, l.K, l.w.g, l.K, l.b.g);
  if (dx) lin_dx(s, dy, l.N, M, l.N, l.w.d, l.K, l.K, dx, l.K, 0);
}

}  // namespace ft

using namespace ft;

void free_fine_train(t2l_ctx* ctx) {
  free_ft((FineTrain*)ctx->fine_train);
  ctx->fine_train = nullptr;
}

int fine_train_bind_impl(t2l_ctx* ctx, const t2l_train_tensor* tensors, int n, const t2l_model_config* cfg) {
  if (!cfg || (n > 0 && !tensors) || n < 0) return fail(ctx, T2L_EINVAL, "fine_train_bind: null tensors / cfg");
  if (cfg->num_layers < 0 || cfg->num_layers > 4) return fail(ctx, T2L_EINVAL, "fine_train_bind: num_layers must be 0..4");
  if (cfg->num_heads != kHeads) return fail(ctx, T2L_EINVAL, "fine_train_bind: the fine stage is built for 4 heads");
  std::unordered_map<std::string, const t2l_train_tensor*> by;
  for (int i = 0; i < n; ++i) {
    if (!tensors[i].name || !tensors[i].data) return fail(ctx, T2L_EINVAL, "fine_train_bind: tensor without name or data");
    by[tensors[i].name] = &tensors[i];
  }
  std::string err;
  auto get = [&](const std::string& name, int64_t numel, bool buffer) -> Ten {
    Ten t;
    auto it = by.find(name);
    if (it == by.end()) {
      if (err.empty()) err = "fine_train_bind: missing tensor " + name;
      return t;
    }
    if (numel > 0 && it->second->numel != numel) {
      if (err.empty()) err = "fine_train_bind: " + name + " has " + std::to_string(it->second->numel) + " elements, expected " + std::to_string(numel);
      return t;
    }
    if (numel <= 0 && (it->second->numel <= 0 || it->second->numel % kW)) {
      if (err.empty()) err = "fine_train_bind: " + name + " must be [rows,128]";
      return t;
    }
    t.d = it->second->data;
    t.g = buffer ? nullptr : it->second->grad;
    t.n = it->second->numel;
    return t;
  };
  auto bn_layer = [&](const std::string& pre, int K, int N) {
    BnLayer l;
    l.K = K;
    l.N = N;
    l.w = get(pre + ".0.weight", (int64_t)N * K, false);
    l.b = get(pre + ".0.bias", N, false);
    l.bw = get(pre + ".1.weight", N, false);
    l.bb = get(pre + ".1.bias", N, false);
    l.rm = get(pre + ".1.running_mean", N, true);
    l.rv = get(pre + ".1.running_var", N, true);
    return l;
  };
  auto* st = new FineTrain();
  const std::string oe = "object_encoder.";
  st->class_embed = cfg->class_embed;
  st->color_embed = cfg->color_embed;
  st->n_layers = cfg->num_layers;
  const int use[4] = {cfg->use_class, cfg->use_color, cfg->use_position, cfg->use_num};
  for (int f = 0; f < 4; ++f) {
    Branch& b = st->br[f];
    b.used = use[f] != 0;
    if (!b.used) continue;
    ++st->n_feat;
    if (f == 0 && cfg->class_embed) {
      b.embed = true;
      b.table = get(oe + "class_embedding.weight", 0, false);
    } else if (f == 0) {
      b.mlp.push_back(bn_layer(oe + "mlp_pointnet.0", 256, kW));
    } else if (f == 1 && cfg->color_embed) {
      b.embed = true;
      b.table = get(oe + "color_embedding.weight", 0, false);
    } else {
      const std::string pre = oe + (f == 1 ? "color_encoder" : f == 2 ? "pos_encoder" : "num_encoder");
      b.mlp.push_back(bn_layer(pre + ".0", f == 3 ? 1 : 3, 64));
      b.mlp.push_back(bn_layer(pre + ".1", 64, kW));
    }
  }
  if (st->n_feat == 0) err = "fine_train_bind: use_features is empty";
  if (st->n_feat > 1) st->merge = bn_layer(oe + "mlp_merge.0", st->n_feat * kW, kW);
  if (!cfg->class_embed && !cfg->use_class) {
    st->pn_stats = true;
    st->pn_only = bn_layer(oe + "mlp_pointnet.0", 256, kW);
    st->pn_only.w.g = st->pn_only.b.g = st->pn_only.bw.g = st->pn_only.bb.g = nullptr;
  }
  auto dec = [&](const std::string& pre, bool obj, int site) {
    DecLayer L;
    L.in_w = get(pre + ".self_attn.in_proj_weight", 3 * kW * kW, false);
    L.in_b = get(pre + ".self_attn.in_proj_bias", 3 * kW, false);
    L.out_w = get(pre + ".self_attn.out_proj.weight", kW * kW, false);
    L.out_b = get(pre + ".self_attn.out_proj.bias", kW, false);
    L.cin_w = get(pre + ".multihead_attn.in_proj_weight", 3 * kW * kW, false);
    L.cin_b = get(pre + ".multihead_attn.in_proj_bias", 3 * kW, false);
    L.cout_w = get(pre + ".multihead_attn.out_proj.weight", kW * kW, false);
    L.cout_b = get(pre + ".multihead_attn.out_proj.bias", kW, false);
    L.l1_w = get(pre + ".linear1.weight", kFF * kW, false);
    L.l1_b = get(pre + ".linear1.bias", kFF, false);
    L.l2_w = get(pre + ".linear2.weight", kW * kFF, false);
    L.l2_b = get(pre + ".linear2.bias", kW, false);
    L.n1_w = get(pre + ".norm1.weight", kW, false);
    L.n1_b = get(pre + ".norm1.bias", kW, false);
    L.n2_w = get(pre + ".norm2.weight", kW, false);
    L.n2_b = get(pre + ".norm2.bias", kW, false);
    L.n3_w = get(pre + ".norm3.weight", kW, false);
    L.n3_b = get(pre + ".norm3.bias", kW, false);
    L.obj = obj;
    L.site = site;
    st->dec.push_back(L);
  };
  if (st->n_layers == 0) {
    dec("cross_hints", false, 0);
  } else {
    for (int i = 0; i < st->n_layers; ++i) {
      dec("cross_objects." + std::to_string(i), true, 6 * (2 * i));
      dec("cross_hints." + std::to_string(i), false, 6 * (2 * i + 1));
    }
  }
  st->o0w = get("mlp_offsets.0.weight", 64 * kW, false);
  st->o0b = get("mlp_offsets.0.bias", 64, false);
  st->o2w = get("mlp_offsets.2.weight", 2 * 64, false);
  st->o2b = get("mlp_offsets.2.bias", 2, false);
  if (!err.empty()) {
    free_ft(st);
    return fail(ctx, T2L_EINVAL, err);
  }
  // the backbone: bound completely (trained, or frozen: no gradient buffers) or not at all; the classifier heads are ignored
  if (int rc = pn_train_bind_group(ctx, tensors, n, "fine_train_bind", &st->pn)) {
    free_ft(st);
    return rc;
  }
  if (st->pn && cfg->class_embed) {
    free_ft(st);
    return fail(ctx, T2L_EINVAL, "fine_train_bind: object_encoder.pointnet.* is bound only with class_embed == 0 (class_embed looks the "
                                 "classes up instead of running the backbone)");
  }
  // Adam over what arrived with a gradient buffer (a name given twice counts once: the entry the step reads)
  std::vector<AdamBound> trained, backbone;
  for (int i = 0; i < n; ++i) {
    const t2l_train_tensor& x = tensors[i];
    if (!x.grad || x.numel <= 0 || by[x.name] != &x) continue;
    (strncmp(x.name, "object_encoder.pointnet.", 24) ? trained : backbone).push_back(AdamBound{x.name, x.data, x.grad, x.numel});
  }
  st->n_own = trained.size();
  trained.insert(trained.end(), backbone.begin(), backbone.end());
  st->n_adam = trained.size();
  T2L_HIP(ctx, hipDeviceSynchronize());  // the previous state's arena may still be in use
  // from here on the bind is accepted: the previous binding's moments move over (an unchanged list under "train_keep_adam_state") or go
  auto* prev = (FineTrain*)ctx->fine_train;
  if (st->n_adam) {
    bool kept = false;
    if (int rc = adam_set_make(ctx, trained, prev ? prev->adam : nullptr, &kept, &st->adam)) {
      free_ft(st);
      return rc;
    }
    if (kept) {
      st->step = prev->step;
      st->step_pn = prev->step_pn;
    }
  }
  free_fine_train(ctx);
  ctx->fine_train = st;
  return T2L_OK;
}

// the arguments of a forward (have_pn: features2 arrives, from the caller or from the backbone)
static int check_forward(t2l_ctx* ctx, const FineTrain* st, const t2l_packed_cells* in, bool have_pn, const float* hint_desc, int n_pairs,
                         int n_hints, float p, const float* out) {
  if (!in || !hint_desc || !out) return fail(ctx, T2L_EINVAL, "fine_train_forward: null input / hint_desc / out_offsets");
  if (n_pairs < 1) return fail(ctx, T2L_EINVAL, "fine_train_forward: n_pairs must be >= 1");
  if (n_hints < 1 || n_hints > kHintMax) return fail(ctx, T2L_EINVAL, "fine_train_forward: n_hints must be 1..8");
  if (in->n_cells != n_pairs || in->n_objects != n_pairs * kObj)
    return fail(ctx, T2L_EINVAL, "fine_train_forward: one padded cell of exactly 16 objects per pair");
  if (!(p >= 0.f && p < 1.f)) return fail(ctx, T2L_EINVAL, "fine_train_forward: dropout_p must be in [0, 1)");
  const Branch* b = st->br;
  if (((b[0].used && !b[0].embed) || st->pn_stats) && !have_pn)
    return fail(ctx, T2L_EINVAL, "fine_train_forward: class_embed is off: pn_feat is required");
  if (b[0].used && b[0].embed && !in->class_idx) return fail(ctx, T2L_EINVAL, "fine_train_forward: class_idx is required");
  if (b[1].used && b[1].embed && !in->color_idx) return fail(ctx, T2L_EINVAL, "fine_train_forward: color_idx is required");
  if (b[1].used && !b[1].embed && !in->rgb) return fail(ctx, T2L_EINVAL, "fine_train_forward: rgb is required");
  if (b[2].used && !in->center) return fail(ctx, T2L_EINVAL, "fine_train_forward: center is required");
  if (b[3].used && !in->n_pts) return fail(ctx, T2L_EINVAL, "fine_train_forward: n_pts is required");
  return T2L_OK;
}

int fine_train_forward_impl(t2l_ctx* ctx, const t2l_packed_cells* in, const float* pn_feat, const float* hint_desc, int n_pairs,
                            int n_hints, float p, uint32_t seed, float* out, hipStream_t s) {
  auto* st = (FineTrain*)ctx->fine_train;
  if (!st) return fail(ctx, T2L_ESTATE, "fine_train_forward: call t2l_fine_train_bind first");
  if (!pn_feat && in) pn_feat = in->pn_feat;
  if (int rc = check_forward(ctx, st, in, pn_feat != nullptr, hint_desc, n_pairs, n_hints, p, out)) return rc;
  st->have_fwd = false;
  st->pn_fwd = false;
  st->P = n_pairs;
  st->H = n_hints;
  for (auto& L : st->dec) {
    L.Tq = L.obj ? kObj : n_hints;
    L.Tk = L.obj ? n_hints : kObj;
  }
  const bool sync = ctx->sync_fn != nullptr;  // BatchNorm statistics over every rank's rows (t2l_train_sync_bn)
  ctx->sync_failed = false;
  Arena count;  // (no base: the count pass)
  plan(st, count, n_pairs, n_hints, p, sync);
  if (count.off > st->ws.cap) {
    T2L_HIP(ctx, hipStreamSynchronize(s));  // the old arena may still be read by queued work of this stream
    if (st->ws.base) (void)hipFree(st->ws.base);
    st->ws = Arena{};
    T2L_HIP(ctx, hipMalloc(&st->ws.base, count.off));
    st->ws.cap = count.off;
  }
  st->ws.off = 0;
  plan(st, st->ws, n_pairs, n_hints, p, sync);
  st->class_idx = in->class_idx;
  st->color_idx = in->color_idx;
  st->rgb = in->rgb;
  st->center = in->center;
  st->n_pts = in->n_pts;
  st->pn_feat = pn_feat;
  st->hint = hint_desc;
  const int P = n_pairs, M0 = P * kObj;
  const int ldE = st->n_feat * kW;
  bool ok = true;  // every row kernel has its instance of width 128
  // ---- ObjectEncoder (object_encoder.py:102-149) + F.normalize (cross_matcher.py:103-104)
  if (sync) {
    // the branches' MLPs side by side, one exchange per layer index: layer 0 of every MLP branch (and mlp_pointnet's statistics-only
    // run), then layer 1 of the two-layer ones
    if (st->br[3].used) hipLaunchKernelGGL(k_num_in, dim3(nblk(M0, 256)), dim3(256), 0, s, in->n_pts, M0, st->br[3].in);
    for (size_t li = 0; li < 2; ++li) {
      std::vector<BnJob> jobs;
      for (int f = 0; f < 4; ++f) {
        Branch& br = st->br[f];
        if (!br.used || br.embed || br.mlp.size() <= li) continue;
        const float* x = li > 0 ? br.mlp[li - 1].out : f == 0 ? pn_feat : f == 1 ? in->rgb : f == 2 ? in->center : br.in;
        jobs.push_back(BnJob{&br.mlp[li], x, nullptr, nullptr, nullptr});
      }
      if (li == 0 && st->pn_stats) jobs.push_back(BnJob{&st->pn_only, pn_feat, nullptr, nullptr, nullptr});
      if (!bn_stage_fwd(ctx, jobs, M0, s)) return stage_failed(ctx, "fine_train_forward");
    }
  }
  int col = 0;
  for (int f = 0; f < 4; ++f) {
    Branch& br = st->br[f];
    if (!br.used) continue;
    const float* last;
    if (sync && !br.embed) {
      last = br.mlp.back().out;
    } else if (br.embed) {
      const int32_t* idx = f == 0 ? in->class_idx : in->color_idx;
      hipLaunchKernelGGL(k_gather, dim3(nblk((int64_t)M0 * kW, 256)), dim3(256), 0, s, br.table.d, (int)(br.table.n / kW), idx, M0, br.raw);
      last = br.raw;
    } else {
      const float* x = f == 0 ? pn_feat : f == 1 ? in->rgb : f == 2 ? in->center : br.in;
      if (f == 3) hipLaunchKernelGGL(k_num_in, dim3(nblk(M0, 256)), dim3(256), 0, s, in->n_pts, M0, br.in);
      for (auto& l : br.mlp) {
        bn_layer_fwd(l, x, M0, s);
        x = l.out;
      }
      last = x;
    }
    ok = rownorm_rows(true, kW, last, nullptr, st->E + col * kW, br.nrm, M0, ldE, s) && ok;
    ++col;
  }
  if (st->pn_stats && !sync) bn_layer_fwd(st->pn_only, pn_feat, M0, s);  // running statistics only
  const float* feat = st->E;
  if (st->n_feat > 1) {
    if (!sync)
      bn_layer_fwd(st->merge, st->E, M0, s);
    else if (!bn_stage_fwd(ctx, {BnJob{&st->merge, st->E, nullptr, nullptr, nullptr}}, M0, s))
      return stage_failed(ctx, "fine_train_forward");
    feat = st->merge.out;
  }
  ok = rownorm_rows(true, kW, feat, nullptr, st->D0, st->nrm0, M0, kW, s) && ok;
  // ---- CCAT (cross_matcher.py:109-124)
  const float *obj = st->D0, *hint = hint_desc;
  for (auto& L : st->dec) {
    L.x = L.obj ? obj : hint;
    L.mem = L.obj ? hint : obj;
    ok = dec_fwd(st, L, p, seed, st->t_ds, s) && ok;
    (L.obj ? obj : hint) = L.out;
  }
  // ---- max over the hints + mlp_offsets (cross_matcher.py:126-131)
  seq_max_fwd_launch(hint, nullptr, P, n_hints, kW, st->pool, st->arg, s);
  lin_fwd(s, st->pool, kW, P, kW, st->o0w.d, kW, st->o0b.d, 64, st->a1, 64, 1);
  lin_fwd(s, st->a1, 64, P, 64, st->o2w.d, 64, st->o2b.d, 2, out, 2);
  T2L_HIP(ctx, hipGetLastError());
  if (!ok) return fail(ctx, T2L_ESTATE, "fine_train_forward: the row kernels have no instance of width 128");
  if (ctx->sync_failed) return fail(ctx, T2L_ESTATE, "fine_train_forward: the cross-rank sum callback (t2l_train_sync_bn) failed");
  st->sync = sync;
  st->have_fwd = true;
  st->p = p;
  st->seed = seed;
  return T2L_OK;
}

int fine_train_forward_points_impl(t2l_ctx* ctx, const t2l_packed_cells* in, const float* pos, const float* rgb, const float* hint_desc,
                                   int n_pairs, int n_hints, float p, uint32_t seed, float* out, hipStream_t s) {
  auto* st = (FineTrain*)ctx->fine_train;
  if (!st) return fail(ctx, T2L_ESTATE, "fine_train_forward_points: call t2l_fine_train_bind first");
  if (!st->pn)
    return fail(ctx, T2L_ESTATE, "fine_train_forward_points: the PointNet++ backbone is not bound (object_encoder.pointnet.* in "
                                 "t2l_fine_train_bind, class_embed == 0)");
  if (!pos || !rgb) return fail(ctx, T2L_EINVAL, "fine_train_forward_points: null pos / rgb");
  if (int rc = check_forward(ctx, st, in, true, hint_desc, n_pairs, n_hints, p, out)) return rc;
  st->have_fwd = false;
  st->pn_fwd = false;
  // one backbone call per cell in the reference (object_encoder.py:92-95): a cell is a pair's 16 objects
  std::vector<int32_t> offs((size_t)n_pairs + 1);
  for (int i = 0; i <= n_pairs; ++i) offs[i] = i * kObj;
  const float* f2 = nullptr;
  if (int rc = pn_train_forward_on(ctx, st->pn, "fine_train_forward_points", pos, rgb, offs.data(), n_pairs, &f2, s)) return rc;
  if (int rc = fine_train_forward_impl(ctx, in, f2, hint_desc, n_pairs, n_hints, p, seed, out, s)) return rc;
  st->pn_fwd = true;
  return T2L_OK;
}

int fine_train_backward_impl(t2l_ctx* ctx, const float* grad_offsets, float* grad_hint, float* grad_pn, hipStream_t s) {
  auto* st = (FineTrain*)ctx->fine_train;
  if (!st || !st->have_fwd) return fail(ctx, T2L_ESTATE, "fine_train_backward: no training-mode forward to differentiate");
  if (!grad_offsets) return fail(ctx, T2L_EINVAL, "fine_train_backward: null grad_offsets");
  if (st->sync && !ctx->sync_fn)
    return fail(ctx, T2L_ESTATE, "fine_train_backward: the forward summed its BatchNorm statistics over the ranks; t2l_train_sync_bn was "
                                 "turned off before its backward");
  const bool sync = st->sync;
  ctx->sync_failed = false;
  const float p = st->p;
  const uint32_t seed = st->seed;
  const int P = st->P, H = st->H, M0 = P * kObj, M1 = P * H;
  // on into the backbone: after a points forward, when it trains and features2 reaches the loss ("class" via mlp_pointnet)
  const bool pn_bwd = st->pn_fwd && pn_train_trainable(st->pn) && st->br[0].used && !st->br[0].embed;
  float* dpn = grad_pn ? grad_pn : pn_bwd ? st->dpn : nullptr;
  // head
  lin_dw(s, grad_offsets, 2, st->a1, 64, P, 2, 64, st->o2w.g, 64, st->o2b.g);
  lin_dx(s, grad_offsets, 2, P, 2, st->o2w.d, 64, 64, st->da1, 64, 0);
  relu_drop_bwd_launch(st->da1, st->a1, (size_t)P * 64, Drop{}, s);  // (no dropout: the plain ReLU backward)
  lin_dw(s, st->da1, 64, st->pool, kW, P, 64, kW, st->o0w.g, kW, st->o0b.g);
  lin_dx(s, st->da1, 64, P, 64, st->o0w.d, kW, kW, st->dpool, kW, 0);
  float *g1 = st->gA1, *g1n = st->gB1, *g0 = st->gA0, *g0n = st->gB0;
  seq_max_bwd_launch(st->dpool, st->arg, P, H, kW, g1, s);
  bool ok = true;
  T2L_HIP(ctx, hipMemsetAsync(g0, 0, (size_t)M0 * kW * sizeof(float), s));
  // CCAT, reverse cascade order
  for (int i = (int)st->dec.size() - 1; i >= 0; --i) {
    DecLayer& L = st->dec[i];
    if (L.obj) {
      ok = dec_bwd(st, L, p, seed, g0, g0n, g1, s) && ok;
      std::swap(g0, g0n);
    } else {
      ok = dec_bwd(st, L, p, seed, g1, g1n, g0, s) && ok;
      std::swap(g1, g1n);
    }
  }
  if (grad_hint) T2L_HIP(ctx, hipMemcpyAsync(grad_hint, g1, (size_t)M1 * kW * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (grad_pn && st->pn_stats)  // features2 fed the statistics only: d loss / d features2 = 0
    T2L_HIP(ctx, hipMemsetAsync(grad_pn, 0, (size_t)M0 * 256 * sizeof(float), s));
  // ObjectEncoder
  const int ldE = st->n_feat * kW;
  float* dfeat = st->n_feat > 1 ? st->ta : st->dE;
  ok = rownorm_rows(false, kW, g0, st->D0, dfeat, st->nrm0, M0, kW, s) && ok;
  if (st->n_feat > 1) {
    if (!sync)
      bn_layer_bwd(st->merge, st->ta, M0, st->tb, st->dE, s);
    else if (!bn_stage_bwd(ctx, {BnJob{&st->merge, nullptr, st->ta, st->tb, st->dE}}, M0, s))
      return stage_failed(ctx, "fine_train_backward");
  }
  int col = 0;
  for (int f = 0; f < 4; ++f) {
    Branch& br = st->br[f];
    if (!br.used) continue;
    float* draw = br.embed ? st->ta : sync ? br.s_draw : st->gA0;  // d of the branch output before its F.normalize
    ok = rownorm_rows(false, kW, st->dE + col * kW, st->E + col * kW, draw, br.nrm, M0, ldE, s) && ok;
    if (br.embed) {
      if (br.table.g)
        hipLaunchKernelGGL(k_scatter_add, dim3(nblk((int64_t)M0 * kW, 256)), dim3(256), 0, s, st->ta, (int)(br.table.n / kW),
                           f == 0 ? st->class_idx : st->color_idx, M0, br.table.g);
    } else if (!sync) {
      // layers in reverse: dout in gA0 / gB0 alternately, dy in ta, dx of the first layer only for features2
      float *dout = st->gA0, *dnext = st->gB0;
      for (int li = (int)br.mlp.size() - 1; li >= 0; --li) {
        float* dx = li > 0 ? dnext : (f == 0 ? dpn : nullptr);
        bn_layer_bwd(br.mlp[li], dout, M0, st->ta, dx, s);
        std::swap(dout, dnext);
      }
    }
    ++col;
  }
  if (sync) {
    // the MLP branches side by side, in reverse: layer 1 of the two-layer ones (d hidden into s_d0), then every layer 0 (d features2
    // of mlp_pointnet into dpn)
    for (int li = 1; li >= 0; --li) {
      std::vector<BnJob> jobs;
      for (int f = 0; f < 4; ++f) {
        Branch& br = st->br[f];
        if (!br.used || br.embed || (int)br.mlp.size() <= li) continue;
        const bool last = li + 1 == (int)br.mlp.size();
        jobs.push_back(BnJob{&br.mlp[li], nullptr, last ? br.s_draw : br.s_d0, last ? br.s_dy : br.s_dy0,
                             li > 0 ? br.s_d0 : (f == 0 ? dpn : nullptr)});
      }
      if (!bn_stage_bwd(ctx, jobs, M0, s)) return stage_failed(ctx, "fine_train_backward");
    }
  }
  T2L_HIP(ctx, hipGetLastError());
  if (!ok) return fail(ctx, T2L_ESTATE, "fine_train_backward: the row kernels have no instance of width 128");
  if (ctx->sync_failed) return fail(ctx, T2L_ESTATE, "fine_train_backward: the cross-rank sum callback (t2l_train_sync_bn) failed");
  if (pn_bwd) {
    st->pn_touched = true;  // the backbone's gradients carry this batch: its tensors take part in the next t2l_fine_adam_step
    return pn_train_backward_on(ctx, st->pn, "fine_train_backward", dpn, s);
  }
  return T2L_OK;
}

// ---- the optimizer (training/fine.py:57 optimizer.zero_grad(), :72 optimizer.step(), :229 optim.Adam(model.parameters(), lr)): train.hip's
// adam_kernel / zero_kernel over this binding's tensors
int fine_adam_step_impl(t2l_ctx* ctx, float lr, float b1, float b2, float eps, hipStream_t s) {
  auto* st = (FineTrain*)ctx->fine_train;
  if (!st) return fail(ctx, T2L_ESTATE, "t2l_fine_adam_step: call t2l_fine_train_bind first");
  st->step += 1;
  const bool pn = st->n_own < st->n_adam && st->pn_touched;
  if (pn) st->step_pn += 1;
  if (!st->adam) return T2L_OK;
  event_begin(ctx, "fine_adam_step", s);
  if (pn && st->step_pn == st->step) {  // one launch: both groups at the same bias correction (every step went through the backbone)
    adam_set_step(st->adam, 0, st->n_adam, st->step, lr, b1, b2, eps, s);
  } else {
    adam_set_step(st->adam, 0, st->n_own, st->step, lr, b1, b2, eps, s);
    if (pn) adam_set_step(st->adam, st->n_own, st->n_adam, st->step_pn, lr, b1, b2, eps, s);
  }
  event_end(ctx, "fine_adam_step", s);
  T2L_HIP(ctx, hipGetLastError());
  return T2L_OK;
}

int fine_zero_grad_impl(t2l_ctx* ctx, hipStream_t s) {
  auto* st = (FineTrain*)ctx->fine_train;
  if (!st) return fail(ctx, T2L_ESTATE, "t2l_fine_zero_grad: call t2l_fine_train_bind first");
  if (st->adam) adam_set_zero(st->adam, s);
  st->pn_touched = false;
  T2L_HIP(ctx, hipGetLastError());
  return T2L_OK;
}

int fine_adam_state_impl(t2l_ctx* ctx, int set, float* m, float* v, int64_t* step, int64_t* numel, hipStream_t s) {
  auto* st = (FineTrain*)ctx->fine_train;
  if (!st) return fail(ctx, T2L_ESTATE, "t2l_fine_adam_state: call t2l_fine_train_bind first");
  const int64_t packed = st->step | (st->step_pn << 32);
  if (!st->adam) {  // nothing is trained: no moments to move
    if (numel) *numel = 0;
    if (step && !set) *step = packed;
    return T2L_OK;
  }
  const int rc = adam_set_state(ctx, st->adam, "t2l_fine_adam_state", set, m, v, step, numel, packed, s);
  if (rc == T2L_OK && set && m) {
    st->step = *step & 0xFFFFFFFFll;
    st->step_pn = st->n_own < st->n_adam ? (*step >> 32) : 0;
  }
  return rc;
}

}  // namespace t2l
