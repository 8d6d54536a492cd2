// Symmetric InfoNCE of training/losses.py:255-283 (ContrastiveLoss), forward + analytic backward, as ONE
// launch of 4 * ceil(B / 32) workgroups (the op is latency bound: 2*B^2*D = 2.1 MFLOP at B = 64).
//
//   ia_i = 1/|im_i|, ip_j = 1/|s_j|                                   losses.py:271-272
//   sim  = (im @ s^T) * ia_i * ip_j            f32 MFMA 32x32x2      :274
//   E    = exp(sim / T); R_i = sum_j E_ij; C_j = sum_i E_ij           :277-278 (no max-subtraction, as the reference)
//   loss = mean_i( log C_i + log R_i - 2 sim_ii / T )                 == :280-281
//   G    = dloss/dsim = (E_ij/C_j + E_ij/R_i - 2 delta_ij) / (T B)
//   d im = ((G  @ s^) - im^ * rowdot) * ia ;  d s = ((G^T @ im^) - s^ * rowdot) * ip     (x^ = x/|x|)
//
// E/G lives in LDS ([Bp][Bp+1] f32, Bp = B rounded up to 32, B <= 128); operands stream from L2.
//
// The pairwise and hardest ranking losses of training/losses.py:192-217 and :321-355 (t2l_ranking_loss) follow further down: the same
// similarity tiles (sim_tiles_lds, sim_tile) and gradient products (grad_tile_lds, grad_rowblock), another G.
#include "t2l_internal.h"

namespace t2l {

typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int CTRL>
__device__ __forceinline__ float loss_dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float wave_sum_f32(float v) {  // all-reduce over the 64 lanes on the VALU
  v += loss_dpp<0xB1>(v);
  v += loss_dpp<0x4E>(v);
  v += loss_dpp<0x141>(v);
  v += loss_dpp<0x140>(v);
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
__device__ __forceinline__ float half_sum(float v) {  // sum over the 32 lanes that share lane>>5 (DPP, no LDS traffic)
  v += loss_dpp<0xB1>(v);
  v += loss_dpp<0x4E>(v);
  v += loss_dpp<0x141>(v);
  v += loss_dpp<0x140>(v);
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// One 32-row block of  out = ((M @ X^) - Y^ * rowdot) * iy   where M is G (transpose=false) or G^T.
// X^ = x * ix (rows k), Y^ = y * iy (rows i). Result rows i0..i0+31, all 256 columns, one wave.
__device__ __forceinline__ void grad_rowblock(const float* __restrict__ G, int ldg, bool transpose, int B, int i0,
                                              const float* __restrict__ x, const float* __restrict__ ix,
                                              const float* __restrict__ y, const float* __restrict__ iy,
                                              float* __restrict__ out, int lane) {
  const int col = lane & 31, half = lane >> 5;
  f32x16 acc[8];
#pragma unroll
  for (int t = 0; t < 8; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  // A-operand row of this lane, clamped like every other row here: in a ragged last block the rows past B - 1 are computed and thrown
  // away, and unclamped they read G up to 31 rows past its end — at B = 129 13 KB past the end of the whole workspace
  const int gi = min(i0 + col, B - 1);
#pragma unroll 8  // the operands of 8 steps in flight: every step's loads come from L2 and nothing else hides their latency
  for (int k0 = 0; k0 < B; k0 += 2) {
    const int k = k0 + half;
    float a = 0.f, scale = 0.f;
    if (k < B) {
      a = transpose ? G[k * ldg + gi] : G[gi * ldg + k];
      scale = ix[k];
    }
    const float* xr = x + (size_t)min(k, B - 1) * kD + col;
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, xr[32 * t] * scale, acc[t], 0, 0, 0);
  }
  // lane holds column 32*t + col, rows i0 + (r&3) + 8*(r>>2) + 4*half.
  // The y rows of the NEXT four accumulator rows are loaded before the current four are stored (double-buffered registers, full
  // blocks store without a branch): written row by row — 8 loads, a reduction, 8 guarded stores — every row's loads queued behind
  // the previous row's stores (s_waitcnt vmcnt(7) x 8 per row: 16 store-drain + load round trips, ~20 of the kernel's 44 us).
  const bool full = i0 + 32 <= B;
  float yb[2][4][8], ib[2][4];
  auto load_rows = [&](int b4, float (&yy)[4][8], float (&ii)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = 4 * b4 + q;
      const int row = min(i0 + (r & 3) + 8 * (r >> 2) + 4 * half, B - 1);
      ii[q] = iy[row];
      const float* yr = y + (size_t)row * kD + col;
#pragma unroll
      for (int t = 0; t < 8; ++t) yy[q][t] = yr[32 * t];
    }
  };
  load_rows(0, yb[0], ib[0]);
#pragma unroll
  for (int b4 = 0; b4 < 4; ++b4) {
    if (b4 + 1 < 4) load_rows(b4 + 1, yb[(b4 + 1) & 1], ib[(b4 + 1) & 1]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = 4 * b4 + q;
      const int row = i0 + (r & 3) + 8 * (r >> 2) + 4 * half;
      const float inv = row < B ? ib[b4 & 1][q] : 0.f;
      float yv[8];
      float part = 0.f;
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        yv[t] = yb[b4 & 1][q][t] * inv;
        part += acc[t][r] * yv[t];
      }
      const float dot = half_sum(part);
      float* orow = out + (size_t)min(row, B - 1) * kD + col;
      if (full) {
#pragma unroll
        for (int t = 0; t < 8; ++t) orow[32 * t] = (acc[t][r] - yv[t] * dot) * inv;
      } else if (row < B) {
#pragma unroll
        for (int t = 0; t < 8; ++t) orow[32 * t] = (acc[t][r] - yv[t] * dot) * inv;
      }
    }
  }
}

// Stage 1 of the fused kernels (contrastive_tiles_kernel, ranking_tiles_kernel): the raw dot products of every 32 x 32 tile into
// S[Bp][ldg] and the inverse norms into ia / ip (0 beyond B), tiles dealt over the workgroup's 4 waves. The caller synchronises.
__device__ __forceinline__ void sim_tiles_lds(const float* im, const float* s, int B, int nb, int ldg,
                                              float* S, float* ia, float* ip, int wave, int col, int half) {
  // 1. raw similarity tiles; a lane streams half a row of each operand, so the squared norms come with them
  for (int tile = wave; tile < nb * nb; tile += 4) {
    const int i0 = (tile / nb) * 32, j0 = (tile % nb) * 32;
    const float4* ap = reinterpret_cast<const float4*>(im + (size_t)min(i0 + col, B - 1) * kD + half * 128);
    const float4* pp = reinterpret_cast<const float4*>(s + (size_t)min(j0 + col, B - 1) * kD + half * 128);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float na = 0.f, np = 0.f;
#pragma unroll 16
    for (int q = 0; q < 32; ++q) {
      const float4 a = ap[q], p = pp[q];
      na += a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w;
      np += p.x * p.x + p.y * p.y + p.z * p.z + p.w * p.w;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, p.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, p.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, p.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, p.w, acc, 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);  // (MFMA -> VALU read behind a loop exit: see gemm_rows2.h)
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    na += __shfl_xor(na, 32);
    np += __shfl_xor(np, 32);
    if (half == 0) {
      if (j0 == 0) ia[i0 + col] = i0 + col < B ? 1.f / sqrtf(na) : 0.f;
      if (i0 == 0) ip[j0 + col] = j0 + col < B ? 1.f / sqrtf(np) : 0.f;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) S[(i0 + (r & 3) + 8 * (r >> 2) + 4 * half) * ldg + j0 + col] = acc[r];
  }
}

// Stage 4 of the fused kernels: from G (in E, zero beyond B), the inverse norms and the two rowdot vectors in LDS,
//   rowdot_i = sum_k G_ik * cos_ik   (and sum_k G_ki * cos_ki for d s),
// whatever loss G is the derivative of.
__device__ __forceinline__ void grad_tile_lds(const float* im, const float* s, int B, int Bp, int nb, int ldg,
                                              const float* E, const float* ia, const float* ip, const float* rdA, const float* rdP,
                                              float* g_im, float* g_s, int wave, int col, int half) {
  // 4. one 32 x 32 tile of d im (mat 0) or d s (mat 1) per wave:  out = ((M @ X^) - Y^ * rowdot) * iy
  const int task = blockIdx.x * 4 + wave;
  if (task >= 2 * nb * 8) return;
  const int mat = task / (nb * 8), i0 = (task % (nb * 8)) / 8 * 32, c0 = (task % 8) * 32;
  const float* x = mat ? im : s;
  const float* ix = mat ? ia : ip;
  const float* y = mat ? s : im;
  const float* iy = mat ? ip : ia;
  const float* rd = mat ? rdP : rdA;
  float* out = mat ? g_s : g_im;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const int gi = i0 + col;
  for (int k0 = 0; k0 < Bp; k0 += 32) {  // 16 steps per round, their operand loads all in flight
    float xv[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) xv[q] = x[(size_t)min(k0 + 2 * q + half, B - 1) * kD + c0 + col];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int k = k0 + 2 * q + half;
      const float a = mat ? E[k * ldg + gi] : E[gi * ldg + k];  // zero beyond B (E is), so the clamped x rows do not count
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, xv[q] * ix[k], acc, 0, 0, 0);
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  float yv[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) yv[r] = y[(size_t)min(i0 + (r & 3) + 8 * (r >> 2) + 4 * half, B - 1) * kD + c0 + col];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = i0 + (r & 3) + 8 * (r >> 2) + 4 * half;
    const float inv = iy[row];
    const float v = (acc[r] - yv[r] * inv * rd[row]) * inv;
    if (row < B) out[(size_t)row * kD + c0 + col] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// The loss as 4*nb workgroups. (Rounds 1-2 ran ONE workgroup — 38.6 us per call at batch 64 against 22.4 us; removed in round 5.) The single workgroup spent half its time
// in the two gradient products — 2*nb row blocks of 8 column tiles on 4 waves — and a quarter in load round trips ahead of the
// similarity tiles. Here EVERY workgroup repeats the cheap part (similarity tiles, E, row / column sums, G: B^2 work, in its own LDS;
// the inverse norms fall out of the operand loads of the similarity tiles, there is no norm pass), and the gradients' 2*nb*8 output
// tiles are dealt one per WAVE over the whole grid: the correction term of the normalisation's backward,
//   rowdot_i = sum_c (G @ s^)_ic * im^_ic = sum_k G_ik * cos_ik        (and sum_k G_ki * cos_ki for d s),
// comes from the B x B matrices in LDS, so a tile needs nothing from its row's other tiles. Workgroup 0 writes the loss.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 1) void contrastive_tiles_kernel(const float* __restrict__ im, const float* __restrict__ s, int B,
                                                                   float inv_t, float* __restrict__ loss, float* __restrict__ g_im,
                                                                   float* __restrict__ g_s) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int Bp = (B + 31) / 32 * 32;
  const int ldg = Bp + 1;
  float* E = smem;               // [Bp][ldg]  E, then G
  float* S = E + Bp * ldg;       // [Bp][ldg]  raw dot products, then cosines
  float* ia = S + Bp * ldg;      // [Bp]
  float* ip = ia + Bp;           // [Bp]
  float* R = ip + Bp;            // [Bp]
  float* C = R + Bp;             // [Bp]
  float* rdA = C + Bp;           // [Bp]  rowdot of d im
  float* rdP = rdA + Bp;         // [Bp]  rowdot of d s
  float* part = rdP + Bp;        // [4][Bp] per-wave column partials
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 31, half = lane >> 5;
  const int nb = Bp / 32;

  sim_tiles_lds(im, s, B, nb, ldg, S, ia, ip, wave, col, half);
  __syncthreads();

  // 2. cosines, E, row sums (wave reduction) and per-wave column partials; columns j = lane, lane + 64
  {
    float c0 = 0.f, c1 = 0.f;
    const float p0 = ip[min(lane, Bp - 1)], p1 = lane + 64 < Bp ? ip[lane + 64] : 0.f;
    for (int i = wave; i < Bp; i += 4) {
      const float a = ia[i];
      float e0 = 0.f, e1 = 0.f;
      if (lane < Bp) {
        const float c = S[i * ldg + lane] * a * p0;
        S[i * ldg + lane] = c;
        e0 = (i < B && lane < B) ? __expf(c * inv_t) : 0.f;
        E[i * ldg + lane] = e0;
      }
      if (lane + 64 < Bp) {
        const float c = S[i * ldg + lane + 64] * a * p1;
        S[i * ldg + lane + 64] = c;
        e1 = (i < B && lane + 64 < B) ? __expf(c * inv_t) : 0.f;
        E[i * ldg + lane + 64] = e1;
      }
      c0 += e0;
      c1 += e1;
      const float r = wave_sum_f32(e0 + e1);
      if (lane == 0) R[i] = r;
    }
    if (lane < Bp) part[wave * Bp + lane] = c0;
    if (lane + 64 < Bp) part[wave * Bp + lane + 64] = c1;
  }
  __syncthreads();
  if (tid < Bp) C[tid] = part[tid] + part[Bp + tid] + part[2 * Bp + tid] + part[3 * Bp + tid];
  __syncthreads();
  if (blockIdx.x == 0 && wave == 0) {
    float v = 0.f;
    for (int i = lane; i < B; i += 64) v += __logf(C[i]) + __logf(R[i]) - 2.f * S[i * ldg + i] * inv_t;
    v = wave_sum_f32(v);
    if (lane == 0) loss[0] = v / (float)B;
  }
  if (!g_im) return;

  // 3. G in place of E, and the two rowdot vectors
  {
    const float sc = inv_t / (float)B;
    float d0 = 0.f, d1 = 0.f;
    const float ic0 = lane < B ? 1.f / C[lane] : 0.f, ic1 = lane + 64 < B ? 1.f / C[lane + 64] : 0.f;
    for (int i = wave; i < Bp; i += 4) {
      const float ir = i < B ? 1.f / R[i] : 0.f;
      float t0 = 0.f, t1 = 0.f;
      if (lane < Bp) {
        const float v = E[i * ldg + lane];
        const float g = (v * ic0 + v * ir - ((i == lane && i < B) ? 2.f : 0.f)) * sc;
        E[i * ldg + lane] = g;
        t0 = g * S[i * ldg + lane];
      }
      if (lane + 64 < Bp) {
        const float v = E[i * ldg + lane + 64];
        const float g = (v * ic1 + v * ir - ((i == lane + 64 && i < B) ? 2.f : 0.f)) * sc;
        E[i * ldg + lane + 64] = g;
        t1 = g * S[i * ldg + lane + 64];
      }
      d0 += t0;
      d1 += t1;
      const float r = wave_sum_f32(t0 + t1);
      if (lane == 0) rdA[i] = r;
    }
    if (lane < Bp) part[wave * Bp + lane] = d0;
    if (lane + 64 < Bp) part[wave * Bp + lane + 64] = d1;
  }
  __syncthreads();
  if (tid < Bp) rdP[tid] = part[tid] + part[Bp + tid] + part[2 * Bp + tid] + part[3 * Bp + tid];
  __syncthreads();

  grad_tile_lds(im, s, B, Bp, nb, ldg, E, ia, ip, rdA, rdP, g_im, g_s, wave, col, half);
}

// ---------------------------------------------------------------------------------------------------------------
// Batches beyond the fused kernel's 128 rows — the GLOBAL contrastive matrix of data-parallel training (SURVEY.md §8e:
// every rank all-gathers the [B,256] embeddings of all ranks and evaluates the loss of the whole W*B batch; 8 x 64 = 512,
// up to 1,024 rows): the same arithmetic as a short chain of launches over a [B][B] matrix in HBM (4 MB at B = 1,024).
// Deterministic (no atomics): row / column sums are one wave per index.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cl_norm_kernel(const float* __restrict__ im, const float* __restrict__ s, int B,
                                                      float* __restrict__ ia, float* __restrict__ ip) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= B) return;
  const float4 a = reinterpret_cast<const float4*>(im + (size_t)i * kD)[lane];
  const float4 p = reinterpret_cast<const float4*>(s + (size_t)i * kD)[lane];
  const float sa = wave_sum_f32(a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w);
  const float sp = wave_sum_f32(p.x * p.x + p.y * p.y + p.z * p.z + p.w * p.w);
  if (lane == 0) { ia[i] = 1.f / sqrtf(sa); ip[i] = 1.f / sqrtf(sp); }
}

// One 32 x 32 tile of raw dot products im_i . s_j (rows clamped to B - 1), one wave: the chain's similarity launches.
__device__ __forceinline__ f32x16 sim_tile(const float* im, const float* s, int B, int i0, int j0, int col,
                                           int half) {
  const float4* ap = reinterpret_cast<const float4*>(im + (size_t)min(i0 + col, B - 1) * kD + half * 128);
  const float4* pp = reinterpret_cast<const float4*>(s + (size_t)min(j0 + col, B - 1) * kD + half * 128);
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll 8
  for (int q = 0; q < 32; ++q) {
    const float4 a = ap[q], p = pp[q];
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, p.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, p.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, p.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, p.w, acc, 0, 0, 0);
  }
  return acc;
}

__global__ __launch_bounds__(64) void cl_sim_kernel(const float* __restrict__ im, const float* __restrict__ s, int B, int nb,
                                                    float inv_t, const float* __restrict__ ia, const float* __restrict__ ip,
                                                    float* __restrict__ E, float* __restrict__ diag) {
  const int lane = threadIdx.x, col = lane & 31, half = lane >> 5;
  const int i0 = (blockIdx.x / nb) * 32, j0 = (blockIdx.x % nb) * 32;
  const f32x16 acc = sim_tile(im, s, B, i0, j0, col, half);
  const int j = j0 + col;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = i0 + (r & 3) + 8 * (r >> 2) + 4 * half;
    if (i < B && j < B) {
      const float sim = acc[r] * ia[i] * ip[j];
      E[(size_t)i * B + j] = __expf(sim * inv_t);
      if (i == j) diag[i] = sim;
    }
  }
}

__global__ __launch_bounds__(256) void cl_sums_kernel(const float* __restrict__ E, int B, float* __restrict__ R, float* __restrict__ C) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= B) return;
  float r = 0.f, c = 0.f;
  for (int j = lane; j < B; j += 64) {
    r += E[(size_t)i * B + j];
    c += E[(size_t)j * B + i];
  }
  r = wave_sum_f32(r);
  c = wave_sum_f32(c);
  if (lane == 0) { R[i] = r; C[i] = c; }
}

__global__ __launch_bounds__(256) void cl_loss_kernel(const float* __restrict__ R, const float* __restrict__ C,
                                                      const float* __restrict__ diag, int B, float inv_t, float* __restrict__ loss) {
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float v = 0.f;
  for (int i = tid; i < B; i += 256) v += __logf(C[i]) + __logf(R[i]) - 2.f * diag[i] * inv_t;
  v = wave_sum_f32(v);
  if (lane == 0) red[wave] = v;
  __syncthreads();
  if (tid == 0) loss[0] = (red[0] + red[1] + red[2] + red[3]) / (float)B;
}

__global__ __launch_bounds__(256) void cl_g_kernel(float* __restrict__ E, const float* __restrict__ R, const float* __restrict__ C,
                                                   int B, float sc) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)B * B) return;
  const int i = (int)(e / B), j = (int)(e % B);
  const float v = E[e];
  E[e] = (v / C[j] + v / R[i] - (i == j ? 2.f : 0.f)) * sc;
}

__global__ __launch_bounds__(64) void cl_grad_kernel(const float* __restrict__ G, int B, int nb, const float* __restrict__ im,
                                                     const float* __restrict__ s, const float* __restrict__ ia,
                                                     const float* __restrict__ ip, float* __restrict__ g_im, float* __restrict__ g_s) {
  const int task = blockIdx.x, i0 = (task % nb) * 32;
  if (task < nb)
    grad_rowblock(G, B, false, B, i0, s, ip, im, ia, g_im, threadIdx.x);
  else
    grad_rowblock(G, B, true, B, i0, im, ia, s, ip, g_s, threadIdx.x);
}

// ---------------------------------------------------------------------------------------------------------------
// The in-batch hinge losses of --ranking_loss pairwise | hardest (training/losses.py:192-217 and :321-355), forward + analytic
// backward. c = im^ . s^T, d_i = c_ii, m the margin, sc = scale / B:
//   hA_ij = m - d_i + c_ij (text i against the other cells), hB_ij = m - d_j + c_ij (cell j against the other texts), i != j
//   pairwise  A_ij = [hA_ij > 0],               Bm_ij = [hB_ij > 0]
//   hardest   A_ij = [j == j1_i][hA_ij > 0],    Bm_ij = [j == j2_i][hB_ij > 0],  j1_i = argmax_j c_ij, j2_i = argmax_j (c_ij - d_j):
//             BOTH maxima run along the row, as the reference's do; the lowest column wins a tie (torch's CPU rule)
//   loss = sc * sum_ij (A_ij hA_ij + Bm_ij hB_ij);  G_ij = sc (A_ij + Bm_ij),  G_ii = -sc (sum_j A_ij + sum_k Bm_ki)
// Only the selection of A and Bm differs between the two (rank_select); the similarity tiles and the gradient products are the
// contrastive loss's. The diagonal is an integer count times sc and every sum has a fixed order: no atomics, same bits every run.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float rank_hinge(float m, float d, float c) { return (m - d) + c; }

__device__ __forceinline__ void argmax_take(float& v, int& j, float ov, int oj) {
  if (ov > v || (ov == v && oj < j)) {
    v = ov;
    j = oj;
  }
}
template <int CTRL>
__device__ __forceinline__ void argmax_dpp(float& v, int& j) {
  argmax_take(v, j, loss_dpp<CTRL>(v), __builtin_amdgcn_update_dpp(0, j, CTRL, 0xF, 0xF, true));
}
// All lanes end with the largest v and, among equals, the lowest j: the butterfly of wave_sum_f32 (the choice is symmetric, so both
// lanes of a pair keep the same winner) — on the VALU, where 12 dependent ds_bpermute round trips per row cost the hardest kernel
// 33 us at 128 rows.
__device__ __forceinline__ void wave_argmax(float& v, int& j) {
  argmax_dpp<0xB1>(v, j);
  argmax_dpp<0x4E>(v, j);
  argmax_dpp<0x141>(v, j);
  argmax_dpp<0x140>(v, j);
  {
    const auto rv = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    const auto rj = __builtin_amdgcn_permlane16_swap((unsigned)j, (unsigned)j, false, false);
    v = __uint_as_float(rv[0]);
    j = (int)rj[0];
    argmax_take(v, j, __uint_as_float(rv[1]), (int)rj[1]);
  }
  {
    const auto rv = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    const auto rj = __builtin_amdgcn_permlane32_swap((unsigned)j, (unsigned)j, false, false);
    v = __uint_as_float(rv[0]);
    j = (int)rj[0];
    argmax_take(v, j, __uint_as_float(rv[1]), (int)rj[1]);
  }
}

struct RankArg {  // a lane's running arg-max candidates of one row (hardest only)
  float b1 = -INFINITY, b2 = -INFINITY;
  int j1 = 0x7fffffff, j2 = 0x7fffffff;
  __device__ __forceinline__ void offer(bool ok, float c, float dj, int j) {  // columns are offered in ascending order
    if (ok && c > b1) { b1 = c; j1 = j; }
    if (ok && c - dj > b2) { b2 = c - dj; j2 = j; }
  }
  __device__ __forceinline__ void reduce() {
    wave_argmax(b1, j1);
    wave_argmax(b2, j2);
  }
};

template <int KIND>
__device__ __forceinline__ void rank_select(bool ok, float c, float di, float dj, float m, int j, const RankArg& arg, bool& A,
                                            bool& Bm, float& hA, float& hB) {
  hA = rank_hinge(m, di, c);
  hB = rank_hinge(m, dj, c);
  A = ok && hA > 0.f && (KIND == T2L_RANK_PAIRWISE || j == arg.j1);
  Bm = ok && hB > 0.f && (KIND == T2L_RANK_PAIRWISE || j == arg.j2);
}

// B <= 128: one launch, the layout and the grid of contrastive_tiles_kernel; stages 2-3 are one pass over the cosines.
template <int KIND>
__global__ __launch_bounds__(256, 1) void ranking_tiles_kernel(const float* __restrict__ im, const float* __restrict__ s, int B,
                                                               float margin, float sc, float* __restrict__ loss,
                                                               float* __restrict__ g_im, float* __restrict__ g_s) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int Bp = (B + 31) / 32 * 32;
  const int ldg = Bp + 1;
  float* E = smem;               // [Bp][ldg]  G
  float* S = E + Bp * ldg;       // [Bp][ldg]  raw dot products, then cosines
  float* ia = S + Bp * ldg;      // [Bp]
  float* ip = ia + Bp;           // [Bp]
  float* D = ip + Bp;            // [Bp]  d_i
  float* nA = D + Bp;            // [Bp]  sum_j A_ij
  float* rdA = nA + Bp;          // [Bp]  rowdot of d im
  float* rdP = rdA + Bp;         // [Bp]  rowdot of d s
  float* part = rdP + Bp;        // [4][Bp] per-wave column partials of G * c
  float* npart = part + 4 * Bp;  // [4][Bp] per-wave column partials of Bm
  float* lpart = npart + 4 * Bp; // [4]     per-wave partials of the loss
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 31, half = lane >> 5;
  const int nb = Bp / 32;

  sim_tiles_lds(im, s, B, nb, ldg, S, ia, ip, wave, col, half);
  __syncthreads();
  if (tid < Bp) D[tid] = S[tid * ldg + tid] * ia[tid] * ip[tid];  // the product order of the cosines below: d_i IS c_ii
  __syncthreads();

  // 2-3. cosines, the selected hinges, G off the diagonal, row sums (wave reduction) and per-wave column partials; j = lane, lane + 64
  {
    const int ja = lane, jb = lane + 64;
    const float p0 = ip[min(ja, Bp - 1)], p1 = jb < Bp ? ip[jb] : 0.f;
    const float dj0 = D[min(ja, Bp - 1)], dj1 = jb < Bp ? D[jb] : 0.f;
    float l = 0.f, t0s = 0.f, t1s = 0.f, n0s = 0.f, n1s = 0.f;
    for (int i = wave; i < Bp; i += 4) {
      const float a = ia[i], di = D[i];
      float c0 = 0.f, c1 = 0.f;
      if (ja < Bp) {
        c0 = S[i * ldg + ja] * a * p0;
        S[i * ldg + ja] = c0;
      }
      if (jb < Bp) {
        c1 = S[i * ldg + jb] * a * p1;
        S[i * ldg + jb] = c1;
      }
      const bool ok0 = i < B && ja < B && ja != i, ok1 = i < B && jb < B && jb != i;
      RankArg arg;
      if (KIND == T2L_RANK_HARDEST) {
        arg.offer(ok0, c0, dj0, ja);
        arg.offer(ok1, c1, dj1, jb);
        arg.reduce();
      }
      bool A0, B0, A1, B1;
      float hA0, hB0, hA1, hB1;
      rank_select<KIND>(ok0, c0, di, dj0, margin, ja, arg, A0, B0, hA0, hB0);
      rank_select<KIND>(ok1, c1, di, dj1, margin, jb, arg, A1, B1, hA1, hB1);
      l += ((A0 ? hA0 : 0.f) + (B0 ? hB0 : 0.f)) + ((A1 ? hA1 : 0.f) + (B1 ? hB1 : 0.f));
      const float g0 = ((A0 ? 1.f : 0.f) + (B0 ? 1.f : 0.f)) * sc, g1 = ((A1 ? 1.f : 0.f) + (B1 ? 1.f : 0.f)) * sc;
      if (ja < Bp) E[i * ldg + ja] = g0;  // zero wherever i or j >= B, and on the diagonal until the counts are known
      if (jb < Bp) E[i * ldg + jb] = g1;
      const float t0 = g0 * c0, t1 = g1 * c1;
      t0s += t0;
      t1s += t1;
      n0s += B0 ? 1.f : 0.f;
      n1s += B1 ? 1.f : 0.f;
      const float r = wave_sum_f32(t0 + t1);
      const float n = wave_sum_f32((A0 ? 1.f : 0.f) + (A1 ? 1.f : 0.f));  // a count: exact in any order
      if (lane == 0) {
        rdA[i] = r;
        nA[i] = n;
      }
    }
    if (ja < Bp) {
      part[wave * Bp + ja] = t0s;
      npart[wave * Bp + ja] = n0s;
    }
    if (jb < Bp) {
      part[wave * Bp + jb] = t1s;
      npart[wave * Bp + jb] = n1s;
    }
    l = wave_sum_f32(l);
    if (lane == 0) lpart[wave] = l;
  }
  __syncthreads();
  if (blockIdx.x == 0 && tid == 0) loss[0] = ((lpart[0] + lpart[1]) + (lpart[2] + lpart[3])) * sc;
  if (!g_im) return;

  // the diagonal of G from the two counts, and its share of both rowdot vectors
  if (tid < Bp) {
    const float n = nA[tid] + ((npart[tid] + npart[Bp + tid]) + (npart[2 * Bp + tid] + npart[3 * Bp + tid]));
    const float gd = n > 0.f ? -sc * n : 0.f;
    const float d = D[tid];
    E[tid * ldg + tid] = gd;
    rdA[tid] = rdA[tid] + gd * d;
    rdP[tid] = ((part[tid] + part[Bp + tid]) + (part[2 * Bp + tid] + part[3 * Bp + tid])) + gd * d;
  }
  __syncthreads();

  grad_tile_lds(im, s, B, Bp, nb, ldg, E, ia, ip, rdA, rdP, g_im, g_s, wave, col, half);
}

// 128 < B <= 1024: the chain. cl_norm_kernel, then the cosines of every tile into Cm[B][B] and d into diag ...
__global__ __launch_bounds__(64) void rl_sim_kernel(const float* __restrict__ im, const float* __restrict__ s, int B, int nb,
                                                    const float* __restrict__ ia, const float* __restrict__ ip,
                                                    float* __restrict__ Cm, float* __restrict__ diag) {
  const int lane = threadIdx.x, col = lane & 31, half = lane >> 5;
  const int i0 = (blockIdx.x / nb) * 32, j0 = (blockIdx.x % nb) * 32;
  const f32x16 acc = sim_tile(im, s, B, i0, j0, col, half);
  const int j = j0 + col;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = i0 + (r & 3) + 8 * (r >> 2) + 4 * half;
    if (i < B && j < B) {
      const float c = acc[r] * ia[i] * ip[j];
      Cm[(size_t)i * B + j] = c;
      if (i == j) diag[i] = c;
    }
  }
}

// ... one wave per row i: the row's selection, its share of the loss, sum_j A_ij, G off the diagonal (G null: forward only), and for
// hardest the column j2 that counts against cell j2's diagonal (-1: row i violates nothing there) ...
template <int KIND>
__global__ __launch_bounds__(256) void rl_rows_kernel(const float* __restrict__ Cm, const float* __restrict__ diag, int B, float margin,
                                                      float sc, float* __restrict__ G, float* __restrict__ nA,
                                                      float* __restrict__ lrow, int* __restrict__ sel2) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= B) return;
  const float* crow = Cm + (size_t)i * B;
  const float di = diag[i];
  RankArg arg;
  if (KIND == T2L_RANK_HARDEST) {
    for (int j = lane; j < B; j += 64) arg.offer(j != i, crow[j], diag[j], j);
    arg.reduce();
  }
  float l = 0.f, n = 0.f;
  bool any2 = false;
  for (int j = lane; j < B; j += 64) {
    const float c = crow[j];
    bool A, Bm;
    float hA, hB;
    rank_select<KIND>(j != i, c, di, diag[j], margin, j, arg, A, Bm, hA, hB);
    l += (A ? hA : 0.f) + (Bm ? hB : 0.f);
    n += A ? 1.f : 0.f;
    any2 = any2 || Bm;
    if (G && j != i) G[(size_t)i * B + j] = ((A ? 1.f : 0.f) + (Bm ? 1.f : 0.f)) * sc;
  }
  l = wave_sum_f32(l);
  n = wave_sum_f32(n);
  const bool hit2 = __ballot(any2) != 0;
  if (lane == 0) {
    lrow[i] = l;
    nA[i] = n;
    if (KIND == T2L_RANK_HARDEST) sel2[i] = hit2 ? arg.j2 : -1;
  }
}

// ... the loss from the rows' shares in a fixed order ...
__global__ __launch_bounds__(256) void rl_loss_kernel(const float* __restrict__ lrow, int B, float sc, float* __restrict__ loss) {
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float v = 0.f;
  for (int i = tid; i < B; i += 256) v += lrow[i];
  v = wave_sum_f32(v);
  if (lane == 0) red[wave] = v;
  __syncthreads();
  if (tid == 0) loss[0] = ((red[0] + red[1]) + (red[2] + red[3])) * sc;
}

// ... one wave per column j: sum_k Bm_kj (the same expression on the same operands as the row pass: the same decision), and
// G_jj = -sc (sum_j' A_jj' + sum_k Bm_kj); then cl_grad_kernel.
template <int KIND>
__global__ __launch_bounds__(256) void rl_diag_kernel(const float* __restrict__ Cm, const float* __restrict__ diag,
                                                      const float* __restrict__ nA, const int* __restrict__ sel2, int B, float margin,
                                                      float sc, float* __restrict__ G) {
  const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= B) return;
  const float dj = diag[j];
  float n = 0.f;
  for (int k = lane; k < B; k += 64) {
    bool hit;
    if (KIND == T2L_RANK_PAIRWISE)
      hit = k != j && rank_hinge(margin, dj, Cm[(size_t)k * B + j]) > 0.f;
    else
      hit = sel2[k] == j;  // (j2 of row k is never k)
    n += hit ? 1.f : 0.f;
  }
  n = wave_sum_f32(n) + nA[j];
  if (lane == 0) G[(size_t)j * B + j] = n > 0.f ? -sc * n : 0.f;
}

static int loss_ws_reserve(t2l_ctx* ctx, size_t need) {
  if (ctx->loss_ws_cap < need) {
    if (ctx->loss_ws) T2L_HIP(ctx, hipFree(ctx->loss_ws));
    ctx->loss_ws = nullptr;
    ctx->loss_ws_cap = 0;
    T2L_HIP(ctx, hipMalloc(&ctx->loss_ws, need));
    ctx->loss_ws_cap = need;
  }
  return T2L_OK;
}

template <int KIND>
static int ranking_launch(t2l_ctx* ctx, const float* im, const float* p, int B, float margin, float sc, float* loss, float* ga,
                          float* gp, hipStream_t s) {
  if (B <= 128) {
    const int Bp = (B + 31) / 32 * 32;
    static PerDeviceOnce attr_done;
    if (attr_done.need(ctx->device)) {
      T2L_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&ranking_tiles_kernel<KIND>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024));
      attr_done.mark(ctx->device);
    }
    event_begin(ctx, "ranking_loss", s);
    const size_t lds = (2 * (size_t)Bp * (Bp + 1) + 14 * Bp + 4) * sizeof(float);
    hipLaunchKernelGGL(ranking_tiles_kernel<KIND>, dim3(ga ? 4 * (Bp / 32) : 1), dim3(256), lds, s, im, p, B, margin, sc, loss, ga, gp);
    event_end(ctx, "ranking_loss", s);
    T2L_HIP(ctx, hipGetLastError());
    return T2L_OK;
  }
  // Cm[B][B], G[nb*32][B] (grad_rowblock's A operand reads whole 32-row blocks: the rows past B are read, never written, and reach
  // no stored output row), then six vectors of B
  const int nb = (B + 31) / 32, rows4 = (B + 3) / 4;
  const size_t nC = (size_t)B * B, nG = (size_t)nb * 32 * B;
  if (int rc = loss_ws_reserve(ctx, (nC + nG + 6 * (size_t)B) * sizeof(float))) return rc;
  float* Cm = (float*)ctx->loss_ws;
  float *G = Cm + nC, *ia = G + nG, *ip = ia + B, *diag = ip + B, *nA = diag + B, *lrow = nA + B;
  int* sel2 = reinterpret_cast<int*>(lrow + B);
  event_begin(ctx, "ranking_loss", s);
  hipLaunchKernelGGL(cl_norm_kernel, dim3(rows4), dim3(256), 0, s, im, p, B, ia, ip);
  hipLaunchKernelGGL(rl_sim_kernel, dim3(nb * nb), dim3(64), 0, s, im, p, B, nb, ia, ip, Cm, diag);
  hipLaunchKernelGGL(rl_rows_kernel<KIND>, dim3(rows4), dim3(256), 0, s, Cm, diag, B, margin, sc, ga ? G : nullptr, nA, lrow, sel2);
  hipLaunchKernelGGL(rl_loss_kernel, dim3(1), dim3(256), 0, s, lrow, B, sc, loss);
  if (ga) {
    hipLaunchKernelGGL(rl_diag_kernel<KIND>, dim3(rows4), dim3(256), 0, s, Cm, diag, nA, sel2, B, margin, sc, G);
    hipLaunchKernelGGL(cl_grad_kernel, dim3(2 * nb), dim3(64), 0, s, G, B, nb, im, p, ia, ip, ga, gp);
  }
  event_end(ctx, "ranking_loss", s);
  T2L_HIP(ctx, hipGetLastError());
  return T2L_OK;
}

int ranking_loss_impl(t2l_ctx* ctx, const float* im, const float* p, int B, int kind, float margin, float scale, float* loss,
                      float* ga, float* gp, hipStream_t s) {
  const float sc = scale / (float)B;
  if (kind == T2L_RANK_PAIRWISE) return ranking_launch<T2L_RANK_PAIRWISE>(ctx, im, p, B, margin, sc, loss, ga, gp, s);
  return ranking_launch<T2L_RANK_HARDEST>(ctx, im, p, B, margin, sc, loss, ga, gp, s);
}

static int loss_big_impl(t2l_ctx* ctx, const float* a, const float* p, int B, float temp, float* loss, float* ga, float* gp,
                         hipStream_t s) {
  if (int rc = loss_ws_reserve(ctx, ((size_t)B * B + 5 * (size_t)B) * sizeof(float))) return rc;
  float* E = (float*)ctx->loss_ws;
  float *ia = E + (size_t)B * B, *ip = ia + B, *diag = ip + B, *R = diag + B, *C = R + B;
  const int nb = (B + 31) / 32, rows4 = (B + 3) / 4;
  event_begin(ctx, "contrastive_loss", s);
  hipLaunchKernelGGL(cl_norm_kernel, dim3(rows4), dim3(256), 0, s, a, p, B, ia, ip);
  hipLaunchKernelGGL(cl_sim_kernel, dim3(nb * nb), dim3(64), 0, s, a, p, B, nb, 1.0f / temp, ia, ip, E, diag);
  hipLaunchKernelGGL(cl_sums_kernel, dim3(rows4), dim3(256), 0, s, E, B, R, C);
  hipLaunchKernelGGL(cl_loss_kernel, dim3(1), dim3(256), 0, s, R, C, diag, B, 1.0f / temp, loss);
  if (ga) {
    hipLaunchKernelGGL(cl_g_kernel, dim3((unsigned)(((size_t)B * B + 255) / 256)), dim3(256), 0, s, E, R, C, B, 1.0f / (temp * (float)B));
    hipLaunchKernelGGL(cl_grad_kernel, dim3(2 * nb), dim3(64), 0, s, E, B, nb, a, p, ia, ip, ga, gp);
  }
  event_end(ctx, "contrastive_loss", s);
  T2L_HIP(ctx, hipGetLastError());
  return T2L_OK;
}

int loss_impl(t2l_ctx* ctx, const float* a, const float* p, int B, float temp, float* loss, float* ga, float* gp,
              hipStream_t s) {
  if (B > T2L_MAX_LOSS_BATCH) return fail(ctx, T2L_EINVAL, "t2l_contrastive_loss: batch > 1024 not supported");
  if (B > 128) return loss_big_impl(ctx, a, p, B, temp, loss, ga, gp, s);
  const int Bp = (B + 31) / 32 * 32;
  static PerDeviceOnce attr_done;
  if (attr_done.need(ctx->device)) {
    T2L_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&contrastive_tiles_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024));
    attr_done.mark(ctx->device);
  }
  event_begin(ctx, "contrastive_loss", s);
  const size_t lds = (2 * (size_t)Bp * (Bp + 1) + 10 * Bp) * sizeof(float);
  hipLaunchKernelGGL(contrastive_tiles_kernel, dim3(ga ? 4 * (Bp / 32) : 1), dim3(256), lds, s, a, p, B, 1.0f / temp, loss, ga, gp);
  event_end(ctx, "contrastive_loss", s);
  T2L_HIP(ctx, hipGetLastError());
  return T2L_OK;
}

}  // namespace t2l
