// What the training translation units share (train.hip through train_kernels.h, fine_train.hip): the counter-based dropout rule, the
// bump arena of a step's activations, the point-count standardization, and the launchers of train_kernels.h's row kernels that the fine
// step uses too (defined in train.hip, which alone includes train_kernels.h): ln_fwd_rows, ln_bwd_rows, rownorm_rows, seq_max_fwd_launch,
// seq_max_bwd_launch, drop_fwd_launch, relu_drop_bwd_launch. No __global__ definitions here, so any number of translation units may
// include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace t2l {
namespace train {

// num_encoder's input is (n_pts - mean) / std with these (models/object_encoder.py:43-44, 141-144)
constexpr float kNumPtsMean = 1826.6844940968194f, kNumPtsStd = 2516.8905096993817f;

// Counter-based dropout: keep element `idx` of site `site` iff the top 24 bits of lowbias32(idx*0x9E3779B1 + key) >= thr,
// key = seed ^ site*0x85EBCA77, thr = p*2^24. oracle/t2l_oracle_train.py:dropout_keep is the same function.
__device__ __forceinline__ bool keep_bit(uint32_t key, uint32_t idx, uint32_t thr) {
  uint32_t x = idx * 0x9E3779B1u + key;
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  x ^= x >> 16;
  return (x >> 8) >= thr;
}
struct Drop {
  uint32_t key = 0, thr = 0;  // thr == 0 -> identity
  float scale = 1.f;          // 1/(1-p)
};
static inline Drop make_drop(uint32_t seed, int site, float p) {
  Drop d;
  d.key = seed ^ (uint32_t)((uint64_t)site * 0x85EBCA77ull);
  d.thr = p > 0.f ? (uint32_t)((double)p * 16777216.0) : 0u;
  d.scale = d.thr ? 1.0f / (1.0f - p) : 1.0f;
  return d;
}

// Bump arena over one device allocation: take() only advances (256-byte granules), the owner compares off with cap after laying a
// pass out and rewinds off itself. Without a base (a pass that only counts) every pointer is null.
struct Arena {
  char* base = nullptr;
  size_t cap = 0, off = 0;
  template <typename T>
  T* take(size_t count) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += (count * sizeof(T) + 255) & ~(size_t)255;
    return p;
  }
};

}  // namespace train

// train.hip: the row kernels of train_kernels.h, by run-time width where they are templates on it. LayerNorm(x + dropout(y)) over T rows
// of D = 128, 256 or 1024 and its backward ((D, waves) one of (128, 4), (256, 16), (256, 4), (1024, 4); dgamma / dbeta added to, never
// null); F.normalize of M rows of D = 128 or 256 between a contiguous side and a side of row stride ld (forward: src contiguous, dst
// strided; backward: src = dy and y strided, dst contiguous). false: there is no instance of that width, and nothing was launched.
bool ln_fwd_rows(int D, const float* x, const float* y, int T, const float* gamma, const float* beta, const train::Drop& dr, float* out,
                 float* xhat, float* rstd, hipStream_t s);
bool ln_bwd_rows(int D, int waves, const float* dout, const float* xhat, const float* rstd, int T, const float* gamma, const train::Drop& dr,
                 float* d_res, float* d_y, float* dgamma, float* dbeta, hipStream_t s);
bool rownorm_rows(bool fwd, int D, const float* src, const float* y, float* dst, float* save_n, int M, int ld, hipStream_t s);
// max over each group's S rows of X (+ R when non-null), first maximum wins, the row kept in arg; the scatter back
void seq_max_fwd_launch(const float* X, const float* R, int B, int S, int D, float* out, int32_t* arg, hipStream_t s);
void seq_max_bwd_launch(const float* g, const int32_t* arg, int B, int S, int D, float* dX, hipStream_t s);
// hd = dropout(h) over n elements; d = dropout'(d) where h > 0, else 0, in place (Drop{}: the plain ReLU backward)
void drop_fwd_launch(const float* h, size_t n, const train::Drop& dr, float* hd, hipStream_t s);
void relu_drop_bwd_launch(float* d, const float* h, size_t n, const train::Drop& dr, hipStream_t s);

}  // namespace t2l
