// What the training translation units share (train.hip through train_kernels.h, fine_train.hip): the counter-based dropout rule, the
// bump arena of a step's activations, the point-count standardization, and the launchers of train_kernels.h's row kernels that the fine
// step uses too (defined in train.hip, which alone includes train_kernels.h): ln_fwd_rows, ln_bwd_rows, rownorm_rows, seq_max_fwd_launch,
// seq_max_bwd_launch, drop_fwd_launch, relu_drop_bwd_launch. No __global__ definitions here, so any number of translation units may
// include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

struct t2l_ctx;

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

// One accumulator slot of a BatchNorm stage: [2 * 1024] channel sums + the ROW COUNT at kBnCount (cross-rank BatchNorm only, `sync`: the
// slot is summed over the ranks between the statistics and the apply launch — t2l_train_sync_bn — and the apply side then divides by
// the global count). The caller's buffer of t2l_train_sync_bn holds, in slots: [0, 16) the coarse object branch (forward | backward),
// 16 / 17 the text head's inter_mlp (forward, backward), [kFineBnSlot0, + kFineBnSlots) the fine step's current stage.
constexpr int kBnCount = 2048;
constexpr int kBnStride = 2056;
constexpr int kFineBnSlot0 = 18, kFineBnSlots = 4;

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

// train.hip: its optimizer state (AdamSet: the moments, the chunk tables of adam_kernel / zero_kernel, the keep rule of adam_plan.h)
// for an owner in another translation unit — the fine stage. adam_set_make builds the set over `trained` in list order; `prev` (may be
// null) is the set of the binding this one replaces: its moments are adopted (*kept; prev then has none) when adam_keep says so and
// stay with it otherwise; prev stays the caller's to adam_set_free, and after a failed call it is as it was. A step takes the tensors
// [t0, t1) of the list (one launch; none for an empty range), the zeroing all of them.
struct AdamSet;
struct AdamBound {
  std::string name;
  float *data, *grad;
  int64_t numel;
};
int adam_set_make(t2l_ctx* ctx, const std::vector<AdamBound>& trained, AdamSet* prev, bool* kept, AdamSet** out);
void adam_set_free(AdamSet* a);
void adam_set_step(const AdamSet* a, size_t t0, size_t t1, int64_t step, float lr, float b1, float b2, float eps, hipStream_t s);
void adam_set_zero(const AdamSet* a, hipStream_t s);
int adam_set_state(t2l_ctx* ctx, AdamSet* a, const char* api, int set, float* m, float* v, int64_t* step, int64_t* numel, int64_t packed,
                   hipStream_t s);

}  // namespace t2l
