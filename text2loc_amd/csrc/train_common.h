// What the training translation units share (train.hip through train_kernels.h, fine_train.hip): the counter-based dropout rule and
// the bump arena of a step's activations, the point-count standardization. No __global__ definitions here, so any number of translation units may include it.
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
// pass out and rewinds off itself.
struct Arena {
  char* base = nullptr;
  size_t cap = 0, off = 0;
  template <typename T>
  T* take(size_t count) {
    T* p = reinterpret_cast<T*>(base + off);
    off += (count * sizeof(T) + 255) & ~(size_t)255;
    return p;
  }
};

}  // namespace train
}  // namespace t2l
