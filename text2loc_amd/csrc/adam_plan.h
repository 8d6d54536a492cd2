// The layout of an optimizer state (train.hip: AdamSet) as plain host code, so that a host-only program can walk it
// (tests/adam_plan_check.cpp): where each trained tensor's moments live, the chunk table of the one-launch step, and when a re-bind
// keeps the previous binding's moments. No HIP in here.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

namespace t2l {

constexpr int64_t kAdamChunk = 1024;  // elements per workgroup of adam_kernel / zero_kernel

struct AdamPlan {
  std::vector<int64_t> offset;                      // tensor i's first element in each half of the moment buffer [2][total]
  std::vector<int32_t> chunk_tensor, chunk_first;   // chunk c covers elements [first * 1024, ...) of tensor chunk_tensor[c]
  std::vector<int32_t> chunk0;                      // [n + 1]: the first chunk of tensor i; chunk0[n] = the chunk count
  int64_t total = 0;
  int n_chunks() const { return (int)chunk_tensor.size(); }
  // the first chunk of tensor k and every tensor behind it; k >= n (no such tensor): the chunk count
  int first_chunk(size_t k) const { return chunk0[k < offset.size() ? k : offset.size()]; }
};

// ceil(numel / 1024) chunks per tensor, in list order (a tensor of 0 elements gets none)
inline AdamPlan adam_plan(const std::vector<int64_t>& numel) {
  AdamPlan p;
  for (size_t i = 0; i < numel.size(); ++i) {
    p.offset.push_back(p.total);
    p.chunk0.push_back(p.n_chunks());
    for (int64_t c = 0; c * kAdamChunk < numel[i]; ++c) {
      p.chunk_tensor.push_back((int32_t)i);
      p.chunk_first.push_back((int32_t)c);
    }
    p.total += numel[i];
  }
  p.chunk0.push_back(p.n_chunks());
  return p;
}

// A re-bind adopts the previous binding's moments (and its owner keeps the step counts) only for the SAME list: option
// "train_keep_adam_state" on at bind time, the previous binding had moments, the trained names equal in order, every element count equal.
inline bool adam_keep(bool option, bool had_moments, const std::vector<std::string>& old_names, const std::vector<int64_t>& old_numel,
                      const std::vector<std::string>& names, const std::vector<int64_t>& numel) {
  return option && had_moments && old_names == names && old_numel == numel;
}

}  // namespace t2l
