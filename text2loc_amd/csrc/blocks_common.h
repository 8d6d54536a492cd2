// What the translation units of the dev-only block library (libt2l_blocks.so: train_blocks.hip, pointnet_blocks.hip, fine_blocks.hip, fine_train_blocks.hip, text_head_blocks.hip, encode_blocks.hip, encode_shaped_blocks.hip) share: one
// thread-local error text behind t2l_blk_last_error. Defined in train_blocks.hip.
#pragma once
#include <string>

#include "t2l_internal.h"

namespace t2l {

int blk_refuse(const std::string& msg);  // keeps the message, returns -1
int blk_finish(const char* who);         // hipGetLastError + a synchronise of the null stream: 0, or -2 with the message kept
// the inter-sentence layer t2l_text_head_load_weights packed for t2l_text_inter (text_head_blocks.hip, which sees th::Weights): false
// when no head is loaded or its inter layer is of no compiled shape
bool blk_text_inter_weights(t2l_ctx* ctx, InterFusedW* W, int* D, int* heads);

// the body of the probe kernels (fine_blocks.hip, encode_blocks.hip): the three forms whose float32 error the derived bounds cannot
// take from the code, as the INCLUDING translation unit compiles them
__device__ __forceinline__ void blk_probe_body(const float* __restrict__ in, float* __restrict__ e, float* __restrict__ rs, float* __restrict__ rc, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float v = in[i];
  e[i] = __expf(v);
  rs[i] = 1.0f / sqrtf(v);
  rc[i] = 1.f / v;
}

}  // namespace t2l
