// The blocks every eval-mode fused layer on 32 x 32 MFMA tiles is built from — the cell encoder (encode.hip, encode_shaped.hip), the
// fused t2l_text_inter layer (encode.hip) and the fine match (fine.hip), gfx950 only: the accumulator row map, the wave all-reduce,
// access to split-f16 LDS planes and the pinned ring that streams packed weight fragments. One definition each; the vector types are
// mfma_h3.h's (h3_*), the accumulator tile is f32x16 (mfma32.h).
#pragma once
#include "mfma32.h"
#include "mfma_h3.h"

namespace t2l {

// accumulator register r of lane half `half` holds row (r & 3) + 8 (r >> 2) + 4 half of a 32 x 32 tile (column = lane & 31)
__device__ __forceinline__ int acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// all-reduce sum over the 64 lanes on the VALU (DPP + v_permlane swaps): __shfl_xor lowers to ds_bpermute_b32 — six dependent
// LDS round trips per sum, and a LayerNorm needs two sums per token row
template <int CTRL>
__device__ __forceinline__ float wave_sum_dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float wave_sum(float v) {
  v += wave_sum_dpp<0xB1>(v);   // quad_perm [1,0,3,2]
  v += wave_sum_dpp<0x4E>(v);   // quad_perm [2,3,0,1]
  v += wave_sum_dpp<0x141>(v);  // row_half_mirror
  v += wave_sum_dpp<0x140>(v);  // row_mirror
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

// A token tile in LDS as two f16 planes (hi | lo of the split form, the same row stride): `off` = row * stride + column, in halves.
// plane_frag: the 8 k-values of a product's token operand, two ds_read_b128 and no conversion (SG, plain f16: the high plane only);
// plane_put4 / plane_get4: 4 consecutive features of a token, split once when stored and rebuilt as hi + lo when read back.
template <bool SG>
__device__ __forceinline__ HFrag plane_frag(const _Float16* __restrict__ hi, const _Float16* __restrict__ lo, int off) {
  HFrag f;
  f.hi = *reinterpret_cast<const h3_f16x8*>(hi + off);
  if constexpr (SG) f.lo = f.hi;
  else f.lo = *reinterpret_cast<const h3_f16x8*>(lo + off);
  return f;
}
__device__ __forceinline__ void plane_put4(_Float16* __restrict__ hi, _Float16* __restrict__ lo, int off, h3_f32x4 v) {
  h3_f16x4 h, l;
  h3_split4(v, h, l);
  *reinterpret_cast<h3_f16x4*>(hi + off) = h;
  // (the plain-f16 option drops the low halves from the PRODUCTS only: the stored activations — the residual stream — keep both)
  *reinterpret_cast<h3_f16x4*>(lo + off) = l;
}
__device__ __forceinline__ h3_f32x4 plane_get4(const _Float16* __restrict__ hi, const _Float16* __restrict__ lo, int off) {
  return h3_join4(*reinterpret_cast<const h3_f16x4*>(hi + off), *reinterpret_cast<const h3_f16x4*>(lo + off));
}

// dev experiment (make exp_enc / exp_fine EXPFLAG=-DT2L_EXP_HOTW, tools/hotw_probe.py; WRONG results, timing only): every weight fragment
// of a tile pass comes from the pass's first two k-steps — the instruction stream stays, the packed-weight stream out of the L2
// disappears. How much of the fused kernels' time is that stream?
#ifdef T2L_EXP_HOTW
#define T2L_HOT(s) ((s) & 1)
#else
#define T2L_HOT(s) (s)
#endif

// The weight fragments of one tile pass (packed by pack_split_f16, offset to the pass's first step and to this lane: 2 uint4 per lane
// and step, 128 uint4 per step), STEPS k-steps, through a register ring DEPTH steps deep: the fragment of step s + DEPTH is requested
// when step s is consumed, sched_barriers keep the requests where they are written (the compiler otherwise sinks every load to its use:
// one L2 round trip of ~1 us in front of every 0.1 us of MFMAs). body(s, fragment). Measured on t2l_text_inter (4,096 x 6): no ring
// 0.218 ms; depth 2 / 3 / 4 / 5 / 6 / 8 / 12 / 16: 0.169 / 0.168 / 0.169 / 0.170 / 0.173 / 0.174 / 0.181 / 0.186 ms — what matters is
// that the next requests are out before the MFMAs start, not how many (deeper rings cost registers and scalar spills).
template <bool SG, int STEPS, int DEPTH, typename F>
__device__ __forceinline__ void stream_weights(const uint4* __restrict__ wp, F&& body) {
  constexpr int D = STEPS < DEPTH ? STEPS : DEPTH;
  HFrag ring[D];
#pragma unroll
  for (int i = 0; i < D; ++i) ring[i] = load_h1<SG>(wp + T2L_HOT(i) * 128);
#pragma unroll
  for (int s = 0; s < STEPS; ++s) {
    const HFrag wf = ring[s % D];
    if (s + D < STEPS) ring[s % D] = load_h1<SG>(wp + T2L_HOT(s + D) * 128);
    __builtin_amdgcn_sched_barrier(0);
    body(s, wf);
    __builtin_amdgcn_sched_barrier(0);
  }
}

}  // namespace t2l
