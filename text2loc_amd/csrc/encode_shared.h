// What the two cell-encoder translation units share: the packed-weight parameter block that t2l_load_weights builds
// (encode.hip) and both kernels read (encode.hip: two cells per workgroup at the published shape; encode_shaped.hip: one cell per
// workgroup at every compiled shape).
#pragma once
#include "t2l_internal.h"
#include "tile_blocks.h"

namespace t2l {

constexpr float kNumMean = 1826.6844940968194f;  // models/object_encoder.py:43
constexpr float kNumStd = 2516.8905096993817f;   // models/object_encoder.py:44

struct SmallMlp {  // get_mlp([in, 64, 256]) with BN folded (language_encoder.py:16-41)
  const float* w1;   // [64][in]
  const float* b1;   // [64]
  const float4* w2p; // packed [8 tiles][8][64] float4   (N=256, K=64)
  const float* b2;   // [256]
};

struct LayerW {
  const float4 *in_wp, *out_wp, *ff1_wp, *ff2_wp;
  const uint4 *in_hp, *out_hp, *ff1_hp, *ff2_hp;  // the same matrices as split-f16 fragments (pack_h)
  const float *in_b, *out_b, *ff1_b, *ff2_b, *ln1_w, *ln1_b, *ln2_w, *ln2_b;
};

struct EncParams {
  const float* class_tab;  // [n_class][256] rows already L2-normalised
  const float* color_tab;  // [n_color][256]
  int n_class, n_color;
  SmallMlp pos, color, num;
  const float4* pn_wp;     // mlp_pointnet packed (N=256,K=256)
  const uint4* pn_hp;
  const float* pn_b;
  const float4* merge_wp;  // nfeat consecutive packings (N=256, K=256), one per 256-wide feature slot
  const uint4* merge_hp;
  const float* merge_b;
  LayerW layer[4];
  int num_layers;
  int class_embed, color_embed, use_class, use_color, use_pos, use_num, nfeat;
  int split_ok;  // every activation entering a split-f16 GEMM is provably below the f16 range for these weights
};

struct EncoderWeights {
  EncParams p;
  char* blob = nullptr;  // every array p points at, one allocation (weight_table.h: Staging)
  // the shape the weights were loaded for (t2l_load_weights_shaped); the published one has the two-cell kernel of encode.hip in
  // front of the shape-templated kernel of encode_shaped.hip
  int embed_dim = kD, object_size = kS, num_heads = 4;
  bool published() const { return embed_dim == kD && object_size == kS && num_heads == 4; }
};

// the one-cell kernel (encode_shaped.hip): true when (embed_dim, num_heads, object_size) is a compiled shape
bool shape_is_compiled(int embed_dim, int num_heads, int object_size);
const char* compiled_shapes_text();
int encode_shaped_impl(t2l_ctx* ctx, const t2l_packed_cells* in, float* out, hipStream_t s);

}  // namespace t2l
