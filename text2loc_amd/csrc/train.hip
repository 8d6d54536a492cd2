// Training step of the object branch (training/coarse.py:31-58): host orchestration.
//   t2l_train_bind              live parameter / gradient / BatchNorm-buffer pointers (no copies: the optimizer's tensors)
//   t2l_encode_cells_train      CellRetrievalNetwork.encode_objects under model.train() (batch-statistics BatchNorm,
//                               the four dropout sites of each TransformerEncoderLayer), activations kept for backward
//   t2l_encode_cells_backward   what autograd does for that graph: gradients accumulated (+=) into the bound buffers
//   t2l_adam_step / t2l_zero_grad   torch.optim.Adam defaults / optimizer.zero_grad()
// Kernels: train_kernels.h.
#include <math.h>
#include <string.h>

#include "adam_plan.h"
#include "t2l_internal.h"
#include "train_kernels.h"

namespace t2l {

using namespace train;

struct TTensor {
  float* data = nullptr;
  float* grad = nullptr;
  int64_t numel = 0;
};
using TensorMap = std::unordered_map<std::string, TTensor>;

// ---- one optimizer state (torch.optim.Adam's moments, inside the library) for the object branch and the text head alike; the layout
// and the keep decision are adam_plan.h's, the step counts the owner's
struct AdamSet {
  std::vector<std::string> names;  // the trained tensors, in step order
  std::vector<int64_t> numel;
  AdamPlan plan;        // offsets, chunks, total
  float* mv = nullptr;  // [2][plan.total]: first moments of all tensors (names order), then second moments
  AdamTensor* d_tensors = nullptr;
  AdamChunk* d_chunks = nullptr;

  // What a re-bind detaches from the binding it is about to free: a re-bind of the SAME model (model.to(), an externally assigned
  // .grad, ...) only moves POINTERS, so build() adopts these moments when adam_keep says so; on every other path (a refused bind
  // included) they are freed here
  struct Old {
    std::vector<std::string> names;
    std::vector<int64_t> numel;
    float* mv = nullptr;
    ~Old() { if (mv) (void)hipFree(mv); }
  };
  void detach(Old& o) {
    o.names = names, o.numel = numel, o.mv = mv;
    mv = nullptr;  // (release() must not free it)
  }
  void release() {
    for (void* p : {(void*)d_tensors, (void*)d_chunks, (void*)mv})
      if (p) (void)hipFree(p);
    d_tensors = nullptr; d_chunks = nullptr; mv = nullptr;
  }
  // build-or-adopt: the tables over `names` (set by the owner; every one is in t). *kept: old's moments were adopted — the owner then
  // keeps its step counts too; otherwise the moments are zero
  int build(t2l_ctx* ctx, const TensorMap& t, Old& old, bool* kept) {
    for (auto& nme : names) numel.push_back(t.at(nme).numel);
    plan = adam_plan(numel);
    const int64_t total = plan.total;
    *kept = adam_keep(ctx->train_keep_adam != 0, old.mv != nullptr, old.names, old.numel, names, numel);
    if (*kept) {
      std::swap(mv, old.mv);
    } else {
      if (old.mv) (void)hipFree(old.mv);  // (before its successor is allocated)
      old.mv = nullptr;
      T2L_HIP(ctx, hipMalloc(&mv, sizeof(float) * 2 * (size_t)total));
      T2L_HIP(ctx, hipMemset(mv, 0, sizeof(float) * 2 * (size_t)total));
    }
    std::vector<AdamTensor> ts;
    std::vector<AdamChunk> cs;
    for (size_t i = 0; i < names.size(); ++i) {
      const TTensor& x = t.at(names[i]);
      ts.push_back(AdamTensor{x.data, x.grad, mv + plan.offset[i], mv + total + plan.offset[i], x.numel});
    }
    for (int c = 0; c < plan.n_chunks(); ++c) cs.push_back(AdamChunk{plan.chunk_tensor[c], plan.chunk_first[c]});
    T2L_HIP(ctx, hipMalloc(&d_tensors, sizeof(AdamTensor) * ts.size()));
    T2L_HIP(ctx, hipMalloc(&d_chunks, sizeof(AdamChunk) * cs.size()));
    T2L_HIP(ctx, hipMemcpy(d_tensors, ts.data(), sizeof(AdamTensor) * ts.size(), hipMemcpyHostToDevice));
    T2L_HIP(ctx, hipMemcpy(d_chunks, cs.data(), sizeof(AdamChunk) * cs.size(), hipMemcpyHostToDevice));
    return T2L_OK;
  }
  // one step of the tensors behind chunks [c0, c1), which have taken `step` steps with this one
  void launch(int c0, int c1, int64_t step, float lr, float b1, float b2, float eps, hipStream_t s) const {
    if (c1 <= c0) return;
    const float bc1 = (float)(1.0 - pow((double)b1, (double)step));
    const float bc2s = (float)sqrt(1.0 - pow((double)b2, (double)step));
    hipLaunchKernelGGL(adam_kernel, dim3(c1 - c0), dim3(256), 0, s, d_tensors, d_chunks + c0, lr, b1, b2, eps, bc1, bc2s);
  }
  void zero(hipStream_t s) const { hipLaunchKernelGGL(zero_kernel, dim3(plan.n_chunks()), dim3(256), 0, s, d_tensors, d_chunks); }
  // t2l_adam_state / t2l_text_adam_state (`api`): the size and, when asked, the step (m == v == NULL), or the moments copied in (set) or
  // out with the step. `packed`: the owner's step count(s) as the call reports them; after a set with moments the owner takes *step.
  int state(t2l_ctx* ctx, const char* api, int set, float* m, float* v, int64_t* step, int64_t* n, int64_t packed, hipStream_t s) {
    const int64_t total = plan.total;
    if (n) *n = total;
    if (!m && !v) {
      if (step && !set) *step = packed;
      return T2L_OK;
    }
    if (!m || !v || !step) return fail(ctx, T2L_EINVAL, std::string(api) + ": pass m, v and step together");
    const size_t bytes = sizeof(float) * (size_t)total;
    T2L_HIP(ctx, hipMemcpyAsync(set ? mv : m, set ? m : mv, bytes, hipMemcpyDeviceToDevice, s));
    T2L_HIP(ctx, hipMemcpyAsync(set ? mv + total : v, set ? v : mv + total, bytes, hipMemcpyDeviceToDevice, s));
    if (!set) *step = packed;
    return T2L_OK;
  }
};

// the same set for an owner outside this file (train_common.h): the fine stage's optimizer
int adam_set_make(t2l_ctx* ctx, const std::vector<AdamBound>& trained, AdamSet* prev, bool* kept, AdamSet** out) {
  AdamSet* a = new AdamSet();
  TensorMap t;
  std::vector<int64_t> numel;
  for (auto& b : trained) {
    a->names.push_back(b.name);
    numel.push_back(b.numel);
    t[b.name] = TTensor{b.data, b.grad, b.numel};
  }
  // prev's moments leave it only when they are adopted; if the build then fails they go back, so the caller's previous binding — pointer
  // tables included — is as it was. Moments that are not adopted stay with prev until the caller frees it.
  AdamSet::Old old;
  const bool adopt = prev && adam_keep(ctx->train_keep_adam != 0, prev->mv != nullptr, prev->names, prev->numel, a->names, numel);
  if (adopt) prev->detach(old);
  if (int rc = a->build(ctx, t, old, kept)) {
    if (adopt) {  // (build swapped them into a before anything could fail)
      prev->mv = a->mv ? a->mv : old.mv;
      a->mv = old.mv = nullptr;
    }
    adam_set_free(a);
    return rc;
  }
  *out = a;
  return T2L_OK;
}
void adam_set_free(AdamSet* a) {
  if (!a) return;
  a->release();
  delete a;
}
void adam_set_step(const AdamSet* a, size_t t0, size_t t1, int64_t step, float lr, float b1, float b2, float eps, hipStream_t s) {
  a->launch(a->plan.first_chunk(t0), a->plan.first_chunk(t1), step, lr, b1, b2, eps, s);
}
void adam_set_zero(const AdamSet* a, hipStream_t s) {
  if (a->plan.n_chunks() > 0) a->zero(s);
}
int adam_set_state(t2l_ctx* ctx, AdamSet* a, const char* api, int set, float* m, float* v, int64_t* step, int64_t* numel, int64_t packed,
                   hipStream_t s) {
  return a->state(ctx, api, set, m, v, step, numel, packed, s);
}

// One [Linear, BatchNorm1d, ReLU] block of get_mlp (models/language_encoder.py:16-41) with its saved activations.
struct MlpLayer {
  std::string prefix;  // e.g. "object_encoder.pos_encoder.1"
  int cin = 0, cout = 0;
  float *y = nullptr, *a = nullptr, *mean = nullptr, *rstd = nullptr;  // pre-BN, post-ReLU, batch statistics
};
struct Branch {
  int kind = 0;  // 0 embedding lookup, 1 small MLP (K<=3 -> 64 -> 256), 2 PointNet-feature MLP (256 -> 256)
  int slot = 0;  // 256-wide slot of the concatenated feature row
  std::string table;          // kind 0
  const int32_t* idx = nullptr;
  const float* x = nullptr;   // kind 1/2 input
  int k_in = 0, standardize = 0;
  std::vector<MlpLayer> layers;
  float* save_n = nullptr;
};
// One nn.TransformerEncoderLayer (4 heads, post-norm, ReLU) with its saved activations: obj_inter_module.l of the object branch, and
// intra_module.0 / inter_module.0 of the text head (enc_layer_alloc / enc_layer_fwd / enc_layer_bwd below)
struct EncLayer {
  std::string prefix;  // of its tensors' names in the state's map
  int T = 0, B = 0, S = 0;    // T = B * S rows: B groups (cells / sentences / descriptions) of S rows that attend to each other
  int FF = 0, site0 = 0;      // feed-forward width; the first of its four dropout sites
  const float* x_in = nullptr;
  float *qkv = nullptr, *P = nullptr, *O = nullptr, *xhat1 = nullptr, *rstd1 = nullptr, *x1 = nullptr, *h = nullptr,
        *hd = nullptr, *xhat2 = nullptr, *rstd2 = nullptr, *x2 = nullptr;
};

constexpr int kBnSlots = 8;  // BatchNorm layers per pass: <= 2*3 small branches + pointnet mlp + merge

struct TrainState {
  t2l_ctx* ctx = nullptr;
  TensorMap t;
  t2l_model_config cfg{};
  AdamSet adam;
  double* bn_acc = nullptr;  // [2][kBnSlots][kBnStride] float64 partial sums of the BatchNorm stages (one slot per BN pass; forward | backward)
  int bn_slot = 0;
  bool fwd_acc_clean = false;  // the previous forward's last launch zeroed all accumulators (no memset launch in a step)
  bool bwd_acc_clean = false;  // the forward zeroed the backward half too; false after a backward used it (a second backward memsets)
  int pn_chunk0 = 0;         // chunks [pn_chunk0, adam.plan.n_chunks()) belong to the PointNet++ backbone (bound last)
  int64_t step = 0;          // Adam step of the object branch
  int64_t step_pn = 0;       // ... of the backbone: it only steps when its backward ran since the last zero_grad (torch.optim.Adam
  bool pn_touched = false;   // skips parameters whose .grad is None and keeps a step count per parameter)
  Arena ws;  // workspace (bump-allocated per forward)
  // the last forward
  bool have_forward = false;
  int M = 0, B = 0, T = 0, n_feat = 0;
  const int32_t* offsets = nullptr;
  std::vector<Branch> branches;
  MlpLayer merge;
  float *cat = nullptr, *X0 = nullptr, *save_nf = nullptr, *out = nullptr, *pool_n = nullptr;
  int32_t* pool_arg = nullptr;
  std::vector<EncLayer> layers;
  uint32_t seed = 0;
  float p = 0.f;
  void* pn = nullptr;  // PnTrain (pointnet_train.h): the PointNet++ backbone's training state, when its tensors are bound
};

static void pn_train_free(void* p);
static int pn_train_bind(t2l_ctx* ctx, TrainState* st, std::vector<std::string>& adam);

static TrainState* state(t2l_ctx* ctx) { return reinterpret_cast<TrainState*>(ctx->train); }

// ---- cross-rank BatchNorm statistics (t2l_train_sync_bn): slots [0, 2 kBnSlots) are the object branch's (forward | backward), the two
// behind them the text head's inter_mlp (forward, backward), then the fine step's (fine_train.hip; train_common.h)
static_assert(kFineBnSlot0 == 2 * kBnSlots + 2, "the fine step's slots start behind the text head's");
int64_t train_sync_bn_doubles() { return (int64_t)(kFineBnSlot0 + kFineBnSlots) * kBnStride; }
void train_sync_changed(t2l_ctx* ctx) {
  if (TrainState* st = state(ctx)) st->fwd_acc_clean = st->bwd_acc_clean = false;
}
static double* acc_base(t2l_ctx* ctx, TrainState* st) { return ctx->sync_fn ? ctx->sync_buf : st->bn_acc; }
// sum `slots` consecutive accumulator slots over the ranks (between a statistics launch and its apply launch)
static void sync_slots(t2l_ctx* ctx, double* first, int slots, hipStream_t s) {
  if (!ctx->sync_fn) return;
  if (ctx->sync_fn(ctx->sync_user, first, (int64_t)slots * kBnStride, (void*)s) != 0) ctx->sync_failed = true;
}

void free_train(t2l_ctx* ctx) {
  TrainState* st = state(ctx);
  if (!st) return;
  st->adam.release();
  for (void* p : {(void*)st->ws.base, (void*)st->bn_acc})
    if (p) (void)hipFree(p);
  pn_train_free(st->pn);
  delete st;
  ctx->train = nullptr;
}

// ---- GEMM launchers -----------------------------------------------------------------------------------------
static thread_local int tl_gemm_bf16 = 0;  // set from the context option "train_bf16" at the top of every forward / backward
static thread_local int tl_gemm_block64 = 0;  // option "train_gemm_block": 64 x 64 output blocks where the shape allows (default: with bf16 operands)
static inline bool blk64(int rows_out_mult, int cols_out) { return tl_gemm_block64 && rows_out_mult % 64 == 0 && cols_out % 64 == 0; }
// gemm_f32.h's contract for a k-contiguous operand: the reduction length is a whole number of 16-steps (gemm_load<true> reads two
// float4 per lane without a test against the end of the range). Every product of the step has one; a launch that has not is refused
// here, loudly, instead of reading past the operand's rows.
static inline bool gemm_kc_ok(int K, const char* who) {
  if (K > 0 && K % 16 == 0) return true;
  fprintf(stderr, "t2l: %s: a k-contiguous operand needs a reduction length that is a multiple of 16, got %d (launch refused)\n", who, K);
  return false;
}
// Y[M,N] = X[M,K] W[N,K]^T + b (relu)
static void gemm_nt_args(GemmArgs g, hipStream_t s) {  // g.M rows (ragged allowed), g.N columns
  if (!gemm_kc_ok(g.K, "gemm_nt")) return;
  if (blk64(64, g.N))
    hipLaunchKernelGGL((gemm4_kernel<true, true>), dim3(g.N / 64, (g.M + 63) / 64, 1), dim3(256), 0, s, g);
  else
    hipLaunchKernelGGL((gemm_kernel<true, true>), dim3(g.N / 32, (g.M + 31) / 32, 1), dim3(256), 0, s, g);
}
static void gemm_nt(const float* X, const float* W, const float* b, float* Y, int M, int N, int K, int relu, hipStream_t s) {
  gemm_nt_args(GemmArgs{X, W, Y, b, M, N, K, K, K, N, relu, 0, K, nullptr, tl_gemm_bf16}, s);
}
// dX[M,Kp] (+)= dY[M,N] W[N,Kp]
static void gemm_nn(const float* dY, const float* W, float* dX, int M, int N, int Kp, int accumulate, hipStream_t s) {
  GemmArgs g{dY, W, dX, nullptr, M, Kp, N, N, Kp, Kp, 0, accumulate, N, nullptr, tl_gemm_bf16};
  if (!gemm_kc_ok(N, "gemm_nn")) return;
  if (blk64(64, Kp))
    hipLaunchKernelGGL((gemm4_kernel<true, false>), dim3(Kp / 64, (M + 63) / 64, 1), dim3(256), 0, s, g);
  else
    hipLaunchKernelGGL((gemm_kernel<true, false>), dim3(Kp / 32, (M + 31) / 32, 1), dim3(256), 0, s, g);
}
// reduction split of dW[N,Kp] += dY[M,N]^T X[M,Kp] over the M rows: >= 64 rows per wave, ~1k workgroups
static void tn_split(int M, int N, int Kp, int blk, int& ksplit, int& kchunk) {
  const int tiles = (N / blk) * (Kp / blk);
  ksplit = std::max(1, std::min((M + 255) / 256, (1024 + tiles - 1) / tiles));
  kchunk = (((M + ksplit - 1) / ksplit) + 63) & ~63;
  ksplit = (M + kchunk - 1) / kchunk;
}
// dW[N,Kp] += dY[M,N]^T X[M,Kp]   (reduction over the M rows, split over grid.z, float atomics);  db[N] += column sums of dY
static void gemm_tn(const float* dY, const float* X, float* dW, float* db, int M, int N, int Kp, hipStream_t s) {
  const bool b64 = blk64(N, Kp);
  int ksplit, kchunk;
  tn_split(M, N, Kp, b64 ? 64 : 32, ksplit, kchunk);
  GemmArgs g{dY, X, dW, nullptr, N, Kp, M, N, Kp, Kp, 0, 1, kchunk, db, tl_gemm_bf16};
  if (b64)
    hipLaunchKernelGGL((gemm4_kernel<false, false>), dim3(Kp / 64, N / 64, ksplit), dim3(256), 0, s, g);
  else
    hipLaunchKernelGGL((gemm_kernel<false, false>), dim3(Kp / 32, N / 32, ksplit), dim3(256), 0, s, g);
}
// dW[N,Kp] += dY^T X (+ db) and dX[M,Kp] (+)= dY W in ONE launch (both read dY only); mask_src / drop: the ReLU + dropout backward
// of the layer that produced X's pre-image, applied in dX's epilogue (epi 2) instead of by a launch of its own
static void gemm_tn_nn(const float* dY, const float* X, float* dW, float* db, const float* W, float* dX, int M, int N, int Kp, int accumulate,
                       const float* mask_src, const Drop* drop, hipStream_t s) {
  if (!gemm_kc_ok(N, "gemm_tn_nn")) return;
  const bool b64 = blk64(N, Kp);
  const int blk = b64 ? 64 : 32;
  int ksplit, kchunk;
  tn_split(M, N, Kp, blk, ksplit, kchunk);
  GemmPair p{};
  p.tn = GemmArgs{dY, X, dW, nullptr, N, Kp, M, N, Kp, Kp, 0, 1, kchunk, db, tl_gemm_bf16};
  p.nn = GemmArgs{dY, W, dX, nullptr, M, Kp, N, N, Kp, Kp, 0, accumulate, N, nullptr, tl_gemm_bf16};
  if (mask_src) {
    p.nn.epi = 2;
    p.nn.mask_src = mask_src;
    p.nn.drop_key = drop->key;
    p.nn.drop_thr = drop->thr;
    p.nn.drop_scale = drop->scale;
  }
  p.tn_gx = Kp / blk;
  p.tn_gy = N / blk;
  p.tn_blocks = p.tn_gx * p.tn_gy * ksplit;
  p.nn_gx = Kp / blk;
  const int nn_blocks = p.nn_gx * ((M + blk - 1) / blk);
  if (b64)
    hipLaunchKernelGGL(gemm4_pair_kernel, dim3(p.tn_blocks + nn_blocks), dim3(256), 0, s, p);
  else
    hipLaunchKernelGGL(gemm_pair_kernel, dim3(p.tn_blocks + nn_blocks), dim3(256), 0, s, p);
}
// Y_q[M,N] = X_q[M,K] W_q[N,K]^T + b_q for n <= 3 independent jobs of one shape, ONE launch (32 x 32 tiles; grid.z = job)
static void gemm_nt_multi(int n, const float* const* X, const float* const* W, const float* const* b, float* const* Y, int M, int N, int K,
                          hipStream_t s) {
  if (!gemm_kc_ok(K, "gemm_nt_multi")) return;
  GemmMulti gm{};
  for (int q = 0; q < n; ++q) gm.j[q] = GemmArgs{X[q], W[q], Y[q], b[q], M, N, K, K, K, N, 0, 0, K, nullptr, tl_gemm_bf16};
  hipLaunchKernelGGL((gemm_multi_kernel<true, true>), dim3(N / 32, (M + 31) / 32, n), dim3(256), 0, s, gm);
}
// dW_q[N,Kp] += dY_q^T X_q (+ db_q) and dX_q[M,Kp] = dY_q W_q for n <= 3 independent jobs of one shape, ONE launch (32 x 32 tiles;
// grid.y = job, a job's blocks flattened in x as gemm_tn_nn's)
static void gemm_tn_nn_multi(int n, const float* const* dY, const float* const* X, float* const* dW, float* const* db, const float* const* W,
                             float* const* dX, int M, int N, int Kp, hipStream_t s) {
  if (!gemm_kc_ok(N, "gemm_tn_nn_multi")) return;
  int ksplit, kchunk;
  tn_split(M, N, Kp, 32, ksplit, kchunk);
  GemmPairMulti gp{};
  int pair_blocks = 0;
  for (int q = 0; q < n; ++q) {
    GemmPair& p = gp.p[q];
    p.tn = GemmArgs{dY[q], X[q], dW[q], nullptr, N, Kp, M, N, Kp, Kp, 0, 1, kchunk, db[q], tl_gemm_bf16};
    p.nn = GemmArgs{dY[q], W[q], dX[q], nullptr, M, Kp, N, N, Kp, Kp, 0, 0, N, nullptr, tl_gemm_bf16};
    p.tn_gx = Kp / 32;
    p.tn_gy = N / 32;
    p.tn_blocks = p.tn_gx * p.tn_gy * ksplit;
    p.nn_gx = Kp / 32;
    pair_blocks = p.tn_blocks + p.nn_gx * ((M + 31) / 32);
  }
  hipLaunchKernelGGL(gemm_pair_multi_kernel, dim3(pair_blocks, n), dim3(256), 0, s, gp);
}
// element-wise dropout of n values (the feed-forward hidden dropout), and the ReLU (h > 0) + dropout backward in place; both training
// steps' (train_common.h)
void drop_fwd_launch(const float* h, size_t n, const Drop& dr, float* hd, hipStream_t s) {
  hipLaunchKernelGGL(drop_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, h, n, dr, hd);
}
void relu_drop_bwd_launch(float* d, const float* h, size_t n, const Drop& dr, hipStream_t s) {
  hipLaunchKernelGGL(relu_drop_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d, h, n, dr);
}
// ---- one TransformerEncoderLayer, for the object branch and the text head alike -----------------------------------------------
// What differs between the two states' Linear products. The text head's run on the tiled LDS-ring GEMM of text_head.hip (fast_gemm:
// 256 x 256 tiles, bf16 planes, split-bf16 by default — 466 GFLOP per step at B = 64 are GEMM-shaped work that the object branch's
// tile-per-workgroup products, built for 1,792-row operands, serve at a third of its rate); shapes it does not take (fewer than 64
// rows, a width that is no multiple of 256) and every product of the object branch keep the products of gemm_f32.h with the same
// operand arithmetic. (An f32-MFMA operand option existed until round 5: 7.6 ms per step against PyTorch's 5.6; removed.)
struct Products {
  t2l_ctx* ctx;
  bool tiled;  // may use fast_gemm
};
static bool t_fast(const Products& pr, int M, int N, int K) { return pr.tiled && N % 256 == 0 && K % 32 == 0 && K % 4 == 0 && M >= 64; }
static void t_gemm_nt(const Products& pr, const float* X, const float* W, const float* b, float* Y, int M, int N, int K, int relu, hipStream_t s) {
  if (t_fast(pr, M, N, K)) (void)fast_gemm(pr.ctx, X, false, W, false, b, Y, M, N, K, relu, 0, pr.ctx->text_train_bf16 == 1, s);
  else gemm_nt(X, W, b, Y, M, N, K, relu, s);
}
// dW[N,Kp] += dY^T X, db[N] += column sums of dY, and (dX != nullptr) dX[M,Kp] (+)= dY W, through the ReLU + dropout backward of the
// layer that produced X's pre-image when mask_src is given
static void t_gemm_tn_nn(const Products& pr, const float* dY, const float* X, float* dW, float* db, const float* W, float* dX, int M, int N, int Kp,
                         int accumulate, const float* mask_src, const Drop* drop, hipStream_t s) {
  if (t_fast(pr, N, Kp, M) && (!dX || t_fast(pr, M, Kp, N)) && N % 4 == 0) {
    const bool single = pr.ctx->text_train_bf16 == 1;
    (void)fast_gemm(pr.ctx, dY, true, X, true, nullptr, dW, N, Kp, M, 0, 1, single, s, db);  // (db: column sums of dY, in its split pass)
    if (dX) {
      (void)fast_gemm(pr.ctx, dY, false, W, true, nullptr, dX, M, Kp, N, 0, accumulate, single, s);
      if (mask_src) relu_drop_bwd_launch(dX, mask_src, (size_t)M * Kp, *drop, s);
    }
    return;
  }
  if (dX) gemm_tn_nn(dY, X, dW, db, W, dX, M, N, Kp, accumulate, mask_src, drop, s);
  else gemm_tn(dY, X, dW, db, M, N, Kp, s);
}

static size_t attn_lds(int S, int HD, bool bwd) { return sizeof(float) * ((size_t)(bwd ? 4 : 3) * S * (HD + 1) + (size_t)(bwd ? 3 : 1) * S * (S + 1)); }
// the attention kernels of a layer: the instance with S at compile time where there is one (the object branch's shape), else S at run time
template <int HD, typename... A>
static void attn_fwd_launch(int B, int S, hipStream_t s, A... a) {
  if (HD == kTHd && S == kTS) hipLaunchKernelGGL((attn_fwd_kernel<kTHd, kTS>), dim3(B * 4), dim3(256), attn_lds(S, HD, false), s, a...);
  else hipLaunchKernelGGL((attn_fwd_kernel<HD, 0>), dim3(B * 4), dim3(256), attn_lds(S, HD, false), s, a...);
}
template <int HD, typename... A>
static void attn_bwd_launch(int B, int S, hipStream_t s, A... a) {
  if (HD == kTHd && S == kTS) hipLaunchKernelGGL((attn_bwd_kernel<kTHd, kTS>), dim3(B * 4), dim3(256), attn_lds(S, HD, true), s, a...);
  else hipLaunchKernelGGL((attn_bwd_kernel<HD, 0>), dim3(B * 4), dim3(256), attn_lds(S, HD, true), s, a...);
}
// the HD = 256 instances (the text head's d = 1024 layer) take more dynamic LDS than a kernel gets unasked: once per device
static void attn256_allow_lds(int device) {
  static PerDeviceOnce once;
  if (once.need(device)) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_fwd_kernel<256, 0>), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_bwd_kernel<256, 0>), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    once.mark(device);
  }
}
// out = LayerNorm(x + dropout(y)) over T rows of D: one wave per row, four rows per workgroup
template <int D>
static void ln_fwd_launch(const float* x, const float* y, int T, const float* gamma, const float* beta, const Drop& dr, float* out, float* xhat,
                          float* rstd, hipStream_t s) {
  hipLaunchKernelGGL((ln_fwd_kernel<D>), dim3((T + 3) / 4), dim3(256), 0, s, x, y, T, gamma, beta, dr, out, xhat, rstd);
}
// its backward; dgamma / dbeta are added to. LN_WAVES: waves per workgroup, the caller's measured choice for its shape (train_kernels.h:
// ln_bwd_kernel): 16 for the object branch's 1,792 rows of 256, in at most 32 workgroups; 4 for the text head, in at most 64 (at
// D = 1024 the partials of 16 waves would not fit the LDS).
template <int D, int LN_WAVES>
static void ln_bwd_launch(const float* dout, const float* xhat, const float* rstd, int T, const float* gamma, const Drop& dr, float* d_res,
                          float* d_y, float* dgamma, float* dbeta, hipStream_t s) {
  const int ln_grid = std::min(LN_WAVES == 16 ? 32 : 64, (T + 15) / 16);
  hipLaunchKernelGGL((ln_bwd_kernel<D, LN_WAVES>), dim3(ln_grid), dim3(LN_WAVES * 64), 0, s, dout, xhat, rstd, T, gamma, dr, d_res, d_y, dgamma,
                     dbeta);
}
// max over a cell's 28 slots + F.normalize (one workgroup per cell), and its backward. zero / zero_n: what the forward's last launch
// clears for the step (pool_norm_fwd_kernel)
static void pool_norm_fwd_launch(const float* x, float* out, int32_t* arg, float* save_n, float* out2, double* zero, int zero_n, int B,
                                 hipStream_t s) {
  hipLaunchKernelGGL(pool_norm_fwd_kernel, dim3(B), dim3(256), 0, s, x, out, arg, save_n, out2, zero, zero_n);
}
static void pool_norm_bwd_launch(const float* gout, const float* out, const int32_t* arg, const float* save_n, float* dX, int B, hipStream_t s) {
  hipLaunchKernelGGL(pool_norm_bwd_kernel, dim3(B), dim3(256), 0, s, gout, out, arg, save_n, dX);
}
// out[b][c] = max over the S rows of group b of (X + R) (R optional) with its argument, and the scatter back (the text head's tokens and
// sentences, the fine step's hints: train_common.h)
void seq_max_fwd_launch(const float* X, const float* R, int B, int S, int D, float* out, int32_t* arg, hipStream_t s) {
  hipLaunchKernelGGL(seq_max_fwd_kernel, dim3((unsigned)(((size_t)B * D + 255) / 256)), dim3(256), 0, s, X, R, B, S, D, out, arg);
}
void seq_max_bwd_launch(const float* g, const int32_t* arg, int B, int S, int D, float* dX, hipStream_t s) {
  hipLaunchKernelGGL(seq_max_bwd_kernel, dim3((unsigned)(((size_t)B * S * D + 255) / 256)), dim3(256), 0, s, g, arg, B, S, D, dX);
}

// the saved activations of L (T, B, S, FF set by the caller)
template <int D>
static void enc_layer_alloc(Arena& ws, EncLayer& L, float p) {
  const size_t T = (size_t)L.T;
  L.qkv = ws.take<float>(T * 3 * D);
  L.P = ws.take<float>((size_t)L.B * 4 * L.S * L.S);
  L.O = ws.take<float>(T * D);
  L.xhat1 = ws.take<float>(T * D);
  L.rstd1 = ws.take<float>(T);
  L.x1 = ws.take<float>(T * D);
  L.h = ws.take<float>(T * L.FF);
  L.hd = p > 0.f ? ws.take<float>(T * L.FF) : L.h;
  L.xhat2 = ws.take<float>(T * D);
  L.rstd2 = ws.take<float>(T);
  L.x2 = ws.take<float>(T * D);
}
// tmp: [T][D] scratch. 7 launches on the products of gemm_f32.h.
template <int D>
static void enc_layer_fwd(const Products& pr, const TensorMap& t, EncLayer& L, uint32_t seed, float p, float* tmp, hipStream_t s) {
  constexpr int HD = D / 4;
  const int T = L.T, FF = L.FF;
  auto W = [&](const char* n) -> const TTensor& { return t.at(L.prefix + n); };
  t_gemm_nt(pr, L.x_in, W(".self_attn.in_proj_weight").data, W(".self_attn.in_proj_bias").data, L.qkv, T, 3 * D, D, 0, s);
  attn_fwd_launch<HD>(L.B, L.S, s, (const float*)L.qkv, L.P, L.O, L.S, make_drop(seed, L.site0 + 0, p));
  t_gemm_nt(pr, L.O, W(".self_attn.out_proj.weight").data, W(".self_attn.out_proj.bias").data, tmp, T, D, D, 0, s);
  ln_fwd_launch<D>(L.x_in, tmp, T, W(".norm1.weight").data, W(".norm1.bias").data, make_drop(seed, L.site0 + 1, p), L.x1, L.xhat1, L.rstd1, s);
  if (t_fast(pr, T, FF, D)) {  // linear1 + ReLU in the GEMM's epilogue (h is kept for backward); the dropout behind it as one pass
    (void)fast_gemm(pr.ctx, L.x1, false, W(".linear1.weight").data, false, W(".linear1.bias").data, L.h, T, FF, D, 1, 0, pr.ctx->text_train_bf16 == 1, s);
    if (p > 0.f) drop_fwd_launch(L.h, (size_t)T * FF, make_drop(seed, L.site0 + 2, p), L.hd, s);
  } else {  // ... and the dropout too in the same epilogue (hd feeds linear2)
    GemmArgs g{L.x1, W(".linear1.weight").data, L.h, W(".linear1.bias").data, T, FF, D, D, D, FF, 1, 0, D, nullptr, tl_gemm_bf16};
    if (p > 0.f) {
      const Drop dr = make_drop(seed, L.site0 + 2, p);
      g.epi = 1;
      g.C2 = L.hd;
      g.drop_key = dr.key;
      g.drop_thr = dr.thr;
      g.drop_scale = dr.scale;
    }
    gemm_nt_args(g, s);
  }
  t_gemm_nt(pr, L.hd, W(".linear2.weight").data, W(".linear2.bias").data, tmp, T, D, FF, 0, s);
  ln_fwd_launch<D>(L.x1, tmp, T, W(".norm2.weight").data, W(".norm2.bias").data, make_drop(seed, L.site0 + 3, p), L.x2, L.xhat2, L.rstd2, s);
}
// The backward's scratch: taken by the CALLER, who knows whether its layers can share one (the object branch's do: same shape).
struct EncScratch {
  float *dA, *dB, *dC, *dB2, *dO, *dH, *dqkv;
};
template <int D>
static EncScratch enc_scratch_take(Arena& ws, int T, int FF) {
  const size_t n = (size_t)T * D;
  EncScratch sc;
  sc.dA = ws.take<float>(n);
  sc.dB = ws.take<float>(n);
  sc.dC = ws.take<float>(n);
  sc.dB2 = ws.take<float>(n);
  sc.dO = ws.take<float>(n);
  sc.dH = ws.take<float>((size_t)T * FF);
  sc.dqkv = ws.take<float>(n * 3);
  return sc;
}
// dcur: gradient w.r.t. the layer's output x2 (read). Returns the gradient w.r.t. the layer's input, which lives in sc.dC (nullptr when
// need_dx is false). 7 launches on the products of gemm_f32.h.
// LN_WAVES: waves per workgroup of the LayerNorm backward (ln_bwd_launch).
template <int D, int LN_WAVES>
static float* enc_layer_bwd(const Products& pr, const TensorMap& t, const EncLayer& L, uint32_t seed, float p, const EncScratch& sc,
                            const float* dcur, bool need_dx, hipStream_t s) {
  constexpr int HD = D / 4;
  const int T = L.T, FF = L.FF;
  auto W = [&](const char* nme) -> const TTensor& { return t.at(L.prefix + nme); };
  auto ln_bwd = [&](const float* dout, const float* xhat, const float* rstd, const TTensor& gamma, const TTensor& beta, int site, float* d_res,
                    float* d_y) {
    ln_bwd_launch<D, LN_WAVES>(dout, xhat, rstd, T, gamma.data, make_drop(seed, site, p), d_res, d_y, gamma.grad, beta.grad, s);
  };
  // norm2 + dropout2
  ln_bwd(dcur, L.xhat2, L.rstd2, W(".norm2.weight"), W(".norm2.bias"), L.site0 + 3, sc.dA, sc.dB);
  {  // linear2: dW2 += dB^T hd, and dH = (dB W2) through the ReLU + dropout backward
    const Drop dr = make_drop(seed, L.site0 + 2, p);
    t_gemm_tn_nn(pr, sc.dB, L.hd, W(".linear2.weight").grad, W(".linear2.bias").grad, W(".linear2.weight").data, sc.dH, T, D, FF, 0, L.h, &dr, s);
  }
  // linear1; dA (= dz2, the residual path) += dH W1
  t_gemm_tn_nn(pr, sc.dH, L.x1, W(".linear1.weight").grad, W(".linear1.bias").grad, W(".linear1.weight").data, sc.dA, T, FF, D, 1, nullptr, nullptr, s);
  // norm1 + dropout1
  ln_bwd(sc.dA, L.xhat1, L.rstd1, W(".norm1.weight"), W(".norm1.bias"), L.site0 + 1, sc.dC, sc.dB2);
  // out_proj
  t_gemm_tn_nn(pr, sc.dB2, L.O, W(".self_attn.out_proj.weight").grad, W(".self_attn.out_proj.bias").grad, W(".self_attn.out_proj.weight").data, sc.dO,
               T, D, D, 0, nullptr, nullptr, s);
  attn_bwd_launch<HD>(L.B, L.S, s, (const float*)L.qkv, (const float*)L.P, (const float*)sc.dO, sc.dqkv, L.S, make_drop(seed, L.site0 + 0, p));
  // in_proj; dC (= dz1, the residual path) += dqkv Win
  t_gemm_tn_nn(pr, sc.dqkv, L.x_in, W(".self_attn.in_proj_weight").grad, W(".self_attn.in_proj_bias").grad,
               need_dx ? W(".self_attn.in_proj_weight").data : nullptr, need_dx ? sc.dC : nullptr, T, 3 * D, D, need_dx ? 1 : 0, nullptr, nullptr, s);
  return need_dx ? sc.dC : nullptr;
}

static int need(t2l_ctx* ctx, TrainState* st, const std::string& name, int64_t numel, bool with_grad, TTensor** out) {
  auto it = st->t.find(name);
  if (it == st->t.end()) return fail(ctx, T2L_EINVAL, "t2l_train_bind: missing tensor '" + name + "'");
  if (it->second.numel != numel)
    return fail(ctx, T2L_EINVAL, "t2l_train_bind: '" + name + "' has " + std::to_string(it->second.numel) + " elements, expected " +
                                     std::to_string(numel));
  if (with_grad && !it->second.grad) return fail(ctx, T2L_EINVAL, "t2l_train_bind: '" + name + "' needs a gradient buffer");
  if (out) *out = &it->second;
  return T2L_OK;
}

static const TTensor& T_(TrainState* st, const std::string& n) { return st->t.at(n); }

// names + shapes of one get_mlp block
static int check_mlp_layer(t2l_ctx* ctx, TrainState* st, const std::string& p, int cin, int cout, std::vector<std::string>& params) {
  int rc;
  if ((rc = need(ctx, st, p + ".0.weight", (int64_t)cin * cout, true, nullptr))) return rc;
  if ((rc = need(ctx, st, p + ".0.bias", cout, true, nullptr))) return rc;
  if ((rc = need(ctx, st, p + ".1.weight", cout, true, nullptr))) return rc;
  if ((rc = need(ctx, st, p + ".1.bias", cout, true, nullptr))) return rc;
  if ((rc = need(ctx, st, p + ".1.running_mean", cout, false, nullptr))) return rc;
  if ((rc = need(ctx, st, p + ".1.running_var", cout, false, nullptr))) return rc;
  for (const char* sfx : {".0.weight", ".0.bias", ".1.weight", ".1.bias"}) params.push_back(p + sfx);
  return T2L_OK;
}

int train_bind_impl(t2l_ctx* ctx, const t2l_train_tensor* tensors, int n, const t2l_model_config* cfg) {
  if (!tensors || n <= 0 || !cfg) return fail(ctx, T2L_EINVAL, "t2l_train_bind: null argument");
  if (cfg->num_heads != kTH) return fail(ctx, T2L_EINVAL, "t2l_train_bind: the training step is built for the published shape only (embed dim 256, 4 attention heads, object_size 28)");
  const int n_feat = (cfg->use_class != 0) + (cfg->use_color != 0) + (cfg->use_position != 0) + (cfg->use_num != 0);
  if (n_feat < 2) return fail(ctx, T2L_EINVAL, "t2l_train_bind: training needs at least two of the class/color/position/num features");
  // with option "train_keep_adam_state" set (the Python seam sets it for exactly a re-bind of the same model) the Adam moments and
  // the bias-correction steps of the previous binding carry over when the parameter list (names and sizes) is unchanged
  AdamSet::Old old;
  int64_t old_step = 0, old_step_pn = 0;
  if (TrainState* o = state(ctx)) {
    o->adam.detach(old);
    old_step = o->step;
    old_step_pn = o->step_pn;
  }
  free_train(ctx);
  TrainState* st = new TrainState();
  ctx->train = st;
  st->cfg = *cfg;
  st->n_feat = n_feat;
  for (int i = 0; i < n; ++i) {
    if (!tensors[i].name || !tensors[i].data) return fail(ctx, T2L_EINVAL, "t2l_train_bind: null name/data");
    st->t[tensors[i].name] = TTensor{tensors[i].data, tensors[i].grad, tensors[i].numel};
  }
  std::vector<std::string>& P = st->adam.names;
  const std::string oe = "object_encoder.";
  int rc;
  if (cfg->use_class) {
    if (cfg->class_embed) {
      auto it = st->t.find(oe + "class_embedding.weight");
      if (it == st->t.end() || !it->second.grad || it->second.numel % kTD) return fail(ctx, T2L_EINVAL, "t2l_train_bind: class_embedding.weight");
      P.push_back(oe + "class_embedding.weight");
    } else if ((rc = check_mlp_layer(ctx, st, oe + "mlp_pointnet.0", 256, kTD, P))) return rc;
  }
  if (cfg->use_color) {
    if (cfg->color_embed) {
      auto it = st->t.find(oe + "color_embedding.weight");
      if (it == st->t.end() || !it->second.grad || it->second.numel % kTD) return fail(ctx, T2L_EINVAL, "t2l_train_bind: color_embedding.weight");
      P.push_back(oe + "color_embedding.weight");
    } else {
      if ((rc = check_mlp_layer(ctx, st, oe + "color_encoder.0", 3, 64, P))) return rc;
      if ((rc = check_mlp_layer(ctx, st, oe + "color_encoder.1", 64, kTD, P))) return rc;
    }
  }
  if (cfg->use_position) {
    if ((rc = check_mlp_layer(ctx, st, oe + "pos_encoder.0", 3, 64, P))) return rc;
    if ((rc = check_mlp_layer(ctx, st, oe + "pos_encoder.1", 64, kTD, P))) return rc;
  }
  if (cfg->use_num) {
    if ((rc = check_mlp_layer(ctx, st, oe + "num_encoder.0", 1, 64, P))) return rc;
    if ((rc = check_mlp_layer(ctx, st, oe + "num_encoder.1", 64, kTD, P))) return rc;
  }
  if ((rc = check_mlp_layer(ctx, st, oe + "mlp_merge.0", n_feat * kTD, kTD, P))) return rc;
  for (int l = 0; l < cfg->num_layers; ++l) {
    const std::string p = "obj_inter_module." + std::to_string(l);
    const std::pair<const char*, int64_t> req[] = {
        {".self_attn.in_proj_weight", 3 * kTD * kTD}, {".self_attn.in_proj_bias", 3 * kTD},
        {".self_attn.out_proj.weight", kTD * kTD},    {".self_attn.out_proj.bias", kTD},
        {".linear1.weight", 2 * kTD * kTD},           {".linear1.bias", 2 * kTD},
        {".linear2.weight", 2 * kTD * kTD},           {".linear2.bias", kTD},
        {".norm1.weight", kTD},                       {".norm1.bias", kTD},
        {".norm2.weight", kTD},                       {".norm2.bias", kTD}};
    for (auto& r : req) {
      if ((rc = need(ctx, st, p + r.first, r.second, true, nullptr))) return rc;
      P.push_back(p + r.first);
    }
  }
  const size_t n_obj_tensors = P.size();
  if ((rc = pn_train_bind(ctx, st, P))) return rc;  // the PointNet++ backbone, when bound with gradients
  T2L_HIP(ctx, hipMalloc(&st->bn_acc, sizeof(double) * kBnStride * kBnSlots * 2));  // slots of the forward, then of the backward
  st->ctx = ctx;
  bool kept;
  if ((rc = st->adam.build(ctx, st->t, old, &kept))) return rc;
  if (kept) {
    st->step = old_step;
    st->step_pn = old_step_pn;
  }
  st->pn_chunk0 = st->adam.plan.first_chunk(n_obj_tensors);
  return T2L_OK;
}

static MlpLayer make_layer(TrainState* st, const std::string& prefix, int cin, int cout, int M) {
  MlpLayer L;
  L.prefix = prefix;
  L.cin = cin;
  L.cout = cout;
  L.y = st->ws.take<float>((size_t)M * cout);
  L.a = st->ws.take<float>((size_t)M * cout);
  L.mean = st->ws.take<float>(cout);
  L.rstd = st->ws.take<float>(cout);
  return L;
}

// ---- the [BatchNorm1d, ReLU] stage of n <= kMaxJobs blocks of one shape, ONE launch per step of it (train_kernels.h): the layers that
// are alone (mlp_merge, mlp_pointnet) with n = 1, the small branches with n = 2 or 3
static BnJob bn_job(TrainState* st, const MlpLayer& L, float* d, int slot) {
  BnJob j{};
  j.y = L.y;
  j.out = L.a;
  j.d = d;
  j.acc = acc_base(st->ctx, st) + (size_t)(slot % (2 * kBnSlots)) * kBnStride;
  j.gamma = T_(st, L.prefix + ".1.weight").data;
  j.beta = T_(st, L.prefix + ".1.bias").data;
  j.run_mean = T_(st, L.prefix + ".1.running_mean").data;
  j.run_var = T_(st, L.prefix + ".1.running_var").data;
  j.save_mean = L.mean;
  j.save_rstd = L.rstd;
  j.dgamma = T_(st, L.prefix + ".1.weight").grad;
  j.dbeta = T_(st, L.prefix + ".1.bias").grad;
  return j;
}
// the jobs of blocks L[0..n) (backward: d[q] = the gradient w.r.t. L[q]'s ReLU output, overwritten) on the next n accumulator slots:
// CONSECUTIVE ones, so that one cross-rank sum covers the launch
static BnMulti bn_jobs(TrainState* st, int n, const MlpLayer* const* L, float* const* d, int M) {
  BnMulti b{};
  b.M = M;
  b.C = L[0]->cout;
  b.momentum = 0.1f;
  b.sync = st->ctx->sync_fn ? 1 : 0;
  for (int q = 0; q < n; ++q) b.j[q] = bn_job(st, *L[q], d ? d[q] : nullptr, st->bn_slot++);
  return b;
}
static void bn_relu_fwd(TrainState* st, const BnMulti& b, int n, hipStream_t s) {
  hipLaunchKernelGGL((bn_stats_kernel<0>), dim3(b.C / 64, (b.M + kBnRows - 1) / kBnRows, n), dim3(256), 0, s, b);
  sync_slots(st->ctx, b.j[0].acc, n, s);
  hipLaunchKernelGGL(bn_apply_fwd_kernel, dim3((unsigned)(((size_t)b.M * b.C + 255) / 256), n), dim3(256), 0, s, b);
}
static void bn_relu_bwd(TrainState* st, const BnMulti& b, int n, hipStream_t s) {
  hipLaunchKernelGGL((bn_stats_kernel<1>), dim3(b.C / 64, (b.M + kBnRows - 1) / kBnRows, n), dim3(256), 0, s, b);
  sync_slots(st->ctx, b.j[0].acc, n, s);
  hipLaunchKernelGGL(bn_apply_bwd_kernel, dim3((unsigned)(((size_t)b.M * b.C + 255) / 256), n), dim3(256), 0, s, b);
}
// F.normalize of n jobs' D-wide rows into (forward) / out of (backward) their slots of the concatenated feature row
template <int D = kTD>
static void rownorm_launch(bool fwd, const RownormJob* j, int n, int M, int Kc, hipStream_t s) {
  RownormMulti rn{};
  rn.M = M;
  rn.ld = Kc;
  for (int q = 0; q < n; ++q) rn.j[q] = j[q];
  if (fwd) hipLaunchKernelGGL(rownorm_fwd_kernel<D>, dim3((M + 3) / 4, n), dim3(256), 0, s, rn);
  else hipLaunchKernelGGL(rownorm_bwd_kernel<D>, dim3((M + 3) / 4, n), dim3(256), 0, s, rn);
}

// ---- the row kernels by run-time width, for callers outside this translation unit (train_common.h: the fine step at 128, the block
// tests at every width). false: no instance of that width — nothing was launched
bool ln_fwd_rows(int D, const float* x, const float* y, int T, const float* gamma, const float* beta, const Drop& dr, float* out, float* xhat,
                 float* rstd, hipStream_t s) {
  if (D == 128) ln_fwd_launch<128>(x, y, T, gamma, beta, dr, out, xhat, rstd, s);
  else if (D == 256) ln_fwd_launch<256>(x, y, T, gamma, beta, dr, out, xhat, rstd, s);
  else if (D == 1024) ln_fwd_launch<1024>(x, y, T, gamma, beta, dr, out, xhat, rstd, s);
  else return false;
  return true;
}
bool ln_bwd_rows(int D, int waves, const float* dout, const float* xhat, const float* rstd, int T, const float* gamma, const Drop& dr,
                 float* d_res, float* d_y, float* dgamma, float* dbeta, hipStream_t s) {
  if (D == 128 && waves == 4) ln_bwd_launch<128, 4>(dout, xhat, rstd, T, gamma, dr, d_res, d_y, dgamma, dbeta, s);
  else if (D == 256 && waves == 16) ln_bwd_launch<256, 16>(dout, xhat, rstd, T, gamma, dr, d_res, d_y, dgamma, dbeta, s);
  else if (D == 256 && waves == 4) ln_bwd_launch<256, 4>(dout, xhat, rstd, T, gamma, dr, d_res, d_y, dgamma, dbeta, s);
  else if (D == 1024 && waves == 4) ln_bwd_launch<1024, 4>(dout, xhat, rstd, T, gamma, dr, d_res, d_y, dgamma, dbeta, s);
  else return false;
  return true;
}
// forward: dst[m] (row stride ld) = normalize(src[m]) (contiguous), the norms to save_n; backward: dst[m] (contiguous) from src = dy
// and y (both row stride ld) and the saved norms. A job list of one, no embedding lookup.
bool rownorm_rows(bool fwd, int D, const float* src, const float* y, float* dst, float* save_n, int M, int ld, hipStream_t s) {
  const RownormJob j{src, nullptr, dst, y, save_n};
  if (D == 128) rownorm_launch<128>(fwd, &j, 1, M, ld, s);
  else if (D == 256) rownorm_launch<256>(fwd, &j, 1, M, ld, s);
  else return false;
  return true;
}

// ---- forward ---------------------------------------------------------------------------------------------------
// one [Linear, BatchNorm1d, ReLU] block that is alone
static void mlp_layer_fwd(TrainState* st, MlpLayer& L, const float* x, int M, hipStream_t s) {
  gemm_nt(x, T_(st, L.prefix + ".0.weight").data, T_(st, L.prefix + ".0.bias").data, L.y, M, L.cout, L.cin, 0, s);
  const MlpLayer* Lp = &L;
  bn_relu_fwd(st, bn_jobs(st, 1, &Lp, nullptr, M), 1, s);
}

// ---- the small feature branches (position, point count, colour: [K -> 64 -> 256] + normalize, identical shapes) stage by stage,
// every stage ONE launch over all of them (kMaxJobs = 3): 7 launches instead of 7 per branch, forward and backward
static SmallkMulti smallk_jobs(int M) {
  SmallkMulti sk{};
  sk.M = M;
  sk.mean = kNumPtsMean;
  sk.stdv = kNumPtsStd;
  sk.rows_per_block = 32;  // (backward; 64 rows per workgroup halve the end-of-workgroup atomics but double the serial row loop: 7.8 -> 10.4 us)
  return sk;
}
static void small_branches_fwd(TrainState* st, const std::vector<int>& which, int M, int Kc, hipStream_t s) {
  const int n = (int)which.size();
  SmallkMulti sk = smallk_jobs(M);
  const float *gx[kMaxJobs], *gw[kMaxJobs], *gb[kMaxJobs];
  float* gy[kMaxJobs];
  RownormJob rn[kMaxJobs];
  const MlpLayer *L0[kMaxJobs], *L1[kMaxJobs];
  for (int q = 0; q < n; ++q) {
    Branch& br = st->branches[which[q]];
    L0[q] = &br.layers[0];
    L1[q] = &br.layers[1];
    sk.j[q].x = br.x;
    sk.j[q].K = br.k_in;
    sk.j[q].standardize = br.standardize;
    sk.j[q].w = T_(st, L0[q]->prefix + ".0.weight").data;
    sk.j[q].b = T_(st, L0[q]->prefix + ".0.bias").data;
    sk.j[q].y = L0[q]->y;
    gx[q] = L0[q]->a;
    gw[q] = T_(st, L1[q]->prefix + ".0.weight").data;
    gb[q] = T_(st, L1[q]->prefix + ".0.bias").data;
    gy[q] = L1[q]->y;
    rn[q] = RownormJob{L1[q]->a, nullptr, st->cat + br.slot * kTD, nullptr, br.save_n};
  }
  const BnMulti b0 = bn_jobs(st, n, L0, nullptr, M);  // (slot order: the first stage's n, then the second's)
  const BnMulti b1 = bn_jobs(st, n, L1, nullptr, M);
  hipLaunchKernelGGL(smallk_fwd_kernel, dim3((M * 64 + 255) / 256, n), dim3(256), 0, s, sk);
  bn_relu_fwd(st, b0, n, s);
  gemm_nt_multi(n, gx, gw, gb, gy, M, kTD, 64, s);
  bn_relu_fwd(st, b1, n, s);
  rownorm_launch(true, rn, n, M, Kc, s);
}
// d2 / d1: [n][M][256] / [n][M][64] scratch (every branch needs its own)
static void small_branches_bwd(TrainState* st, const std::vector<int>& which, int M, int Kc, const float* dcat, float* d2, float* d1,
                               hipStream_t s) {
  const int n = (int)which.size();
  SmallkMulti sk = smallk_jobs(M);
  RownormJob rn[kMaxJobs];
  const MlpLayer *L0[kMaxJobs], *L1[kMaxJobs];
  float *dq2[kMaxJobs], *dq1[kMaxJobs], *gdw[kMaxJobs], *gdb[kMaxJobs];
  const float *gx[kMaxJobs], *gw[kMaxJobs];
  for (int q = 0; q < n; ++q) {
    const Branch& br = st->branches[which[q]];
    L0[q] = &br.layers[0];
    L1[q] = &br.layers[1];
    dq2[q] = d2 + (size_t)q * M * kTD;
    dq1[q] = d1 + (size_t)q * M * 64;
    rn[q] = RownormJob{dcat + br.slot * kTD, nullptr, dq2[q], st->cat + br.slot * kTD, br.save_n};
    gx[q] = L0[q]->a;
    gdw[q] = T_(st, L1[q]->prefix + ".0.weight").grad;
    gdb[q] = T_(st, L1[q]->prefix + ".0.bias").grad;
    gw[q] = T_(st, L1[q]->prefix + ".0.weight").data;
    sk.j[q].x = br.x;
    sk.j[q].K = br.k_in;
    sk.j[q].standardize = br.standardize;
    sk.j[q].dy = dq1[q];
    sk.j[q].dW = T_(st, L0[q]->prefix + ".0.weight").grad;
    sk.j[q].db = T_(st, L0[q]->prefix + ".0.bias").grad;
  }
  const BnMulti b1 = bn_jobs(st, n, L1, dq2, M);  // (slot order: the second stage's n, then the first's)
  const BnMulti b0 = bn_jobs(st, n, L0, dq1, M);
  rownorm_launch(false, rn, n, M, Kc, s);
  bn_relu_bwd(st, b1, n, s);
  gemm_tn_nn_multi(n, dq2, gx, gdw, gdb, gw, dq1, M, kTD, 64, s);
  bn_relu_bwd(st, b0, n, s);
  hipLaunchKernelGGL(smallk_bwd_kernel, dim3((M + 31) / 32, n), dim3(256), 0, s, sk);
}

int train_forward_impl(t2l_ctx* ctx, const t2l_packed_cells* in, float p, uint32_t seed, float* out_emb, hipStream_t s) {
  TrainState* st = state(ctx);
  if (!st) return fail(ctx, T2L_ESTATE, "t2l_encode_cells_train: call t2l_train_bind first");
  if (!in || !out_emb || in->n_cells <= 0 || in->n_objects <= 1 || !in->offsets)
    return fail(ctx, T2L_EINVAL, "t2l_encode_cells_train: bad arguments (BatchNorm batch statistics need >= 2 objects)");
  if (!(p >= 0.f && p < 1.f)) return fail(ctx, T2L_EINVAL, "t2l_encode_cells_train: dropout_p must be in [0,1)");
  const t2l_model_config& c = st->cfg;
  if ((c.use_class && (c.class_embed ? !in->class_idx : !in->pn_feat)) || (c.use_color && (c.color_embed ? !in->color_idx : !in->rgb)) ||
      (c.use_position && !in->center) || (c.use_num && !in->n_pts))
    return fail(ctx, T2L_EINVAL, "t2l_encode_cells_train: a packed input the configuration needs is NULL");
  const int M = in->n_objects, B = in->n_cells, T = B * kTS, Kc = st->n_feat * kTD;
  if ((uint64_t)T * 2 * kTD >= (1ull << 32)) return fail(ctx, T2L_EINVAL, "t2l_encode_cells_train: batch too large for the dropout counters");
  // workspace: generous closed-form bound, grown on demand
  const size_t need_bytes =
      sizeof(float) * ((size_t)M * (2 * Kc + 30 * kTD) + (size_t)T * kTD * 18 +
                       (size_t)c.num_layers * ((size_t)T * (13 * kTD + 8) + (size_t)B * kTH * kTS * kTS) + (size_t)B * kTD * 4) +
      (1 << 20);
  if (need_bytes > st->ws.cap) {
    if (st->ws.base) (void)hipFree(st->ws.base);
    st->ws.base = nullptr;
    st->ws.cap = 0;
    T2L_HIP(ctx, hipMalloc(&st->ws.base, need_bytes));
    st->ws.cap = need_bytes;
  }
  tl_gemm_bf16 = ctx->train_bf16;
  tl_gemm_block64 = ctx->train_gemm_block == 64 || (ctx->train_gemm_block == 0 && ctx->train_bf16 != 0);
  st->ws.off = 0;
  st->have_forward = false;
  st->M = M; st->B = B; st->T = T;
  st->offsets = in->offsets;
  st->seed = seed;
  st->p = p;
  st->branches.clear();
  st->layers.clear();
  event_begin(ctx, "train_forward", s);
  st->bn_slot = 0;
  // the accumulators are cleared by the previous forward's last launch (pool_norm_fwd_kernel); a memset only the first time or after
  // a forward that did not get that far
  ctx->sync_failed = false;
  if (!st->fwd_acc_clean) T2L_HIP(ctx, hipMemsetAsync(acc_base(ctx, st), 0, sizeof(double) * kBnStride * kBnSlots, s));
  st->fwd_acc_clean = false;

  st->cat = st->ws.take<float>((size_t)M * Kc);
  const std::string oe = "object_encoder.";
  int slot = 0;
  std::vector<int> smalls;  // indices of the small branches: launched together below, one launch per stage
  auto small_branch = [&](const std::string& name, const float* x, int k, int standardize) {
    Branch br;
    br.kind = 1; br.slot = slot++; br.x = x; br.k_in = k; br.standardize = standardize;
    br.layers.push_back(make_layer(st, oe + name + ".0", k, 64, M));
    br.layers.push_back(make_layer(st, oe + name + ".1", 64, kTD, M));
    br.save_n = st->ws.take<float>(M);
    smalls.push_back((int)st->branches.size());
    st->branches.push_back(br);
  };
  std::vector<int> embeds;  // the embedding lookups: one launch for both tables
  auto embed_branch = [&](const std::string& table, const int32_t* idx) {
    Branch br;
    br.kind = 0; br.slot = slot++; br.table = oe + table; br.idx = idx;
    br.save_n = st->ws.take<float>(M);
    embeds.push_back((int)st->branches.size());
    st->branches.push_back(br);
  };
  if (c.use_class) {
    if (c.class_embed) {
      embed_branch("class_embedding.weight", in->class_idx);
    } else {  // PointNet++ features2 -> mlp_pointnet (object_encoder.py:86-99,112)
      Branch br;
      br.kind = 2; br.slot = slot++; br.x = in->pn_feat; br.k_in = 256;
      br.layers.push_back(make_layer(st, oe + "mlp_pointnet.0", 256, kTD, M));
      br.save_n = st->ws.take<float>(M);
      mlp_layer_fwd(st, br.layers[0], in->pn_feat, M, s);
      const RownormJob rn{br.layers[0].a, nullptr, st->cat + br.slot * kTD, nullptr, br.save_n};
      rownorm_launch(true, &rn, 1, M, Kc, s);
      st->branches.push_back(br);
    }
  }
  if (c.use_color) {
    if (c.color_embed) embed_branch("color_embedding.weight", in->color_idx);
    else small_branch("color_encoder", in->rgb, 3, 0);
  }
  if (c.use_position) small_branch("pos_encoder", in->center, 3, 0);
  if (c.use_num) small_branch("num_encoder", in->n_pts, 1, 1);
  if (!embeds.empty()) {
    RownormJob rn[kMaxJobs];
    for (size_t q = 0; q < embeds.size(); ++q) {
      const Branch& br = st->branches[embeds[q]];
      rn[q] = RownormJob{T_(st, br.table).data, br.idx, st->cat + br.slot * kTD, nullptr, br.save_n};
    }
    rownorm_launch(true, rn, (int)embeds.size(), M, Kc, s);
  }
  if (!smalls.empty()) small_branches_fwd(st, smalls, M, Kc, s);

  st->merge = make_layer(st, oe + "mlp_merge.0", Kc, kTD, M);
  mlp_layer_fwd(st, st->merge, st->cat, M, s);
  st->X0 = st->ws.take<float>((size_t)T * kTD);
  st->save_nf = st->ws.take<float>(M);
  hipLaunchKernelGGL(scatter_norm_fwd_kernel, dim3((T + 3) / 4), dim3(256), 0, s, st->merge.a, in->offsets, B, st->X0, st->save_nf);

  float* tmp = st->ws.take<float>((size_t)T * kTD);
  const float* x = st->X0;
  const Products pr{ctx, false};  // the object branch's products are the tile-per-workgroup ones of gemm_f32.h
  for (int l = 0; l < c.num_layers; ++l) {
    EncLayer L;
    L.prefix = "obj_inter_module." + std::to_string(l);
    L.T = T; L.B = B; L.S = kTS; L.FF = 2 * kTD; L.site0 = 4 * l; L.x_in = x;
    enc_layer_alloc<kTD>(st->ws, L, p);
    enc_layer_fwd<kTD>(pr, st->t, L, seed, p, tmp, s);
    x = L.x2;
    st->layers.push_back(L);
  }
  st->out = st->ws.take<float>((size_t)B * kTD);
  st->pool_n = st->ws.take<float>(B);
  st->pool_arg = st->ws.take<int32_t>((size_t)B * kTD);
  pool_norm_fwd_launch(x, st->out, st->pool_arg, st->pool_n, out_emb, acc_base(ctx, st), kBnStride * kBnSlots * 2, B, s);
  event_end(ctx, "train_forward", s);
  T2L_HIP(ctx, hipGetLastError());
  st->fwd_acc_clean = true;
  st->bwd_acc_clean = true;
  if (st->ws.off > st->ws.cap) return fail(ctx, T2L_ENOMEM, "t2l_encode_cells_train: workspace bound exceeded (internal error)");
  if (ctx->sync_failed) return fail(ctx, T2L_ESTATE, "t2l_encode_cells_train: the cross-rank sum callback (t2l_train_sync_bn) failed");
  st->have_forward = true;
  return T2L_OK;
}

// ---- backward --------------------------------------------------------------------------------------------------
// d: gradient w.r.t. the block's ReLU output [M,cout] (overwritten); x: the block's input; dx (optional) receives d W.
static void mlp_layer_bwd(TrainState* st, const MlpLayer& L, float* d, const float* x, int M, float* dx, hipStream_t s) {
  const MlpLayer* Lp = &L;
  bn_relu_bwd(st, bn_jobs(st, 1, &Lp, &d, M), 1, s);
  const TTensor &W = T_(st, L.prefix + ".0.weight"), &b = T_(st, L.prefix + ".0.bias");
  if (dx) gemm_tn_nn(d, x, W.grad, b.grad, W.data, dx, M, L.cout, L.cin, 0, nullptr, nullptr, s);
  else gemm_tn(d, x, W.grad, b.grad, M, L.cout, L.cin, s);
}

int train_backward_impl(t2l_ctx* ctx, const float* grad_emb, float* grad_pn_feat, hipStream_t s) {
  TrainState* st = state(ctx);
  if (!st || !st->have_forward) return fail(ctx, T2L_ESTATE, "t2l_encode_cells_backward: no forward pass to differentiate");
  if (!grad_emb) return fail(ctx, T2L_EINVAL, "t2l_encode_cells_backward: null gradient");
  const int M = st->M, B = st->B, T = st->T, Kc = st->n_feat * kTD;
  tl_gemm_bf16 = ctx->train_bf16;
  tl_gemm_block64 = ctx->train_gemm_block == 64 || (ctx->train_gemm_block == 0 && ctx->train_bf16 != 0);
  const size_t mark = st->ws.off;
  event_begin(ctx, "train_backward", s);
  st->bn_slot = kBnSlots;  // the backward's half of the accumulators: zeroed by the forward's memset, unless this is a second backward
  ctx->sync_failed = false;
  if (!st->bwd_acc_clean)
    T2L_HIP(ctx, hipMemsetAsync(acc_base(ctx, st) + (size_t)kBnSlots * kBnStride, 0, sizeof(double) * kBnStride * kBnSlots, s));
  st->bwd_acc_clean = false;
  float* dcur = st->ws.take<float>((size_t)T * kTD);
  // the layers' scratch is taken ONCE and shared by all of them: taken per layer (as the text head does for its two layers of
  // different shape) it would add 10 T kTD floats per layer, which the forward's workspace bound does not hold
  EncScratch sc = enc_scratch_take<kTD>(st->ws, T, 2 * kTD);
  float* dfeat = st->ws.take<float>((size_t)M * kTD);
  float* dcat = st->ws.take<float>((size_t)M * Kc);
  float* d2 = st->ws.take<float>((size_t)kMaxJobs * M * kTD);  // scratch of the feature branches: one region per small branch (they run
  float* d1 = st->ws.take<float>((size_t)kMaxJobs * M * 64);   // together, stage by stage); the others use region 0 one after the other
  if (st->ws.off > st->ws.cap) {
    st->ws.off = mark;
    return fail(ctx, T2L_ENOMEM, "t2l_encode_cells_backward: workspace bound exceeded (internal error)");
  }
  pool_norm_bwd_launch(grad_emb, st->out, st->pool_arg, st->pool_n, dcur, B, s);
  const Products pr{ctx, false};
  for (int l = (int)st->layers.size() - 1; l >= 0; --l) {
    float* dx = enc_layer_bwd<kTD, 16>(pr, st->t, st->layers[l], st->seed, st->p, sc, dcur, true, s);
    sc.dC = dcur;  // (the layer's input gradient lives in the scratch's dC: the consumed dcur takes its place)
    dcur = dx;
  }
  // tokens -> objects, merge MLP
  hipLaunchKernelGGL(scatter_norm_bwd_kernel, dim3((M + 3) / 4), dim3(256), 0, s, dcur, st->X0, st->save_nf, st->offsets, B, M, dfeat);
  mlp_layer_bwd(st, st->merge, dfeat, st->cat, M, dcat, s);
  {  // embedding tables: normalize-backward of both slots in one launch, then the per-row sums of both tables in one
    RownormJob rn[kMaxJobs];
    EmbedSumMulti es{};
    es.M = M;
    int ne = 0, max_rows = 0;
    for (const Branch& br : st->branches) {
      if (br.kind != 0) continue;
      float* dq = d2 + (size_t)ne * M * kTD;
      rn[ne] = RownormJob{dcat + br.slot * kTD, nullptr, dq, st->cat + br.slot * kTD, br.save_n};
      es.g[ne] = dq;
      es.idx[ne] = br.idx;
      es.dtable[ne] = T_(st, br.table).grad;
      es.rows[ne] = (int)(T_(st, br.table).numel / kTD);
      max_rows = std::max(max_rows, es.rows[ne]);
      ++ne;
    }
    if (ne) {
      rownorm_launch(false, rn, ne, M, Kc, s);
      if (max_rows > 1) hipLaunchKernelGGL(embed_sum_kernel, dim3(max_rows - 1, kEmbSplit, ne), dim3(256), 0, s, es);
    }
  }
  for (const Branch& br : st->branches) {
    if (br.kind != 2) continue;  // the PointNet++-feature branch: one [256 -> 256] block
    const RownormJob rn{dcat + br.slot * kTD, nullptr, d2, st->cat + br.slot * kTD, br.save_n};
    rownorm_launch(false, &rn, 1, M, Kc, s);
    mlp_layer_bwd(st, br.layers[0], d2, br.x, M, grad_pn_feat, s);
  }
  {
    std::vector<int> smalls;
    for (size_t i = 0; i < st->branches.size(); ++i)
      if (st->branches[i].kind == 1) smalls.push_back((int)i);
    if (!smalls.empty()) small_branches_bwd(st, smalls, M, Kc, dcat, d2, d1, s);
  }
  event_end(ctx, "train_backward", s);
  st->ws.off = mark;
  T2L_HIP(ctx, hipGetLastError());
  if (ctx->sync_failed) return fail(ctx, T2L_ESTATE, "t2l_encode_cells_backward: the cross-rank sum callback (t2l_train_sync_bn) failed");
  return T2L_OK;
}

int adam_step_impl(t2l_ctx* ctx, float lr, float b1, float b2, float eps, hipStream_t s) {
  TrainState* st = state(ctx);
  if (!st) return fail(ctx, T2L_ESTATE, "t2l_adam_step: call t2l_train_bind first");
  st->step += 1;
  // the backbone's tensors step only when its backward added into their gradients since the last zero_grad (a batch that
  // passed precomputed features2 leaves them untouched: torch.optim.Adam would skip .grad = None parameters, not decay them)
  const int n_chunks = st->adam.plan.n_chunks();
  const bool pn = st->pn_chunk0 < n_chunks && st->pn_touched;
  if (pn) st->step_pn += 1;
  event_begin(ctx, "adam_step", s);
  if (pn && st->step_pn == st->step) {
    st->adam.launch(0, n_chunks, st->step, lr, b1, b2, eps, s);
  } else {
    st->adam.launch(0, st->pn_chunk0, st->step, lr, b1, b2, eps, s);
    if (pn) st->adam.launch(st->pn_chunk0, n_chunks, st->step_pn, lr, b1, b2, eps, s);
  }
  event_end(ctx, "adam_step", s);
  T2L_HIP(ctx, hipGetLastError());
  return T2L_OK;
}

int adam_state_impl(t2l_ctx* ctx, int set, float* m, float* v, int64_t* step, int64_t* numel, hipStream_t s) {
  TrainState* st = state(ctx);
  if (!st) return fail(ctx, T2L_ESTATE, "t2l_adam_state: call t2l_train_bind first");
  const int rc = st->adam.state(ctx, "t2l_adam_state", set, m, v, step, numel, st->step | (st->step_pn << 32), s);
  if (rc == T2L_OK && set && m) {
    st->step = *step & 0xFFFFFFFFll;
    st->step_pn = st->pn_chunk0 < st->adam.plan.n_chunks() ? (*step >> 32) : 0;
  }
  return rc;
}

int zero_grad_impl(t2l_ctx* ctx, hipStream_t s) {
  TrainState* st = state(ctx);
  if (!st) return fail(ctx, T2L_ESTATE, "t2l_zero_grad: call t2l_train_bind first");
  st->adam.zero(s);
  st->pn_touched = false;
  T2L_HIP(ctx, hipGetLastError());
  return T2L_OK;
}

// =================================================================================================================
// The TEXT head in training mode (SURVEY.md 8 f-4 / a9's other half): LanguageEncoder.forward downstream of the frozen T5's
// hidden states under model.train() (models/language_encoder.py:127-147 as run by training/coarse.py:44,55-56 — the published
// command trains this head: --fixed_embedding freezes T5 only, README.md:87-99):
//   hidden [n_sent, L, 1024] -> TransformerEncoderLayer(1024, 4 heads, ff 4096; the four dropout sites live) over the L tokens ->
//   max over tokens -> Linear(1024 -> 256) + BatchNorm1d with the statistics of THIS batch of sentences (running buffers
//   updated) -> view [n_desc, S, 256] -> x += TransformerEncoderLayer(256, 4 heads, ff 1024)(x) over the S sentences -> max
//   over the sentences -> out [n_desc, 256]  (F.normalize stays with the caller: cell_retrieval.py:57-63).
// The FINE head (LanguageEncoder(is_fine=True), fine_embed_dim 128: language_encoder.py:137-141) is the same pipeline cut off behind
// the BatchNorm at width 128: bound without inter_module tensors, out [n_sent, 128], the backward starts at the BatchNorm.
// Forward keeps the activations; backward accumulates (+=) into the bound .grad buffers — the parameters stay torch's and are
// stepped by t2l_text_adam_step (one launch over the 13.6 M head parameters; torch.optim.Adam when the caller prefers). The same
// modular f32 kernels as the object branch (gemm_f32.h products, option train_bf16 for bf16 / split-bf16 operands), and its
// transformer layer (enc_layer_* above) with the products descriptor that lets a product run on the tiled GEMM.
// =================================================================================================================
struct TextTrain {
  t2l_ctx* ctx = nullptr;
  TensorMap t;
  std::string prefix;
  Arena ws;
  bool have_forward = false;
  int n_sent = 0, L = 0, n_desc = 0, S = 0;
  int D = 256;        // width of inter_mlp: 256 (the coarse head) or 128 (the fine head)
  bool fine = false;  // the fine layout: no inter_module, the head ends behind inter_mlp's BatchNorm (out [n_sent, D])
  float p = 0.f;
  uint32_t seed = 0;
  EncLayer intra, inter;
  float *pooled = nullptr, *mlp_y = nullptr, *mlp_out = nullptr, *bn_mean = nullptr, *bn_rstd = nullptr, *out = nullptr;
  int32_t *tok_arg = nullptr, *sent_arg = nullptr;
  AdamSet adam;  // over the head's parameters, in bind order (t2l_text_adam_step)
  int64_t step = 0;
};
static TextTrain* tstate(t2l_ctx* ctx) { return reinterpret_cast<TextTrain*>(ctx->text_train); }
void free_text_train(t2l_ctx* ctx) {
  TextTrain* st = tstate(ctx);
  if (!st) return;
  st->adam.release();
  if (st->ws.base) (void)hipFree(st->ws.base);
  delete st;
  ctx->text_train = nullptr;
}
static const TTensor& TT(TextTrain* st, const std::string& n) { return st->t.at(st->prefix + n); }

__global__ void add_inplace_kernel(float* __restrict__ a, const float* __restrict__ b, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) a[i] += b[i];
}

// inter_mlp's BatchNorm (no ReLU behind it) over the n_sent rows of mlp_y; PHASE, acc: bn_plain_fwd_kernel
template <int PHASE>
static void text_bn_fwd(TextTrain* st, double* acc, hipStream_t s) {
  hipLaunchKernelGGL((bn_plain_fwd_kernel<PHASE>), dim3(st->D / 4), dim3(256), 0, s, (const float*)st->mlp_y, st->n_sent, st->D,
                     TT(st, "inter_mlp.0.1.weight").data, TT(st, "inter_mlp.0.1.bias").data, TT(st, "inter_mlp.0.1.running_mean").data,
                     TT(st, "inter_mlp.0.1.running_var").data, 0.1f, st->mlp_out, st->bn_mean, st->bn_rstd, acc);
}
template <int PHASE>
static void text_bn_bwd(TextTrain* st, float* dX, double* acc, hipStream_t s) {
  hipLaunchKernelGGL((bn_plain_bwd_kernel<PHASE>), dim3(st->D / 4), dim3(256), 0, s, dX, (const float*)st->mlp_y, st->n_sent, st->D,
                     TT(st, "inter_mlp.0.1.weight").data, (const float*)st->bn_mean, (const float*)st->bn_rstd,
                     TT(st, "inter_mlp.0.1.weight").grad, TT(st, "inter_mlp.0.1.bias").grad, acc);
}

static int text_train_bind_body(t2l_ctx* ctx, const t2l_train_tensor* tensors, int n, const char* prefix) {
  if (!tensors || n <= 0) return fail(ctx, T2L_EINVAL, "t2l_text_train_bind: null argument");
  // a re-bind of the same parameter list (moved storage: model.to(), re-assigned .grad) keeps the optimizer state, as t2l_train_bind does
  AdamSet::Old old;
  int64_t old_step = 0;
  if (TextTrain* o = tstate(ctx)) {
    o->adam.detach(old);
    old_step = o->step;
  }
  free_text_train(ctx);
  TextTrain* st = new TextTrain();
  ctx->text_train = st;
  st->ctx = ctx;
  st->prefix = prefix ? prefix : "language_encoder.";
  for (int i = 0; i < n; ++i) {
    if (!tensors[i].name || !tensors[i].data) return fail(ctx, T2L_EINVAL, "t2l_text_train_bind: null name/data");
    st->t[tensors[i].name] = TTensor{tensors[i].data, tensors[i].grad, tensors[i].numel};
  }
  auto need_t = [&](const std::string& name, int64_t numel, bool grad) -> int {
    auto it = st->t.find(st->prefix + name);
    if (it == st->t.end() || it->second.numel != numel || (grad && !it->second.grad))
      return fail(ctx, T2L_EINVAL, "t2l_text_train_bind: tensor '" + st->prefix + name + "' missing, mis-sized or without a gradient buffer "
                                   "(the engine trains the two published heads: the coarse one — intra_module 1 x (1024, 4 heads, 4096), "
                                   "inter_mlp 1024 -> 256, inter_module 1 x (256, 4 heads, 1024) — and the fine one — the same intra_module, "
                                   "inter_mlp 1024 -> 128, no inter_module tensors at all)");
    return T2L_OK;
  };
  int rc;
  auto layer = [&](const std::string& lp, int64_t D, int64_t FF) -> int {
    const std::pair<const char*, int64_t> req[] = {{".self_attn.in_proj_weight", 3 * D * D}, {".self_attn.in_proj_bias", 3 * D},
                                                   {".self_attn.out_proj.weight", D * D},    {".self_attn.out_proj.bias", D},
                                                   {".linear1.weight", FF * D},              {".linear1.bias", FF},
                                                   {".linear2.weight", D * FF},              {".linear2.bias", D},
                                                   {".norm1.weight", D},                     {".norm1.bias", D},
                                                   {".norm2.weight", D},                     {".norm2.bias", D}};
    for (auto& r : req)
      if ((rc = need_t(lp + r.first, r.second, true))) return rc;
    return T2L_OK;
  };
  // the layout follows from the names alone: ANY <prefix>inter_module.* tensor asks for the coarse head (and then all of
  // inter_module.0 must be there at 256 / 1024); none at all asks for the fine head, whose inter_mlp is 128 wide
  st->fine = true;
  for (auto& kv : st->t)
    if (kv.first.compare(0, st->prefix.size() + 13, st->prefix + "inter_module.") == 0) st->fine = false;
  st->D = st->fine ? 128 : 256;
  const int64_t D = st->D;
  if ((rc = layer("intra_module.0", 1024, 4096)) || (!st->fine && (rc = layer("inter_module.0", 256, 1024)))) return rc;
  if ((rc = need_t("inter_mlp.0.0.weight", D * 1024, true)) || (rc = need_t("inter_mlp.0.0.bias", D, true)) ||
      (rc = need_t("inter_mlp.0.1.weight", D, true)) || (rc = need_t("inter_mlp.0.1.bias", D, true)) ||
      (rc = need_t("inter_mlp.0.1.running_mean", D, false)) || (rc = need_t("inter_mlp.0.1.running_var", D, false)))
    return rc;
  for (int i = 0; i < n; ++i)  // Adam over every bound tensor that has a gradient buffer, in bind order (each is in st->t: inserted above)
    if (tensors[i].grad) st->adam.names.push_back(tensors[i].name);
  bool kept;
  if ((rc = st->adam.build(ctx, st->t, old, &kept))) return rc;
  if (kept) st->step = old_step;
  attn256_allow_lds(ctx->device);
  return T2L_OK;
}

int text_train_bind_impl(t2l_ctx* ctx, const t2l_train_tensor* tensors, int n, const char* prefix) {
  const int rc = text_train_bind_body(ctx, tensors, n, prefix);
  if (rc != T2L_OK) free_text_train(ctx);  // a refused bind leaves nothing half-bound behind: the next forward reports "bind first"
  return rc;
}

int text_train_forward_impl(t2l_ctx* ctx, const float* hidden, int n_sent, int L, int n_desc, float p, uint32_t seed, float* out, hipStream_t s) {
  TextTrain* st = tstate(ctx);
  if (!st) return fail(ctx, T2L_ESTATE, "t2l_text_head_train: call t2l_text_train_bind first");
  if (!hidden || !out) return fail(ctx, T2L_EINVAL, "t2l_text_head_train: null buffer");
  if (n_desc < 1 || n_sent < n_desc || n_sent % n_desc) return fail(ctx, T2L_EINVAL, "t2l_text_head_train: the sentences must split evenly over the descriptions");
  const int S = n_sent / n_desc;
  if (L < 1 || L > 32 || S > 32) return fail(ctx, T2L_EINVAL, "t2l_text_head_train: need 1 <= n_tokens <= 32 and <= 32 sentences per description");
  if (!(p >= 0.f && p < 1.f)) return fail(ctx, T2L_EINVAL, "t2l_text_head_train: dropout_p must be in [0, 1)");
  tl_gemm_bf16 = ctx->text_train_bf16;
  tl_gemm_block64 = ctx->train_gemm_block == 64 || (ctx->train_gemm_block == 0 && ctx->text_train_bf16 != 0);
  const size_t T1 = (size_t)n_sent * L;
  // saved activations + the backward's scratch: ~31 floats per (row, column) of each layer, see enc_layer_alloc / enc_scratch_take
  const size_t need = sizeof(float) * (32 * (T1 * 1024 + (size_t)n_sent * 256) + 2 * (size_t)n_sent * 4 * L * L + 2 * (size_t)n_desc * 4 * S * S +
                                       8 * (size_t)n_sent * 1024 + 16 * (size_t)n_desc * 256) + (1 << 20);
  if (st->ws.cap < need) {
    if (st->ws.base) T2L_HIP(ctx, hipFree(st->ws.base));
    st->ws.base = nullptr;
    st->ws.cap = 0;
    T2L_HIP(ctx, hipMalloc(&st->ws.base, need));
    st->ws.cap = need;
  }
  st->ws.off = 0;
  st->have_forward = false;
  st->n_sent = n_sent; st->L = L; st->n_desc = n_desc; st->S = S; st->p = p; st->seed = seed;
  event_begin(ctx, "text_train_forward", s);
  float* tmp = st->ws.take<float>(T1 * 1024);
  const Products pr{ctx, true};
  EncLayer& A = st->intra;
  A = EncLayer{};
  A.prefix = st->prefix + "intra_module.0"; A.T = (int)T1; A.B = n_sent; A.S = L; A.FF = 4096; A.site0 = 0; A.x_in = hidden;
  enc_layer_alloc<1024>(st->ws, A, p);
  enc_layer_fwd<1024>(pr, st->t, A, seed, p, tmp, s);
  st->pooled = st->ws.take<float>((size_t)n_sent * 1024);
  st->tok_arg = st->ws.take<int32_t>((size_t)n_sent * 1024);
  seq_max_fwd_launch(A.x2, nullptr, n_sent, L, 1024, st->pooled, st->tok_arg, s);
  const int D = st->D;
  st->mlp_y = st->ws.take<float>((size_t)n_sent * D);
  st->mlp_out = st->ws.take<float>((size_t)n_sent * D);
  st->bn_mean = st->ws.take<float>(D);
  st->bn_rstd = st->ws.take<float>(D);
  // (D = 128 is no multiple of the fast GEMM's 256-column tile: the fine head's Linear runs on the gemm_f32.h product, same operands)
  t_gemm_nt(pr, st->pooled, TT(st, "inter_mlp.0.0.weight").data, TT(st, "inter_mlp.0.0.bias").data, st->mlp_y, n_sent, D, 1024, 0, s);
  if (ctx->sync_fn) {  // statistics | sum over the ranks | apply (t2l_train_sync_bn)
    double* acc = ctx->sync_buf + (size_t)(2 * kBnSlots) * kBnStride;
    ctx->sync_failed = false;
    text_bn_fwd<1>(st, acc, s);
    sync_slots(ctx, acc, 1, s);
    text_bn_fwd<2>(st, acc, s);
  } else {
    text_bn_fwd<0>(st, nullptr, s);
  }
  if (st->fine) {  // the fine head ends here: one vector per hint, viewed [n_desc, S, D] by the caller (language_encoder.py:137-141)
    T2L_HIP(ctx, hipMemcpyAsync(out, st->mlp_out, sizeof(float) * (size_t)n_sent * D, hipMemcpyDeviceToDevice, s));
    event_end(ctx, "text_train_forward", s);
    T2L_HIP(ctx, hipGetLastError());
    if (st->ws.off > st->ws.cap) return fail(ctx, T2L_ENOMEM, "t2l_text_head_train: workspace bound exceeded (internal error)");
    if (ctx->sync_failed) return fail(ctx, T2L_ESTATE, "t2l_text_head_train: the cross-rank sum callback (t2l_train_sync_bn) failed");
    st->have_forward = true;
    return T2L_OK;
  }
  EncLayer& I = st->inter;
  I = EncLayer{};
  I.prefix = st->prefix + "inter_module.0"; I.T = n_sent; I.B = n_desc; I.S = S; I.FF = 1024; I.site0 = 4; I.x_in = st->mlp_out;
  enc_layer_alloc<256>(st->ws, I, p);
  enc_layer_fwd<256>(pr, st->t, I, seed, p, tmp, s);
  st->out = st->ws.take<float>((size_t)n_desc * 256);
  st->sent_arg = st->ws.take<int32_t>((size_t)n_desc * 256);
  seq_max_fwd_launch(I.x2, st->mlp_out, n_desc, S, 256, st->out, st->sent_arg, s);
  T2L_HIP(ctx, hipMemcpyAsync(out, st->out, sizeof(float) * (size_t)n_desc * 256, hipMemcpyDeviceToDevice, s));
  event_end(ctx, "text_train_forward", s);
  T2L_HIP(ctx, hipGetLastError());
  if (st->ws.off > st->ws.cap) return fail(ctx, T2L_ENOMEM, "t2l_text_head_train: workspace bound exceeded (internal error)");
  if (ctx->sync_failed) return fail(ctx, T2L_ESTATE, "t2l_text_head_train: the cross-rank sum callback (t2l_train_sync_bn) failed");
  st->have_forward = true;
  return T2L_OK;
}

int text_train_backward_impl(t2l_ctx* ctx, const float* grad_out, hipStream_t s) {
  TextTrain* st = tstate(ctx);
  if (!st || !st->have_forward) return fail(ctx, T2L_ESTATE, "t2l_text_head_backward: no forward pass to differentiate");
  if (!grad_out) return fail(ctx, T2L_EINVAL, "t2l_text_head_backward: null gradient");
  tl_gemm_bf16 = ctx->text_train_bf16;
  tl_gemm_block64 = ctx->train_gemm_block == 64 || (ctx->train_gemm_block == 0 && ctx->text_train_bf16 != 0);
  const size_t mark = st->ws.off;
  const Products pr{ctx, true};
  const int n_sent = st->n_sent, n_desc = st->n_desc, S = st->S, L = st->L;
  const int D = st->D;
  event_begin(ctx, "text_train_backward", s);
  float* dX;
  if (st->fine) {  // grad_out IS the gradient behind the BatchNorm; its backward works in place, so on a copy
    dX = st->ws.take<float>((size_t)n_sent * D);
    T2L_HIP(ctx, hipMemcpyAsync(dX, grad_out, sizeof(float) * (size_t)n_sent * D, hipMemcpyDeviceToDevice, s));
  } else {
    // max over the sentences: the gradient goes to the arg-max row of (x + layer(x)) — to the layer's output AND to the residual x
    float* dY2 = st->ws.take<float>((size_t)n_sent * 256);
    seq_max_bwd_launch(grad_out, st->sent_arg, n_desc, S, 256, dY2, s);
    dX = enc_layer_bwd<256, 4>(pr, st->t, st->inter, st->seed, st->p, enc_scratch_take<256>(st->ws, n_sent, 1024), dY2, true, s);
    hipLaunchKernelGGL(add_inplace_kernel, dim3((unsigned)(((size_t)n_sent * 256 + 255) / 256)), dim3(256), 0, s, dX, (const float*)dY2, (size_t)n_sent * 256);
  }
  // inter_mlp: BatchNorm (batch statistics), Linear
  if (ctx->sync_fn) {
    double* acc = ctx->sync_buf + (size_t)(2 * kBnSlots + 1) * kBnStride;
    ctx->sync_failed = false;
    text_bn_bwd<1>(st, dX, acc, s);
    sync_slots(ctx, acc, 1, s);
    text_bn_bwd<2>(st, dX, acc, s);
  } else {
    text_bn_bwd<0>(st, dX, nullptr, s);
  }
  float* dpool = st->ws.take<float>((size_t)n_sent * 1024);
  t_gemm_tn_nn(pr, dX, st->pooled, TT(st, "inter_mlp.0.0.weight").grad, TT(st, "inter_mlp.0.0.bias").grad, TT(st, "inter_mlp.0.0.weight").data, dpool,
               n_sent, D, 1024, 0, nullptr, nullptr, s);
  // max over the tokens, then the d = 1024 layer (its input, T5's hidden states, is a constant: no dX)
  float* dX2 = st->ws.take<float>((size_t)n_sent * L * 1024);
  seq_max_bwd_launch(dpool, st->tok_arg, n_sent, L, 1024, dX2, s);
  enc_layer_bwd<1024, 4>(pr, st->t, st->intra, st->seed, st->p, enc_scratch_take<1024>(st->ws, n_sent * L, 4096), dX2, false, s);
  event_end(ctx, "text_train_backward", s);
  const bool over = st->ws.off > st->ws.cap;
  st->ws.off = mark;
  T2L_HIP(ctx, hipGetLastError());
  if (over) return fail(ctx, T2L_ENOMEM, "t2l_text_head_backward: workspace bound exceeded (internal error)");
  if (ctx->sync_failed) return fail(ctx, T2L_ESTATE, "t2l_text_head_backward: the cross-rank sum callback (t2l_train_sync_bn) failed");
  return T2L_OK;
}

// ---- the head's optimizer: torch.optim.Adam's arithmetic (adam_kernel) over every bound parameter in ONE launch
int text_adam_step_impl(t2l_ctx* ctx, float lr, float b1, float b2, float eps, hipStream_t s) {
  TextTrain* st = tstate(ctx);
  if (!st) return fail(ctx, T2L_ESTATE, "t2l_text_adam_step: call t2l_text_train_bind first");
  st->step += 1;
  event_begin(ctx, "text_adam_step", s);
  st->adam.launch(0, st->adam.plan.n_chunks(), st->step, lr, b1, b2, eps, s);
  event_end(ctx, "text_adam_step", s);
  T2L_HIP(ctx, hipGetLastError());
  return T2L_OK;
}

int text_zero_grad_impl(t2l_ctx* ctx, hipStream_t s) {
  TextTrain* st = tstate(ctx);
  if (!st) return fail(ctx, T2L_ESTATE, "t2l_text_zero_grad: call t2l_text_train_bind first");
  st->adam.zero(s);
  T2L_HIP(ctx, hipGetLastError());
  return T2L_OK;
}

int text_adam_state_impl(t2l_ctx* ctx, int set, float* m, float* v, int64_t* step, int64_t* numel, hipStream_t s) {
  TextTrain* st = tstate(ctx);
  if (!st) return fail(ctx, T2L_ESTATE, "t2l_text_adam_state: call t2l_text_train_bind first");
  const int rc = st->adam.state(ctx, "t2l_text_adam_state", set, m, v, step, numel, st->step, s);
  if (rc == T2L_OK && set && m) st->step = *step;
  return rc;
}

}  // namespace t2l

#include "pointnet_train.h"
