// Dev-only block library (libt2l_blocks.so; never shipped, not part of include/t2l.h): the training step's products and layer kernels
// one launch at a time, so that tests/test_gpu_train_blocks.py can hold each against a float64 reference element by element.
// This translation unit IS train.hip plus the wrappers below: it reaches the step's own static launchers (gemm_nt_args, gemm_nn,
// gemm_tn, gemm_tn_nn, gemm_nt_multi, gemm_tn_nn_multi, attn_*_launch, pool_norm_*_launch), the launchers it shares with the fine step
// (train_common.h: ln_*_rows, rownorm_rows, seq_max_*_launch, drop_fwd_launch, relu_drop_bwd_launch — one width switch for everybody)
// and the thread-local operand arithmetic / block option they read. No grid expression lives here.
//
// Every wrapper takes device pointers and refuses, with -1 and a message (t2l_blk_last_error), any shape outside the contract of the
// kernel it launches BEFORE it launches (gemm_f32.h's header, train_kernels.h): a mistaken test gets an error, never an out-of-bounds
// launch. Return: 0, -1 (refused), -2 (the HIP runtime reported an error; the launch is synchronised before the wrapper returns).
//   arith: 0 f32, 1 bf16, 2 split-bf16 operands (GemmArgs::bf16);  block: 1 = 64 x 64 output blocks where the shape allows
//   (seed, site, p): the dropout site, through make_drop
#include "train.hip"
#include "blocks_common.h"

namespace t2l {

static thread_local std::string tl_blk_error;

int blk_refuse(const std::string& msg) {  // (shared with pointnet_blocks.hip)
  tl_blk_error = msg;
  return -1;
}
int blk_finish(const char* who) {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess) {
    tl_blk_error = std::string(who) + ": " + hipGetErrorString(e);
    return -2;
  }
  return 0;
}

namespace {

int refuse(const std::string& msg) { return blk_refuse(msg); }
int finish(const char* who) { return blk_finish(who); }
bool bad_option(int arith, int block, float p) { return arith < 0 || arith > 2 || block < 0 || block > 1 || !(p >= 0.f && p < 1.f); }
void set_options(int arith, int block) {
  tl_gemm_bf16 = arith;
  tl_gemm_block64 = block;
}
const char* kOptions = ": arith must be 0, 1 or 2, block 0 or 1, p in [0, 1)";
const char* kMult32 = ": every output width must be a multiple of 32 (gemm_f32.h: N, and M too when !A_KC)";
const char* kMult16 = ": a k-contiguous operand needs a reduction length that is a multiple of 16 (gemm_f32.h)";

}  // namespace
}  // namespace t2l

using namespace t2l;

extern "C" {

const char* t2l_blk_last_error() { return tl_blk_error.c_str(); }

// Y[M,N] = X[M,K] W[N,K]^T (+ b) (relu); epi == 1: through gemm_nt_args as linear1 does — Y = the ReLU output, Y2 = the same after dropout
int t2l_blk_gemm_nt(const float* X, const float* W, const float* b, float* Y, float* Y2, int M, int N, int K, int relu, int epi, int arith,
                    int block, uint32_t seed, int site, float p) {
  const std::string who = "t2l_blk_gemm_nt";
  if (bad_option(arith, block, p) || (epi != 0 && epi != 1)) return refuse(who + kOptions + ", epi 0 or 1");
  if (M < 1 || N < 32 || N % 32) return refuse(who + kMult32);
  if (K < 16 || K % 16) return refuse(who + kMult16);
  if (!X || !W || !Y || (epi == 1 && !Y2)) return refuse(who + ": null pointer");
  set_options(arith, block);
  if (epi == 1) {
    GemmArgs g{X, W, Y, b, M, N, K, K, K, N, relu, 0, K, nullptr, tl_gemm_bf16};
    const Drop dr = make_drop(seed, site, p);
    g.epi = 1;
    g.C2 = Y2;
    g.drop_key = dr.key;
    g.drop_thr = dr.thr;
    g.drop_scale = dr.scale;
    gemm_nt_args(g, nullptr);
  } else {
    gemm_nt(X, W, b, Y, M, N, K, relu, nullptr);
  }
  return finish("t2l_blk_gemm_nt");
}

// dX[M,Kp] (+)= dY[M,N] W[N,Kp]
int t2l_blk_gemm_nn(const float* dY, const float* W, float* dX, int M, int N, int Kp, int accumulate, int arith, int block) {
  const std::string who = "t2l_blk_gemm_nn";
  if (bad_option(arith, block, 0.f)) return refuse(who + kOptions);
  if (M < 1 || Kp < 32 || Kp % 32) return refuse(who + kMult32);
  if (N < 16 || N % 16) return refuse(who + kMult16);
  if (!dY || !W || !dX) return refuse(who + ": null pointer");
  set_options(arith, block);
  gemm_nn(dY, W, dX, M, N, Kp, accumulate, nullptr);
  return finish("t2l_blk_gemm_nn");
}

// dW[N,Kp] += dY[M,N]^T X[M,Kp];  db[N] += column sums of dY (db may be null)
int t2l_blk_gemm_tn(const float* dY, const float* X, float* dW, float* db, int M, int N, int Kp, int arith, int block) {
  const std::string who = "t2l_blk_gemm_tn";
  if (bad_option(arith, block, 0.f)) return refuse(who + kOptions);
  if (M < 1 || N < 32 || N % 32 || Kp < 32 || Kp % 32) return refuse(who + kMult32);
  if (!dY || !X || !dW) return refuse(who + ": null pointer");
  set_options(arith, block);
  gemm_tn(dY, X, dW, db, M, N, Kp, nullptr);
  return finish("t2l_blk_gemm_tn");
}

// both of the above from ONE launch; mask_src (optional): dX through the ReLU mask (mask_src > 0) and the dropout site
int t2l_blk_gemm_tn_nn(const float* dY, const float* X, float* dW, float* db, const float* W, float* dX, int M, int N, int Kp, int accumulate,
                       const float* mask_src, int arith, int block, uint32_t seed, int site, float p) {
  const std::string who = "t2l_blk_gemm_tn_nn";
  if (bad_option(arith, block, p)) return refuse(who + kOptions);
  if (M < 1 || N < 32 || N % 32 || Kp < 32 || Kp % 32) return refuse(who + kMult32);  // (N % 32 == 0 covers the dX product's reduction)
  if (!dY || !X || !dW || !W || !dX) return refuse(who + ": null pointer");
  set_options(arith, block);
  const Drop dr = make_drop(seed, site, p);
  gemm_tn_nn(dY, X, dW, db, W, dX, M, N, Kp, accumulate, mask_src, &dr, nullptr);
  return finish("t2l_blk_gemm_tn_nn");
}

// n <= 3 jobs of one shape in one launch (the small feature branches): Y_q = X_q W_q^T + b_q
int t2l_blk_gemm_nt_multi(int n, const float* const* X, const float* const* W, const float* const* b, float* const* Y, int M, int N, int K,
                          int arith) {
  const std::string who = "t2l_blk_gemm_nt_multi";
  if (bad_option(arith, 0, 0.f) || n < 1 || n > 3) return refuse(who + kOptions + ", 1 to 3 jobs");
  if (M < 1 || N < 32 || N % 32) return refuse(who + kMult32);
  if (K < 16 || K % 16) return refuse(who + kMult16);
  if (!X || !W || !b || !Y) return refuse(who + ": null pointer");
  for (int q = 0; q < n; ++q)
    if (!X[q] || !W[q] || !Y[q]) return refuse(who + ": null pointer");
  set_options(arith, 0);
  gemm_nt_multi(n, X, W, b, Y, M, N, K, nullptr);
  return finish("t2l_blk_gemm_nt_multi");
}

// ... dW_q += dY_q^T X_q, db_q += column sums, dX_q = dY_q W_q
int t2l_blk_gemm_tn_nn_multi(int n, const float* const* dY, const float* const* X, float* const* dW, float* const* db, const float* const* W,
                             float* const* dX, int M, int N, int Kp, int arith) {
  const std::string who = "t2l_blk_gemm_tn_nn_multi";
  if (bad_option(arith, 0, 0.f) || n < 1 || n > 3) return refuse(who + kOptions + ", 1 to 3 jobs");
  if (M < 1 || N < 32 || N % 32 || Kp < 32 || Kp % 32) return refuse(who + kMult32);
  if (!dY || !X || !dW || !db || !W || !dX) return refuse(who + ": null pointer");
  for (int q = 0; q < n; ++q)
    if (!dY[q] || !X[q] || !dW[q] || !W[q] || !dX[q]) return refuse(who + ": null pointer");
  set_options(arith, 0);
  gemm_tn_nn_multi(n, dY, X, dW, db, W, dX, M, N, Kp, nullptr);
  return finish("t2l_blk_gemm_tn_nn_multi");
}

// self-attention of B groups of S rows, 4 heads of HD (64 or 256): qkv [B S][12 HD] -> P [B 4][S][S], O [B S][4 HD]
static int attn_shape(const std::string& who, int B, int S, int HD, float p) {
  if (!(p >= 0.f && p < 1.f)) return refuse(who + ": p must be in [0, 1)");
  if (B < 1 || S < 1) return refuse(who + ": need at least one group of one row");
  if (S > 32) return refuse(who + ": S > 32 (the kernels hold a group's S x S tiles in LDS: at most 32 rows per group)");
  if (HD != 64 && HD != 256) return refuse(who + ": head dim must be 64 or 256 (the instances the step builds)");
  return 0;
}
int t2l_blk_attn_fwd(const float* qkv, float* P, float* O, int B, int S, int HD, uint32_t seed, int site, float p) {
  const std::string who = "t2l_blk_attn_fwd";
  if (int rc = attn_shape(who, B, S, HD, p)) return rc;
  if (!qkv || !P || !O) return refuse(who + ": null pointer");
  int device = 0;
  if (hipGetDevice(&device) != hipSuccess) return refuse(who + ": no device");
  const Drop dr = make_drop(seed, site, p);
  if (HD == 64) {
    attn_fwd_launch<64>(B, S, nullptr, qkv, P, O, S, dr);
  } else {
    attn256_allow_lds(device);
    attn_fwd_launch<256>(B, S, nullptr, qkv, P, O, S, dr);
  }
  return finish("t2l_blk_attn_fwd");
}
int t2l_blk_attn_bwd(const float* qkv, const float* P, const float* dO, float* dqkv, int B, int S, int HD, uint32_t seed, int site, float p) {
  const std::string who = "t2l_blk_attn_bwd";
  if (int rc = attn_shape(who, B, S, HD, p)) return rc;
  if (!qkv || !P || !dO || !dqkv) return refuse(who + ": null pointer");
  int device = 0;
  if (hipGetDevice(&device) != hipSuccess) return refuse(who + ": no device");
  const Drop dr = make_drop(seed, site, p);
  if (HD == 64) {
    attn_bwd_launch<64>(B, S, nullptr, qkv, P, dO, dqkv, S, dr);
  } else {
    attn256_allow_lds(device);
    attn_bwd_launch<256>(B, S, nullptr, qkv, P, dO, dqkv, S, dr);
  }
  return finish("t2l_blk_attn_bwd");
}

// out = LayerNorm(x + dropout(y)) over T rows of D (128, 256 or 1024); xhat and rstd saved
int t2l_blk_ln_fwd(const float* x, const float* y, int T, int D, const float* gamma, const float* beta, float* out, float* xhat, float* rstd,
                   uint32_t seed, int site, float p) {
  const std::string who = "t2l_blk_ln_fwd";
  if (!(p >= 0.f && p < 1.f)) return refuse(who + ": p must be in [0, 1)");
  const std::string shape = who + ": need T >= 1 and D 128, 256 or 1024 (the instances the steps build)";
  if (T < 1 || (D != 128 && D != 256 && D != 1024)) return refuse(shape);
  if (!x || !y || !gamma || !beta || !out || !xhat || !rstd) return refuse(who + ": null pointer");
  if (!ln_fwd_rows(D, x, y, T, gamma, beta, make_drop(seed, site, p), out, xhat, rstd, nullptr)) return refuse(shape);
  return finish("t2l_blk_ln_fwd");
}
// its backward: d_res, d_y written, dgamma / dbeta added to. (D, waves): (256, 16) the object branch, (256, 4) and (1024, 4) the text
// head, (128, 4) the fine step
int t2l_blk_ln_bwd(const float* dout, const float* xhat, const float* rstd, int T, int D, int waves, const float* gamma, float* d_res, float* d_y,
                   float* dgamma, float* dbeta, uint32_t seed, int site, float p) {
  const std::string who = "t2l_blk_ln_bwd";
  if (!(p >= 0.f && p < 1.f)) return refuse(who + ": p must be in [0, 1)");
  const std::string shape = who + ": need T >= 1 and (D, waves) one of (128, 4), (256, 16), (256, 4), (1024, 4) (the instances the steps build)";
  const bool inst = (waves == 4 && (D == 128 || D == 256 || D == 1024)) || (waves == 16 && D == 256);
  if (T < 1 || !inst) return refuse(shape);
  if (!dout || !xhat || !rstd || !gamma || !d_res || !d_y || !dgamma || !dbeta) return refuse(who + ": null pointer");
  if (!ln_bwd_rows(D, waves, dout, xhat, rstd, T, gamma, make_drop(seed, site, p), d_res, d_y, dgamma, dbeta, nullptr)) return refuse(shape);
  return finish("t2l_blk_ln_bwd");
}

// F.normalize of M rows of D (128 or 256). Forward: dst[m] (row stride ld >= D) = src[m] / max(|src[m]|, 1e-12) from contiguous src, the
// norms to save_n. Backward: dx[m] (contiguous) from dy and y (both row stride ld) and the saved norms.
static int rownorm_shape(const std::string& who, int M, int D, int ld) {
  if (M < 1) return refuse(who + ": need M >= 1");
  if (D != 128 && D != 256) return refuse(who + ": D must be 128 or 256 (the instances the steps build)");
  if (ld < D) return refuse(who + ": ld < D (the strided side holds a whole row)");
  return 0;
}
int t2l_blk_rownorm_fwd(const float* src, int M, int D, float* dst, int ld, float* save_n) {
  const std::string who = "t2l_blk_rownorm_fwd";
  if (int rc = rownorm_shape(who, M, D, ld)) return rc;
  if (!src || !dst || !save_n) return refuse(who + ": null pointer");
  if (!rownorm_rows(true, D, src, nullptr, dst, save_n, M, ld, nullptr)) return refuse(who + ": no instance of this width");
  return finish("t2l_blk_rownorm_fwd");
}
int t2l_blk_rownorm_bwd(const float* dy, const float* y, int ld, const float* save_n, int M, int D, float* dx) {
  const std::string who = "t2l_blk_rownorm_bwd";
  if (int rc = rownorm_shape(who, M, D, ld)) return rc;
  if (!dy || !y || !save_n || !dx) return refuse(who + ": null pointer");
  if (!rownorm_rows(false, D, dy, y, dx, const_cast<float*>(save_n), M, ld, nullptr)) return refuse(who + ": no instance of this width");
  return finish("t2l_blk_rownorm_bwd");
}

// hd = dropout(h) over n elements; d = dropout'(d) where h > 0, else 0, in place
static int drop_shape(const std::string& who, int64_t n, float p) {
  if (!(p >= 0.f && p < 1.f)) return refuse(who + ": p must be in [0, 1)");
  if (n < 1) return refuse(who + ": need n >= 1");
  if (n >= (1ll << 32)) return refuse(who + ": n >= 2^32 (the dropout counters are 32 bits wide)");
  return 0;
}
int t2l_blk_drop_fwd(const float* h, int64_t n, float* hd, uint32_t seed, int site, float p) {
  const std::string who = "t2l_blk_drop_fwd";
  if (int rc = drop_shape(who, n, p)) return rc;
  if (!h || !hd) return refuse(who + ": null pointer");
  drop_fwd_launch(h, (size_t)n, make_drop(seed, site, p), hd, nullptr);
  return finish("t2l_blk_drop_fwd");
}
int t2l_blk_relu_drop_bwd(float* d, const float* h, int64_t n, uint32_t seed, int site, float p) {
  const std::string who = "t2l_blk_relu_drop_bwd";
  if (int rc = drop_shape(who, n, p)) return rc;
  if (!d || !h) return refuse(who + ": null pointer");
  relu_drop_bwd_launch(d, h, (size_t)n, make_drop(seed, site, p), nullptr);
  return finish("t2l_blk_relu_drop_bwd");
}

// max over the 28 slots of each of B cells + F.normalize: X [B 28][256] -> out, out2 [B][256], arg [B][256], save_n [B]
int t2l_blk_pool_norm_fwd(const float* X, float* out, int32_t* arg, float* save_n, float* out2, int B) {
  const std::string who = "t2l_blk_pool_norm_fwd";
  if (B < 1) return refuse(who + ": need at least one cell");
  if (!X || !out || !arg || !save_n || !out2) return refuse(who + ": null pointer");
  pool_norm_fwd_launch(X, out, arg, save_n, out2, nullptr, 0, B, nullptr);
  return finish("t2l_blk_pool_norm_fwd");
}
int t2l_blk_pool_norm_bwd(const float* gout, const float* out, const int32_t* arg, const float* save_n, float* dX, int B) {
  const std::string who = "t2l_blk_pool_norm_bwd";
  if (B < 1) return refuse(who + ": need at least one cell");
  if (!gout || !out || !arg || !save_n || !dX) return refuse(who + ": null pointer");
  pool_norm_bwd_launch(gout, out, arg, save_n, dX, B, nullptr);
  return finish("t2l_blk_pool_norm_bwd");
}

// out[b][c] = max over the S rows of group b of (X + R) (R optional), first maximal row wins; arg keeps the row
static int seq_shape(const std::string& who, int B, int S, int D) {
  if (B < 1 || S < 1 || D < 1) return refuse(who + ": need B, S, D >= 1");
  if (S > 32) return refuse(who + ": S > 32 (the text head takes at most 32 rows per group)");
  if ((uint64_t)B * S * D >= (1ull << 31)) return refuse(who + ": too many elements");
  return 0;
}
int t2l_blk_seq_max_fwd(const float* X, const float* R, int B, int S, int D, float* out, int32_t* arg) {
  const std::string who = "t2l_blk_seq_max_fwd";
  if (int rc = seq_shape(who, B, S, D)) return rc;
  if (!X || !out || !arg) return refuse(who + ": null pointer");
  seq_max_fwd_launch(X, R, B, S, D, out, arg, nullptr);
  return finish("t2l_blk_seq_max_fwd");
}
int t2l_blk_seq_max_bwd(const float* g, const int32_t* arg, int B, int S, int D, float* dX) {
  const std::string who = "t2l_blk_seq_max_bwd";
  if (int rc = seq_shape(who, B, S, D)) return rc;
  if (!g || !arg || !dX) return refuse(who + ": null pointer");
  seq_max_bwd_launch(g, arg, B, S, D, dX, nullptr);
  return finish("t2l_blk_seq_max_bwd");
}

}  // extern "C"

// =================================================================================================================================
// The PointNet++ training kernels (pointnet_train.h, gemm_rows2.h), one launch at a time: tests/test_gpu_pointnet_train_blocks.py
// against the float64 references of tests/pointnet_train_blocks.py. The wrappers call the launchers pn_forward_core /
// pn_backward_core call (gemm_rows2, gemm_tn2, pn_block_fwd, pn_block_bwd, pn_*_launch). Shapes are refused first, then every index
// table is copied to the host and held against its contract — sorted cells, row counts, group offsets, index ranges — so that a mistaken
// test gets a message, never an out-of-bounds launch. Edge-row tensors (A, C, X, y, a, d) are bf16 exactly when arith == 1.
// =================================================================================================================================
namespace t2l {
namespace {

struct PnShape { int K, N; };
// (K, N) of the gemm_rows2 launches of a step: the layers with statistics, the input-gradient products, the scattered ones
const PnShape kPnRows2Stat[] = {{32, 32}, {32, 64}, {96, 128}, {128, 128}, {160, 256}, {256, 256}, {288, 512}, {512, 1024}};
const PnShape kPnRows2Plain[] = {{64, 32}, {128, 128}, {256, 256}, {1024, 512}, {512, 288}, {128, 64}, {256, 128}};
// (K, N, fused X) of the gemm_tn2 launches
struct PnTnShape { int N, K; bool fused; };
const PnTnShape kPnTn2[] = {{64, 32, true},   {128, 128, true}, {256, 256, true},  {1024, 512, false},
                            {32, 32, false},  {128, 96, false}, {256, 160, false}, {512, 288, false}};
const char* kPnWidths = ": not a layer shape of the backbone (pn_bind_core: 6/67/131/259 -> 32/128/256/512 -> 64/128/256/1024)";
const char* kPnArith = ": arith must be 0, 1 or 2";
const size_t kPnMaxRows = (size_t)1 << 30;  // (pn_forward_core's own limit per level)

bool pn_channels_ok(int C) { return C >= 32 && C <= 1024 && (C & (C - 1)) == 0; }

int pn_hip_fail(const std::string& who, hipError_t e) {
  tl_blk_error = who + ": " + hipGetErrorString(e);
  return -2;
}
// a device table on the host (synchronous copy: nothing of the wrapper is in flight yet)
int pn_fetch(const std::string& who, const int32_t* dev, size_t n, std::vector<int32_t>& h) {
  h.resize(n);
  if (n == 0) return 0;
  const hipError_t e = hipMemcpy(h.data(), dev, n * sizeof(int32_t), hipMemcpyDeviceToHost);
  return e == hipSuccess ? 0 : pn_hip_fail(who, e);
}
// row_cell [E]: sorted, inside [0, n_cells); rows[cell] = its rows
std::string pn_check_row_cell(const std::vector<int32_t>& rc, int n_cells, std::vector<int64_t>& rows) {
  rows.assign(n_cells, 0);
  for (size_t i = 0; i < rc.size(); ++i) {
    if (rc[i] < 0 || rc[i] >= n_cells) return ": row_cell[" + std::to_string(i) + "] = " + std::to_string(rc[i]) + " leaves [0, n_cells)";
    if (i && rc[i] < rc[i - 1]) return ": row_cell is not sorted at row " + std::to_string(i);
    ++rows[rc[i]];
  }
  return "";
}
// cnt [n_cells] == the rows of every cell, and every cell has at least two (the product never builds a smaller one: an object has
// 32 or more edge rows)
std::string pn_check_cnt(const std::vector<int32_t>& cnt, const std::vector<int64_t>& rows) {
  for (size_t c = 0; c < rows.size(); ++c) {
    if ((int64_t)cnt[c] != rows[c])
      return ": cnt[" + std::to_string(c) + "] = " + std::to_string(cnt[c]) + " but the cell has " + std::to_string(rows[c]) + " rows";
    if (rows[c] < 2) return ": cell " + std::to_string(c) + " has fewer than 2 rows";
  }
  return "";
}
// goff [G + 1]: from 0, increasing (no group without a row), ending at E
std::string pn_check_goff(const std::vector<int32_t>& goff, size_t E) {
  if (goff.empty() || goff[0] != 0) return ": goff does not start at 0";
  for (size_t g = 1; g < goff.size(); ++g)
    if (goff[g] <= goff[g - 1]) return ": goff is not increasing at group " + std::to_string(g - 1) + " (a group with no row)";
  if ((size_t)goff.back() != E) return ": goff ends at " + std::to_string(goff.back()) + ", not at E = " + std::to_string(E);
  return "";
}
// cell_of_obj [n_obj]: sorted, inside [0, n_cells)
std::string pn_check_cell_of_obj(const std::vector<int32_t>& co, int n_cells) {
  for (size_t o = 0; o < co.size(); ++o) {
    if (co[o] < 0 || co[o] >= n_cells) return ": cell_of_obj[" + std::to_string(o) + "] leaves [0, n_cells)";
    if (o && co[o] < co[o - 1]) return ": cell_of_obj is not sorted at object " + std::to_string(o);
  }
  return "";
}
std::string pn_check_range(const char* name, const std::vector<int32_t>& v, int64_t lo, int64_t hi) {
  for (size_t i = 0; i < v.size(); ++i)
    if (v[i] < lo || v[i] >= hi)
      return std::string(": ") + name + "[" + std::to_string(i) + "] = " + std::to_string(v[i]) + " leaves [" + std::to_string(lo) + ", " +
             std::to_string(hi) + ")";
  return "";
}
// the rows of every cell from the group offsets: a group lies inside one object, hence one cell
void pn_rows_of_groups(const std::vector<int32_t>& goff, const std::vector<int32_t>& co, int nd, int n_cells, std::vector<int64_t>& rows) {
  rows.assign(n_cells, 0);
  for (size_t g = 0; g + 1 < goff.size(); ++g) rows[co[g / nd]] += goff[g + 1] - goff[g];
}
// one get_mlp layer's tensors under the names pn_block_fwd / pn_block_bwd look up: always as layer 1 of the level "blk", so that the
// fused operand's beta ("blk.0.1.bias": the layer below) has a name of its own
void pn_block_names(PnTrain& pt, PnLevel& L, const float* bias, const float* gamma, const float* beta, float* run_mean, float* run_var,
                    float* dgamma, float* dbeta, const float* below_beta, int C, int K) {
  L.prefix = "blk";
  auto put = [&](const char* n, const float* data, float* grad, int64_t numel) {
    pt.t[std::string("blk.") + n] = TTensor{const_cast<float*>(data), grad, numel};
  };
  put("1.0.bias", bias, nullptr, C);
  put("1.1.weight", gamma, dgamma, C);
  put("1.1.bias", beta, dbeta, C);
  put("1.1.running_mean", run_mean, nullptr, C);
  put("1.1.running_var", run_var, nullptr, C);
  put("0.1.bias", below_beta, nullptr, K);
}

}  // namespace
}  // namespace t2l

extern "C" {

// C[M,N] = f(A)[M,K] W[N,K]^T (+ bias) through gemm_rows2. a_mean / a_rg / a_beta (all or none): f = the fused BatchNorm + ReLU of the
// layer below, tables [n_cells][K]; acc ([n_cells][2][1024] doubles, ADDED to): the BatchNorm sums of C per (cell, column) — both need
// row_cell [M]. scat_dst ([scat_rows][scat_cols], ADDED to): the scattered output through scat_src [M] in C's place.
int t2l_blk_pn_rows2(const void* A, const float* W, const float* bias, void* C, int64_t M, int N, int K, int arith, const float* a_mean,
                     const float* a_rg, const float* a_beta, const int32_t* row_cell, int n_cells, double* acc, const int32_t* scat_src,
                     float* scat_dst, int scat_cols, int64_t scat_rows) {
  const std::string who = "t2l_blk_pn_rows2";
  if (arith < 0 || arith > 2) return refuse(who + kPnArith);
  if (M < 1 || (size_t)M > kPnMaxRows) return refuse(who + ": need 1 <= M <= 2^30");
  if (K < 32 || K % 16) return refuse(who + kMult16);
  if (N < 32 || N % 32) return refuse(who + kMult32);
  const bool fused = a_mean || a_rg || a_beta, stats = acc != nullptr, scat = scat_src || scat_dst;
  if (stats && N > 1024) return refuse(who + ": C > 1024 columns with statistics (acc is [cell][2][1024])");
  bool shape = false;
  if (stats) {
    for (const PnShape& q : kPnRows2Stat) shape |= q.K == K && q.N == N;
  } else {
    for (const PnShape& q : kPnRows2Plain) shape |= q.K == K && q.N == N;
  }
  if (!shape) return refuse(who + kPnWidths);
  if (fused && !stats) return refuse(who + ": a fused operand without statistics (no such instance of rows2_kernel exists)");
  if (!A || !W) return refuse(who + ": null pointer");
  if (fused && (!a_mean || !a_rg || !a_beta)) return refuse(who + ": null pointer (the fused operand needs a_mean, a_rg and a_beta)");
  if ((fused || stats) && !row_cell) return refuse(who + ": null pointer (row_cell)");
  if (scat && (!scat_src || !scat_dst)) return refuse(who + ": null pointer (scat_src and scat_dst come together)");
  if (scat && stats) return refuse(who + ": a scattered output with statistics (the step builds none)");
  if (!scat && !C) return refuse(who + ": null pointer");
  if (scat && (scat_cols < 1 || scat_cols > N || scat_rows < 1)) return refuse(who + ": need 1 <= scat_cols <= N and scat_rows >= 1");
  if ((fused || stats) && n_cells < 1) return refuse(who + ": need n_cells >= 1");
  std::vector<int32_t> h;
  if (row_cell) {
    if (int rc = pn_fetch(who, row_cell, (size_t)M, h)) return rc;
    std::vector<int64_t> rows;
    const std::string bad = pn_check_row_cell(h, n_cells, rows);
    if (!bad.empty()) return refuse(who + bad);
  }
  if (scat) {
    if (int rc = pn_fetch(who, scat_src, (size_t)M, h)) return rc;
    const std::string bad = pn_check_range("scat_src", h, 0, scat_rows);
    if (!bad.empty()) return refuse(who + bad);
  }
  tl_gemm_bf16 = arith;
  gemm_rows2(reinterpret_cast<const float*>(A), W, bias, reinterpret_cast<float*>(C), (size_t)M, N, K, a_mean, a_rg, a_beta, row_cell, acc,
             nullptr, scat_src, scat_dst, scat_cols);
  return finish("t2l_blk_pn_rows2");
}

// dW[N][ldw] += dY[M,N]^T f(X)[M,K] (columns k < k_real), db[N] += column sums of dY (db may be null) through gemm_tn2; x_mean / x_rg /
// x_beta (all or none, with row_cell [M]): the fused BatchNorm + ReLU of the layer that produced X
int t2l_blk_pn_tn2(const void* dY, const void* X, float* dW, float* db, int64_t M, int N, int K, int k_real, int ldw, const float* x_mean,
                   const float* x_rg, const float* x_beta, const int32_t* row_cell, int n_cells, int arith) {
  const std::string who = "t2l_blk_pn_tn2";
  if (arith < 0 || arith > 2) return refuse(who + kPnArith);
  if (M < 1 || (size_t)M > kPnMaxRows) return refuse(who + ": need 1 <= M <= 2^30");
  if (K < 32 || K % 16) return refuse(who + kMult16);
  if (N < 32 || N % 32) return refuse(who + kMult32);
  const bool fused = x_mean || x_rg || x_beta;
  bool shape = false;
  for (const PnTnShape& q : kPnTn2) shape |= q.N == N && q.K == K && q.fused == fused;
  if (!shape) return refuse(who + kPnWidths);
  if (k_real <= K - 32 || k_real > K) return refuse(who + ": need K - 32 < k_real <= K (X is padded to the next multiple of 32)");
  if (ldw < k_real) return refuse(who + ": ldw < k_real (a row of dW holds the real columns)");
  if (!dY || !X || !dW) return refuse(who + ": null pointer");
  if (fused && (!x_mean || !x_rg || !x_beta || !row_cell)) return refuse(who + ": null pointer (the fused operand needs x_mean, x_rg, x_beta and row_cell)");
  if (fused) {
    if (n_cells < 1) return refuse(who + ": need n_cells >= 1");
    std::vector<int32_t> h;
    std::vector<int64_t> rows;
    if (int rc = pn_fetch(who, row_cell, (size_t)M, h)) return rc;
    const std::string bad = pn_check_row_cell(h, n_cells, rows);
    if (!bad.empty()) return refuse(who + bad);
  }
  tl_gemm_bf16 = arith;
  const bool launched = gemm_tn2(reinterpret_cast<const float*>(dY), reinterpret_cast<const float*>(X), dW, db, (size_t)M, N, K, k_real, ldw,
                                 x_mean, x_rg, x_beta, row_cell, nullptr);
  if (!launched) {
    (void)finish("t2l_blk_pn_tn2");
    return refuse(who + ": no tn2_kernel instance for this shape");
  }
  return finish("t2l_blk_pn_tn2");
}

// one get_mlp layer in training mode through pn_block_fwd: y = f(X) W^T + bias [E, C] with the BatchNorm sums from the product's
// epilogue, then mean / rstd (/ rg) [n_cells][C], the running statistics updated once per cell in cell order, and a = relu(bn(y)) if
// a != nullptr. f_mean / f_rg / f_beta (all or none): X is the pre-BatchNorm output of the layer below, normalised as it is loaded.
// acc: [n_cells][2][1024] doubles of scratch.
int t2l_blk_pn_block_fwd(const void* X, const float* W, int64_t E, int K, int C, int arith, const float* bias, const float* gamma,
                         const float* beta, float* run_mean, float* run_var, const int32_t* row_cell, const int32_t* cnt, int n_cells,
                         double* acc, void* y, void* a, float* mean, float* rstd, float* rg, const float* f_mean, const float* f_rg,
                         const float* f_beta) {
  const std::string who = "t2l_blk_pn_block_fwd";
  if (arith < 0 || arith > 2) return refuse(who + kPnArith);
  if (E < 1 || (size_t)E > kPnMaxRows || n_cells < 1) return refuse(who + ": need 1 <= E <= 2^30 and n_cells >= 1");
  if (K < 32 || K % 16) return refuse(who + kMult16);
  if (C < 32 || C % 32) return refuse(who + kMult32);
  if (C > 1024) return refuse(who + ": C > 1024 (acc is [cell][2][1024])");
  bool shape = false;
  for (const PnShape& q : kPnRows2Stat) shape |= q.K == K && q.N == C;
  if (!shape) return refuse(who + kPnWidths);
  const bool fused = f_mean || f_rg || f_beta;
  if (!X || !W || !bias || !gamma || !beta || !run_mean || !run_var || !row_cell || !cnt || !acc || !y || !mean || !rstd)
    return refuse(who + ": null pointer");
  if (fused && (!f_mean || !f_rg || !f_beta)) return refuse(who + ": null pointer (the fused operand needs f_mean, f_rg and f_beta)");
  std::vector<int32_t> h_rc, h_cnt;
  std::vector<int64_t> rows;
  if (int rc = pn_fetch(who, row_cell, (size_t)E, h_rc)) return rc;
  if (int rc = pn_fetch(who, cnt, (size_t)n_cells, h_cnt)) return rc;
  std::string bad = pn_check_row_cell(h_rc, n_cells, rows);
  if (bad.empty()) bad = pn_check_cnt(h_cnt, rows);
  if (!bad.empty()) return refuse(who + bad);
  PnTrain pt;
  PnLevel L;
  pn_block_names(pt, L, bias, gamma, beta, run_mean, run_var, nullptr, nullptr, f_beta, C, K);
  pt.n_cells = n_cells;
  pt.half = arith == 1;
  pt.acc = acc;
  L.E = (size_t)E;
  L.row_cell = const_cast<int32_t*>(row_cell);
  L.cnt = const_cast<int32_t*>(cnt);
  L.mean1 = const_cast<float*>(f_mean);
  L.rg1 = const_cast<float*>(f_rg);
  tl_gemm_bf16 = arith;
  pn_block_fwd(&pt, L, 1, reinterpret_cast<const float*>(X), W, K, C, reinterpret_cast<float*>(y), reinterpret_cast<float*>(a), mean, rstd, rg,
               fused, nullptr);
  return finish("t2l_blk_pn_block_fwd");
}

// the BatchNorm + ReLU backward of one layer through pn_block_bwd: d [E, C] becomes the gradient w.r.t. the Linear output in place,
// dgamma / dbeta [C] are ADDED to; k1 / k2 [n_cells][C] are the coefficient tables it builds on the way (acc: scratch as above).
//   rows form   (dxout == nullptr): d holds the gradient w.r.t. the ReLU output; the ReLU sign from the stored a, or (a == nullptr)
//               recomputed from y with rg; tables row_cell [E]
//   groups form (dxout != nullptr): the gradient is dxout [G, C] at the arg-max rows arg [G, C] (d is only written); ysel / xout [G, C],
//               goff [G + 1], cell_of_obj [G / nd]
int t2l_blk_pn_block_bwd(void* d, const void* y, const void* a, int64_t E, int C, int arith, const float* mean, const float* rstd,
                         const float* rg, const float* gamma, const float* beta, float* dgamma, float* dbeta, const int32_t* row_cell,
                         const int32_t* cnt, int n_cells, double* acc, float* k1, float* k2, const float* dxout, const int32_t* arg,
                         const float* ysel, const float* xout, const int32_t* goff, const int32_t* cell_of_obj, int64_t G, int nd) {
  const std::string who = "t2l_blk_pn_block_bwd";
  if (arith < 0 || arith > 2) return refuse(who + kPnArith);
  if (E < 1 || (size_t)E > kPnMaxRows || n_cells < 1) return refuse(who + ": need 1 <= E <= 2^30 and n_cells >= 1");
  if (!pn_channels_ok(C)) return refuse(who + ": C must be a power of two in [32, 1024] (acc is [cell][2][1024])");
  const bool groups = dxout != nullptr;
  if (!d || !y || !mean || !rstd || !gamma || !beta || !dgamma || !dbeta || !cnt || !acc || !k1 || !k2) return refuse(who + ": null pointer");
  std::vector<int32_t> h_cnt, h;
  std::vector<int64_t> rows;
  if (int rc = pn_fetch(who, cnt, (size_t)n_cells, h_cnt)) return rc;
  if (groups) {
    if (!arg || !ysel || !xout || !goff || !cell_of_obj) return refuse(who + ": null pointer (the groups form needs arg, ysel, xout, goff, cell_of_obj)");
    if (G < 1 || G > E || nd < 1 || G % nd) return refuse(who + ": need 1 <= G <= E and G a multiple of nd >= 1");
    std::vector<int32_t> h_goff, h_co;
    if (int rc = pn_fetch(who, goff, (size_t)G + 1, h_goff)) return rc;
    if (int rc = pn_fetch(who, cell_of_obj, (size_t)(G / nd), h_co)) return rc;
    if (int rc = pn_fetch(who, arg, (size_t)G * C, h)) return rc;
    std::string bad = pn_check_goff(h_goff, (size_t)E);
    if (bad.empty()) bad = pn_check_cell_of_obj(h_co, n_cells);
    if (bad.empty()) {
      pn_rows_of_groups(h_goff, h_co, nd, n_cells, rows);
      bad = pn_check_cnt(h_cnt, rows);
    }
    for (size_t i = 0; bad.empty() && i < h.size(); ++i)
      if (h[i] < h_goff[i / C] || h[i] >= h_goff[i / C + 1])
        bad = ": arg[" + std::to_string(i) + "] = " + std::to_string(h[i]) + " leaves the rows of its group";
    if (!bad.empty()) return refuse(who + bad);
  } else {
    if (!row_cell || (!a && !rg)) return refuse(who + ": null pointer (the rows form needs row_cell and a, or rg in its place)");
    if (int rc = pn_fetch(who, row_cell, (size_t)E, h)) return rc;
    std::string bad = pn_check_row_cell(h, n_cells, rows);
    if (bad.empty()) bad = pn_check_cnt(h_cnt, rows);
    if (!bad.empty()) return refuse(who + bad);
  }
  PnTrain pt;
  PnLevel L;
  pn_block_names(pt, L, nullptr, gamma, beta, nullptr, nullptr, dgamma, dbeta, nullptr, C, C);
  pt.n_cells = n_cells;
  pt.half = arith == 1;
  pt.acc = acc;
  pt.bk1 = k1;
  pt.bk2 = k2;
  pt.cell_of_obj = const_cast<int32_t*>(cell_of_obj);
  L.E = (size_t)E;
  L.G = (size_t)G;
  L.nd = nd;
  L.row_cell = const_cast<int32_t*>(row_cell);
  L.cnt = const_cast<int32_t*>(cnt);
  L.goff = const_cast<int32_t*>(goff);
  L.arg = const_cast<int32_t*>(arg);
  L.ysel = const_cast<float*>(ysel);
  L.xout = const_cast<float*>(xout);
  tl_gemm_bf16 = arith;
  pn_block_bwd(&pt, L, 1, reinterpret_cast<float*>(d), reinterpret_cast<const float*>(y), reinterpret_cast<const float*>(a), C, mean, rstd, rg,
               dxout, nullptr);
  return finish("t2l_blk_pn_block_bwd");
}

// xout [G, C] = max over the rows of every group of relu(bn(y)), arg = the first maximal row, ysel = y there (pt_segmax_kernel)
int t2l_blk_pn_segmax(const void* y, const int32_t* goff, int64_t G, int64_t E, int C, int nd, const int32_t* cell_of_obj, int n_cells,
                      const float* mean, const float* rstd, const float* gamma, const float* beta, float* xout, int32_t* arg, float* ysel,
                      int arith) {
  const std::string who = "t2l_blk_pn_segmax";
  if (arith < 0 || arith > 2) return refuse(who + kPnArith);
  if (!pn_channels_ok(C)) return refuse(who + ": C must be a power of two in [32, 1024]");
  if (E < 1 || (size_t)E > kPnMaxRows || n_cells < 1) return refuse(who + ": need 1 <= E <= 2^30 and n_cells >= 1");
  if (G < 1 || G > E || nd < 1 || G % nd) return refuse(who + ": need 1 <= G <= E and G a multiple of nd >= 1");
  if (!y || !goff || !cell_of_obj || !mean || !rstd || !gamma || !beta || !xout || !arg || !ysel) return refuse(who + ": null pointer");
  std::vector<int32_t> h_goff, h_co;
  if (int rc = pn_fetch(who, goff, (size_t)G + 1, h_goff)) return rc;
  if (int rc = pn_fetch(who, cell_of_obj, (size_t)(G / nd), h_co)) return rc;
  std::string bad = pn_check_goff(h_goff, (size_t)E);
  if (bad.empty()) bad = pn_check_cell_of_obj(h_co, n_cells);
  if (!bad.empty()) return refuse(who + bad);
  pn_segmax_launch(arith == 1, reinterpret_cast<const float*>(y), goff, (size_t)G, C, nd, cell_of_obj, mean, rstd, gamma, beta, xout, arg, ysel,
                   nullptr);
  return finish("t2l_blk_pn_segmax");
}

// the row tables of a level, then its edge inputs. sa != 0: pt_compact_kernel from nbr33 [G][33] and goff [G + 1] (an input);
// sa == 0: pt_iota_rows_kernel, `per` rows per group, goff an OUTPUT. Then pt_gather_kernel: X [E][kp] = [x_src | pos_src - centre | 0]
// from x_src [n_src][cin], pos_src [n_src][3] and pos_ctr [G][3] (null: no centre is subtracted). cell_of_obj [G / nd].
int t2l_blk_pn_rows(int sa, const int32_t* nbr33, int32_t* goff, int64_t G, int nd, int per, const int32_t* cell_of_obj, int n_cells, int64_t E,
                    int32_t* src, int32_t* row_group, int32_t* row_cell, const float* x_src, const float* pos_src, const float* pos_ctr,
                    int64_t n_src, int cin, int kp, void* X, int arith) {
  const std::string who = "t2l_blk_pn_rows";
  if (arith < 0 || arith > 2) return refuse(who + kPnArith);
  if (cin != 3 && cin != 64 && cin != 128 && cin != 256) return refuse(who + kPnWidths);
  if (kp != (cin + 3 + 31) / 32 * 32) return refuse(who + ": kp must be cin + 3 rounded up to a multiple of 32");
  if (E < 1 || (size_t)E > kPnMaxRows || n_cells < 1 || n_src < 1 || (size_t)n_src > kPnMaxRows)
    return refuse(who + ": need 1 <= E, n_src <= 2^30 and n_cells >= 1");
  if (G < 1 || G > E || nd < 1 || G % nd) return refuse(who + ": need 1 <= G <= E and G a multiple of nd >= 1");
  if (!goff || !cell_of_obj || !src || !row_group || !row_cell || !x_src || !pos_src || !X || (sa && !nbr33)) return refuse(who + ": null pointer");
  std::vector<int32_t> h_co;
  if (int rc = pn_fetch(who, cell_of_obj, (size_t)(G / nd), h_co)) return rc;
  std::string bad = pn_check_cell_of_obj(h_co, n_cells);
  if (!bad.empty()) return refuse(who + bad);
  if (sa) {
    std::vector<int32_t> h_goff, h_nbr;
    if (int rc = pn_fetch(who, goff, (size_t)G + 1, h_goff)) return rc;
    if (int rc = pn_fetch(who, nbr33, (size_t)G * 33, h_nbr)) return rc;
    bad = pn_check_goff(h_goff, (size_t)E);
    for (size_t g = 0; bad.empty() && g < (size_t)G; ++g) {
      const int rows = h_goff[g + 1] - h_goff[g], loop = h_nbr[g * 33 + 32] >= 0 ? 1 : 0;
      if (rows > 33) bad = ": group " + std::to_string(g) + " has more than 33 rows";
      for (int slot = 0; bad.empty() && slot < 33; ++slot) {
        const int v = h_nbr[g * 33 + slot];
        if (v >= n_src) bad = ": nbr33 of group " + std::to_string(g) + " leaves [0, n_src)";
        else if (slot < 32 && (v >= 0) != (slot < rows - loop))
          bad = ": nbr33 of group " + std::to_string(g) + " does not hold goff's row count in its first slots";
      }
    }
    if (!bad.empty()) return refuse(who + bad);
    pn_compact_launch(nbr33, goff, (size_t)G, nd, cell_of_obj, src, row_group, row_cell, nullptr);
  } else {
    if (nd != 1 || per < 1 || (int64_t)per * G != E) return refuse(who + ": the iota form needs nd == 1 and E == per * G");
    if (n_src < E) return refuse(who + ": the iota form reads source row i for edge row i: n_src < E");
    pn_iota_launch((size_t)E, per, cell_of_obj, src, row_group, row_cell, goff, nullptr);
  }
  pn_gather_launch(arith == 1, x_src, pos_src, pos_ctr, src, row_group, (size_t)E, cin, kp, reinterpret_cast<float*>(X), nullptr);
  return finish("t2l_blk_pn_rows");
}

// FPS, then the ball query, of one level: pos [n_obj][ns][3] -> pos_out [n_obj][nd][3], nbr33 [n_obj nd][33], cnt_g [n_obj nd].
// r2 = radius * radius as a float32 product (pn_forward_core's)
int t2l_blk_pn_index(const float* pos, int n_obj, int ns, int nd, float radius, const int32_t* cell_base, int self_loops, float* pos_out,
                     int32_t* nbr33, int32_t* cnt_g) {
  const std::string who = "t2l_blk_pn_index";
  if (ns != 256 && ns != 128 && ns != 64) return refuse(who + ": ns must be 256, 128 or 64 (the levels of the backbone)");
  if (n_obj < 1 || nd < 1 || nd > ns || (size_t)n_obj * ns > kPnMaxRows) return refuse(who + ": need n_obj >= 1 and 1 <= nd <= ns");
  if (!(radius > 0.f)) return refuse(who + ": need radius > 0");
  if (!pos || !cell_base || !pos_out || !nbr33 || !cnt_g) return refuse(who + ": null pointer");
  std::vector<int32_t> h;
  if (int rc = pn_fetch(who, cell_base, (size_t)n_obj, h)) return rc;
  for (int o = 0; o < n_obj; ++o)
    if (h[o] < 0 || h[o] > o || (o && h[o] < h[o - 1]))
      return refuse(who + ": cell_base[" + std::to_string(o) + "] is not the first object of a cell at or before it");
  const float r2 = radius * radius;
  if (!pn_fps_launch(ns, pos, n_obj, nd, pos_out, nullptr)) return refuse(who + ": no instance for this ns");
  (void)pn_ball_launch(ns, pos, pos_out, n_obj, nd, r2, cell_base, self_loops ? 1 : 0, nbr33, cnt_g, nullptr);
  return finish("t2l_blk_pn_index");
}

// the exact copies: op 0 pad  W [rows][a] -> out [rows][b] (zeros from column a on);  1 transpose  W [rows][a] -> out [a][rows];
// 2 slice  in [rows][b] (an edge-row tensor) -> out [rows][a] float32;  3 relu-mask  out[i] = 0 where !(in[i] > 0), rows elements
int t2l_blk_pn_layout(int op, const void* in, void* out, int64_t rows, int a, int b, int arith) {
  const std::string who = "t2l_blk_pn_layout";
  if (arith < 0 || arith > 2) return refuse(who + kPnArith);
  if (op < 0 || op > 3) return refuse(who + ": op must be 0 (pad), 1 (transpose), 2 (slice) or 3 (relu-mask)");
  if (rows < 1 || (size_t)rows > kPnMaxRows) return refuse(who + ": need 1 <= rows <= 2^30");
  if (!in || !out) return refuse(who + ": null pointer");
  const float* fin = reinterpret_cast<const float*>(in);
  float* fout = reinterpret_cast<float*>(out);
  if (op == 0) {
    if (a < 1 || b < a || b % 32 || rows * b >= (1ll << 31)) return refuse(who + ": pad needs 1 <= kin <= kp, kp a multiple of 32, rows * kp < 2^31");
    pn_pad_launch(fin, (int)rows, a, b, fout, nullptr);
  } else if (op == 1) {
    if (a < 1 || rows * a >= (1ll << 31)) return refuse(who + ": transpose needs Kp >= 1 and N * Kp < 2^31");
    pn_transpose_launch(fin, (int)rows, a, fout, nullptr);
  } else if (op == 2) {
    if (a < 1 || b < a || b % 32) return refuse(who + ": slice needs 1 <= cin <= kp, kp a multiple of 32");
    pn_slice_launch(arith == 1, fin, (size_t)rows, a, b, fout, nullptr);
  } else {
    pn_relu_mask_launch(fout, fin, (size_t)rows, nullptr);
  }
  return finish("t2l_blk_pn_layout");
}

}  // extern "C"
