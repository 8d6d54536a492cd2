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
