// Dev-only block library (libt2l_blocks.so; never shipped, not part of include/t2l.h): the text head's kernels one launch at a time, so
// that tests/test_gpu_text_head_blocks.py can hold every output element against a float64 reference (tests/text_head_blocks.py).
// This translation unit IS text_head.hip plus the wrappers below and is linked in text_head.o's place: every launch goes through the
// product's own launcher (th_launch_gemm, fast_gemm) or is the product's own hipLaunchKernelGGL line with the caller's pointers.
//
// The planes are the CALLER'S: the test packs T16 / T32 with its own numpy restatement of the layouts, so the layout is held from both
// sides. Every wrapper refuses (-1, message through t2l_blk_last_error, nothing launched) a shape outside the contract of the kernel
// it launches — among them the ring's minimum: th_gemm_kernel needs n_my * KT >= 4 k-steps per workgroup (K >= 64 for a lone tile).
//
//   t2l_blk_th_set_cus   the CU count the grid rule sees (a multiple of 8; 0 restores the device's): 8 CUs give a workgroup of a
//                        2 x 2-tile product four jobs, which reaches the ring's cross-tile prefetch at a few hundred rows
//   t2l_blk_th_saved     after t2l_text_head on a context made through THIS library: one workspace buffer of the last pass
//
// Not wrapped: th_attn_kernel<256> and th_ln_kernel<., 256> (nothing launches them) and accumulate == 2 (no caller sets it).
// Return: 0, -1 (refused), -2 (the HIP runtime reported an error). The launch is synchronised before a wrapper returns.
#include "text_head.hip"
#include "blocks_common.h"

namespace t2l {
namespace {

const char* kRing = ": th_gemm_kernel needs K a multiple of 32 and at least four k-steps per job (K / ksplit >= 64)";

int th_blk_device(const std::string& who) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return blk_refuse(who + ": no device");
  if (th_kernel_attributes(dev) != hipSuccess) return blk_refuse(who + ": hipFuncSetAttribute failed");
  return 0;
}

}  // namespace

// for encode_blocks.hip: the inter layer as text_inter_impl hands it to text_inter_fused_launch
bool blk_text_inter_weights(t2l_ctx* ctx, InterFusedW* W, int* D, int* heads) {
  const th::Weights* T = ctx ? (const th::Weights*)ctx->text_head : nullptr;
  if (!T || !T->has_inter) return false;
  *W = T->fused;
  *D = T->inter_dim;
  *heads = T->inter_heads;
  return true;
}

}  // namespace t2l

using namespace t2l;
using namespace t2l::th;

extern "C" {

int t2l_blk_th_set_cus(int n) {
  if (n != 0 && (n < 8 || n % 8 || n > 1024)) return blk_refuse("t2l_blk_th_set_cus: 0 (the device's count) or a multiple of 8 up to 1024");
  th_cu_override = n;
  return 0;
}

int t2l_blk_th_cus() { return th_cu_count(); }

// the grid the product's rule gives a product of m_tiles x n_tiles tiles cut into ks k-parts, under the CU count in effect
int t2l_blk_th_grid(int m_tiles, int n_tiles, int ks) { return (m_tiles < 1 || n_tiles < 1 || ks < 1) ? 0 : th_gemm_grid(m_tiles, n_tiles, ks); }

// row-major f32 x [M][C] -> T16 f16 planes hi, lo of m_pad rows (rows >= M zeros); flag |= 1 for |v| >= 3e4, inf, NaN
int t2l_blk_th_split(const float* x, int M, int C, int m_pad, void* hi, void* lo, int* flag) {
  const std::string who = "t2l_blk_th_split";
  if (!x || !hi || !lo || !flag) return blk_refuse(who + ": null pointer");
  if (M < 1 || C < 256 || C % 256 || m_pad < M || m_pad % 256) return blk_refuse(who + ": need M >= 1, C a multiple of 256, m_pad >= M a multiple of 256");
  hipLaunchKernelGGL(th_split_kernel, dim3(m_pad / 32, C / 256), dim3(256), 0, nullptr, x, M, C, (_Float16*)hi, (_Float16*)lo, flag);
  return blk_finish("t2l_blk_th_split");
}

// row-major f32 a [R][C] -> T16 bf16 planes of a (trans = 0: rows R, contraction C) or of a^T (trans = 1: rows C, contraction R) with
// fast_gemm's padding: rows to a multiple of 256, the contraction to a multiple of 64 (*rows_pad, *k_pad); cap = elements per plane.
// colsum (trans only, nullable): colsum[c] += sum_r a[r][c]
int t2l_blk_th_split_bf16(int trans, const float* a, int R, int C, void* hi, void* lo, int64_t cap, float* colsum, int* rows_pad, int* k_pad) {
  const std::string who = "t2l_blk_th_split_bf16";
  if (!a || !hi || !lo || !rows_pad || !k_pad) return blk_refuse(who + ": null pointer");
  if (R < 1 || C < 4 || C % 4) return blk_refuse(who + ": need R >= 1 and C a multiple of 4 (float4 reads of a row)");
  if (!trans && colsum) return blk_refuse(who + ": the column sum is part of the transposed pass only");
  const int rows = trans ? C : R, kc = trans ? R : C;
  const int kp = (kc + 63) / 64 * 64, rp = (rows + kTile - 1) / kTile * kTile;
  *rows_pad = rp, *k_pad = kp;
  if (cap < (int64_t)rp * kp) return blk_refuse(who + ": the planes are too small");
  if (trans) hipLaunchKernelGGL(th_split_bf16_kernel<true>, dim3(rp / 128, kp / 64), dim3(256), 0, nullptr, a, R, C, kp, (__bf16*)hi, (__bf16*)lo, colsum);
  else hipLaunchKernelGGL(th_split_bf16_kernel<false>, dim3(rp / 32, (kp + 255) / 256), dim3(256), 0, nullptr, a, R, C, kp, (__bf16*)hi, (__bf16*)lo, (float*)nullptr);
  return blk_finish("t2l_blk_th_split_bf16");
}

// th_launch_gemm<epi> on f16 planes: OUT[m][n] = sum_k X[m][k] W[n][k] + bias[n] (+ residual) -> epi 0: T32 out0; 1: T32 out0 with the
// residual planes rh / rl [m_pad][N] added; 2: ReLU -> T16 planes out0 (hi), out1 (lo; split only), flag; 3: row-major out0 [M][n_real]
// (relu, accumulate 0 / 1). W planes [256 n_tiles][K], X planes [256 m_tiles][K], bias [N = 256 n_tiles].
int t2l_blk_th_gemm(int epi, int single, const void* wh, const void* wl, const void* xh, const void* xl, const float* bias, const void* rh,
                    const void* rl, void* out0, void* out1, int* flag, int m_tiles, int n_tiles, int K, int N, int M, int n_real, int relu,
                    int accumulate) {
  const std::string who = "t2l_blk_th_gemm";
  if (epi < 0 || epi > 3 || (single != 0 && single != 1)) return blk_refuse(who + ": epi 0..3, single 0 / 1");
  if (K < 64 || K % 32) return blk_refuse(who + kRing);
  if (m_tiles < 1 || n_tiles < 1 || N != n_tiles * kTile || M < 1 || M > m_tiles * kTile)
    return blk_refuse(who + ": need m_tiles, n_tiles >= 1, N = 256 n_tiles, 1 <= M <= 256 m_tiles");
  if (n_real < 4 || n_real % 4 || n_real > N || (epi != kEpiRowMajor && n_real != N)) return blk_refuse(who + ": n_real a multiple of 4 in 4..N (= N unless row-major)");
  if (epi != kEpiRowMajor && (relu || accumulate)) return blk_refuse(who + ": relu / accumulate belong to the row-major epilogue");
  if ((relu != 0 && relu != 1) || (accumulate != 0 && accumulate != 1))
    return blk_refuse(who + ": relu 0 / 1, accumulate 0 / 1 (2: no caller sets it; 3: fast_gemm's slabs, through t2l_blk_fast_gemm)");
  if (!wh || !xh || !bias || !out0 || (!single && (!wl || !xl))) return blk_refuse(who + ": null operand");
  if (epi == kEpiResidT32 && (!rh || !rl)) return blk_refuse(who + ": the residual epilogue reads both residual planes");
  if (epi == kEpiReluT16 && (!flag || (!single && !out1))) return blk_refuse(who + ": the ReLU epilogue needs the flag (and out1 unless single)");
  if (int rc = th_blk_device(who)) return rc;
  GemmArgs g{};
  g.wh = (const char*)wh, g.wl = (const char*)wl, g.xh = (const char*)xh, g.xl = (const char*)xl, g.bias = bias;
  g.rh = (const char*)rh, g.rl = (const char*)rl, g.out0 = out0, g.out1 = out1, g.flag = flag;
  g.m_tiles = m_tiles, g.n_tiles = n_tiles, g.K = K, g.N = N, g.M = M, g.n_real = n_real, g.relu = relu, g.accumulate = accumulate;
  const bool sg = single != 0;
  if (epi == kEpiT32) th_launch_gemm<kEpiT32>(sg, g, nullptr);
  else if (epi == kEpiResidT32) th_launch_gemm<kEpiResidT32>(sg, g, nullptr);
  else if (epi == kEpiReluT16) th_launch_gemm<kEpiReluT16>(sg, g, nullptr);
  else th_launch_gemm<kEpiRowMajor>(sg, g, nullptr);
  return blk_finish("t2l_blk_th_gemm");
}

// th_attn_kernel<1024> with the product's grid: qkv T32 [m_pad][3072], n_sent sentences of L tokens -> T16 planes ohi, olo [m_pad][1024]
int t2l_blk_th_attn(const float* qkv, int n_sent, int L, void* ohi, void* olo, int* flag) {
  const std::string who = "t2l_blk_th_attn";
  if (!qkv || !ohi || !olo || !flag) return blk_refuse(who + ": null pointer");
  if (n_sent < 1 || L < 1 || L > kMaxL) return blk_refuse(who + ": need n_sent >= 1 and 1 <= L <= 32");
  const int G = 32 / L, n_groups = (n_sent + G - 1) / G;
  hipLaunchKernelGGL(th_attn_kernel<1024>, dim3(n_groups), dim3(256), 0, nullptr, qkv, n_sent, L, n_groups, (_Float16*)ohi, (_Float16*)olo, flag);
  return blk_finish("t2l_blk_th_attn");
}

// th_ln_kernel<pool> over y T32 [m_pad][1024] with the product's LDS sizes. pool = 0: T16 planes hi, lo [m_pad][1024] and the flag;
// pool = 1: pooled[sentence][1024] = max over the sentence's L rows (M = n_sent L; the caller pre-fills pooled with -inf, as the product does)
int t2l_blk_th_ln(int pool, const float* y, const float* gamma, const float* beta, int M, int L, int m_pad, void* hi, void* lo, float* pooled,
                  int* flag) {
  const std::string who = "t2l_blk_th_ln";
  if (!y || !gamma || !beta) return blk_refuse(who + ": null pointer");
  if (M < 1 || m_pad < M || m_pad % 32) return blk_refuse(who + ": need 1 <= M <= m_pad, m_pad a multiple of 32");
  if (pool ? (!pooled || L < 1 || L > kMaxL || M % L) : (!hi || !lo || !flag))
    return blk_refuse(who + ": pool needs pooled, 1 <= L <= 32 and M a multiple of L; else hi, lo and the flag");
  if (int rc = th_blk_device(who)) return rc;
  if (pool)
    hipLaunchKernelGGL(th_ln_kernel<true>, dim3(m_pad / 32), dim3(256), 32 * 1028 * 4, nullptr, y, gamma, beta, M, L, (_Float16*)nullptr, (_Float16*)nullptr,
                       pooled, flag);
  else
    hipLaunchKernelGGL(th_ln_kernel<false>, dim3(m_pad / 32), dim3(256), 8 * 32 * 4, nullptr, y, gamma, beta, M, L, (_Float16*)hi, (_Float16*)lo,
                       (float*)nullptr, flag);
  return blk_finish("t2l_blk_th_ln");
}

// fast_gemm as train.hip calls it (null stream); *ks = the k-split it chose
int t2l_blk_fast_gemm(t2l_ctx* ctx, const float* A, int a_trans, const float* B, int b_trans, const float* bias, float* out, int Mo, int No, int Kc,
                      int relu, int accumulate, int single, float* a_colsum, int* ks) {
  const std::string who = "t2l_blk_fast_gemm";
  if (!ctx || !A || !B || !out || !ks) return blk_refuse(who + ": null pointer");
  if (Mo < 1 || No < kTile || No % kTile || No > 16384 || Kc < 1) return blk_refuse(who + ": need Mo, Kc >= 1 and No a multiple of 256 up to 16384");
  if ((a_trans && Mo % 4) || ((!a_trans || !b_trans) && Kc % 4)) return blk_refuse(who + ": a row the split pass reads must be a multiple of 4 floats long");
  if ((relu != 0 && relu != 1) || (accumulate != 0 && accumulate != 1)) return blk_refuse(who + ": relu 0 / 1, accumulate 0 / 1");
  if (a_colsum && !a_trans) return blk_refuse(who + ": the column sum rides in the transposed split of A");
  if (hipSetDevice(ctx->device) != hipSuccess) return blk_refuse(who + ": no device");
  const int k_pad = (Kc + 63) / 64 * 64, m_tiles = (Mo + kTile - 1) / kTile;
  *ks = fast_ksplit(m_tiles, No / kTile, k_pad >> 4);
  if ((k_pad >> 4) / *ks < 4) return blk_refuse(who + kRing);
  if (fast_gemm(ctx, A, a_trans != 0, B, b_trans != 0, bias, out, Mo, No, Kc, relu, accumulate, single != 0, nullptr, a_colsum) != T2L_OK)
    return blk_refuse(who + ": " + t2l_last_error(ctx));
  return blk_finish("t2l_blk_fast_gemm");
}

// One workspace buffer of the LAST pass of the last t2l_text_head call on ctx. Fields: xh xl (x planes), qkv (T32), oh ol, x1h x1l, hh hl
// (T16 planes, m_pad rows of the pass), y (T32, as LayerNorm2 read it), pooled (f32 [n_sent][1024]), ph pl (its planes, sp_cap rows).
// *bytes: the size; dst (nullable: the size alone) holds cap bytes.
int t2l_blk_th_saved(t2l_ctx* ctx, const char* field, void* dst, int64_t cap, int64_t* bytes) {
  const std::string who = "t2l_blk_th_saved";
  if (!ctx || !field || !bytes) return blk_refuse(who + ": null context / field / bytes");
  Weights* W = (Weights*)ctx->text_head;
  if (!W || !W->ws || W->last_n_sent < 1) return blk_refuse(who + ": no t2l_text_head call on this context");
  const ThLayout y = th_layout(W->last_n_sent, W->last_L, W->last_rows);
  const int ns = W->last_n_sent - (y.n_chunks - 1) * y.spc;
  const size_t m_pad = (size_t)((ns * W->last_L + kTile - 1) / kTile * kTile);
  const std::string f = field;
  const struct {
    const char* name;
    size_t off, n;
  } tab[] = {{"xh", y.o_xh, m_pad * kDM * 2},   {"xl", y.o_xl, m_pad * kDM * 2},   {"qkv", y.o_qkv, m_pad * 3 * kDM * 4},
             {"oh", y.o_oh, m_pad * kDM * 2},   {"ol", y.o_ol, m_pad * kDM * 2},   {"y", y.o_y, m_pad * kDM * 4},
             {"x1h", y.o_1h, m_pad * kDM * 2},  {"x1l", y.o_1l, m_pad * kDM * 2},  {"hh", y.o_hh, m_pad * kFF * 2},
             {"hl", y.o_hl, m_pad * kFF * 2},   {"pooled", y.o_pool, (size_t)W->last_n_sent * kDM * 4},
             {"ph", y.o_ph, (size_t)y.sp_cap * kDM * 2}, {"pl", y.o_pl, (size_t)y.sp_cap * kDM * 2}};
  for (const auto& e : tab)
    if (f == e.name) {
      *bytes = (int64_t)e.n;
      if (!dst) return 0;
      if (cap < (int64_t)e.n) return blk_refuse(who + ": dst is too small for " + f);
      if (e.off + e.n > W->ws_cap) return blk_refuse(who + ": the workspace is smaller than the layout");
      if (hipSetDevice(ctx->device) != hipSuccess) return blk_refuse(who + ": no device");
      if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(dst, W->ws + e.off, e.n, hipMemcpyDeviceToDevice) != hipSuccess) {
        blk_refuse(who + ": copy failed");
        return -2;
      }
      return blk_finish("t2l_blk_th_saved");
    }
  return blk_refuse(who + ": no field " + f);
}

}  // extern "C"
