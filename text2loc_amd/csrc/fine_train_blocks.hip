// Dev-only block library (libt2l_blocks.so; never shipped, not part of include/t2l.h): the fine-stage training step's own kernels one
// launch at a time, so that tests/test_gpu_fine_train_blocks.py can hold every element against a float64 reference
// (tests/fine_train_blocks.py). This translation unit IS fine_train.hip plus the wrappers below and is linked in fine_train.o's place:
// every launch goes through the product's own static launchers (lin_fwd / lin_dx / lin_dw, so the split over the rows is the
// product's policy) or is the product's own hipLaunchKernelGGL line with the caller's pointers.
//
// t2l_blk_ft_bn_sync_fwd / _bwd run the phased BatchNorm of the cross-rank statistics with the ranks emulated as parts of the rows.
//
// Two doors into a bound context (t2l_fine_train_bind through this library) after the product's own t2l_fine_train_forward:
//   t2l_blk_ft_saved    copies one saved activation of the last forward out of the context's arena
//   t2l_blk_ft_dec_bwd  one call of the product's dec_bwd on one layer of the bound state
//
// Return: 0, -1 (refused, message through t2l_blk_last_error; nothing was launched), -2 (the HIP runtime reported an error). The
// launch is synchronised before a wrapper returns.
#include "fine_train.hip"
#include "blocks_common.h"

namespace t2l {
namespace ft {

static bool blk_bad_p(float p) { return !(p >= 0.f && p < 1.f); }

// (pointer, element count, 1 = int32) of a saved field, or false
static bool blk_bn_field(const BnLayer& l, const std::string& f, int M, const void** ptr, int64_t* n) {
  if (f == "xhat") *ptr = l.xhat, *n = (int64_t)M * l.N;
  else if (f == "out") *ptr = l.out, *n = (int64_t)M * l.N;
  else if (f == "rstd") *ptr = l.rstd, *n = l.N;
  else return false;
  return true;
}

static bool blk_field(const FineTrain* st, int layer, const std::string& f, const void** ptr, int64_t* n) {
  const int P = st->P, H = st->H, M0 = P * kObj;
  if (layer >= 0) {
    const DecLayer& L = st->dec[layer];
    const int64_t M = (int64_t)P * L.Tq, Mm = (int64_t)P * L.Tk;
    const struct {
      const char* name;
      const float* p;
      int64_t n;
    } tab[] = {{"qkv", L.qkv, M * 3 * kW}, {"Ps", L.Ps, (int64_t)P * kHeads * L.Tq * L.Tq}, {"os", L.os, M * kW}, {"xh1", L.xh1, M * kW},
               {"r1", L.r1, M}, {"x1", L.x1, M * kW}, {"q2", L.q2, M * kW}, {"kv2", L.kv2, Mm * 2 * kW},
               {"Pc", L.Pc, (int64_t)P * kHeads * L.Tq * L.Tk}, {"oc", L.oc, M * kW}, {"xh2", L.xh2, M * kW}, {"r2", L.r2, M},
               {"x2", L.x2, M * kW}, {"h1", L.h1, M * kFF}, {"h1d", L.h1d, M * kFF}, {"xh3", L.xh3, M * kW}, {"r3", L.r3, M},
               {"out", L.out, M * kW}};
    for (const auto& e : tab)
      if (f == e.name) {
        *ptr = e.p, *n = e.n;
        return true;
      }
    return false;
  }
  static const char* const names[4] = {"class", "color", "position", "num"};
  for (int b = 0; b < 4; ++b) {
    const std::string pre = std::string(names[b]) + ".";
    if (f.compare(0, pre.size(), pre) != 0) continue;
    const Branch& br = st->br[b];
    if (!br.used) return false;
    const std::string rest = f.substr(pre.size());
    if (rest == "raw") {
      if (!br.embed) return false;
      *ptr = br.raw, *n = (int64_t)M0 * kW;
      return true;
    }
    if (rest == "nrm") {
      *ptr = br.nrm, *n = M0;
      return true;
    }
    if (rest == "in") {
      if (b != 3) return false;
      *ptr = br.in, *n = M0;
      return true;
    }
    if (rest.size() > 2 && rest[1] == '.' && rest[0] >= '0' && rest[0] - '0' < (int)br.mlp.size())
      return blk_bn_field(br.mlp[rest[0] - '0'], rest.substr(2), M0, ptr, n);
    return false;
  }
  if (f.compare(0, 6, "merge.") == 0) return st->n_feat > 1 && blk_bn_field(st->merge, f.substr(6), M0, ptr, n);
  if (f.compare(0, 8, "pn_only.") == 0) return st->pn_stats && blk_bn_field(st->pn_only, f.substr(8), M0, ptr, n);
  if (f == "E") *ptr = st->E, *n = (int64_t)M0 * kW * st->n_feat;
  else if (f == "D0") *ptr = st->D0, *n = (int64_t)M0 * kW;
  else if (f == "nrm0") *ptr = st->nrm0, *n = M0;
  else if (f == "pool") *ptr = st->pool, *n = (int64_t)P * kW;
  else if (f == "arg") *ptr = st->arg, *n = (int64_t)P * kW;
  else if (f == "a1") *ptr = st->a1, *n = (int64_t)P * 64;
  else return false;
  (void)H;
  return true;
}

static FineTrain* blk_state(const std::string& who, t2l_ctx* ctx, int layer, bool enc_ok) {
  FineTrain* st = ctx ? (FineTrain*)ctx->fine_train : nullptr;
  if (!st || !st->have_fwd) {
    blk_refuse(who + ": no context, or no training-mode forward (t2l_fine_train_bind, t2l_fine_train_forward)");
    return nullptr;
  }
  if (layer >= (int)st->dec.size() || layer < (enc_ok ? -1 : 0)) {
    blk_refuse(who + ": no such decoder layer (cascade order: cross_objects.0, cross_hints.0, ...; a 0-layer model has cross_hints alone)");
    return nullptr;
  }
  return st;
}

}  // namespace ft
}  // namespace t2l

using namespace t2l;
using namespace t2l::ft;

extern "C" {

// Y[M,N] (row stride ldy) = X[M,K] (ldx) · W[N,K]ᵀ (ldw) + b (nullable) (ReLU)
int t2l_blk_ft_lin_fwd(const float* X, int64_t ldx, int M, int K, const float* W, int64_t ldw, const float* b, int N, float* Y, int64_t ldy,
                       int relu) {
  const std::string who = "t2l_blk_ft_lin_fwd";
  if (!X || !W || !Y) return blk_refuse(who + ": null pointer");
  if (M < 1 || N < 1 || K < 1 || ldx < K || ldw < K || ldy < N) return blk_refuse(who + ": need M, N, K >= 1 and ldx, ldw >= K, ldy >= N");
  lin_fwd(nullptr, X, ldx, M, K, W, ldw, b, N, Y, ldy, relu != 0);
  return blk_finish("t2l_blk_ft_lin_fwd");
}

// dX[M,K] (ldx) (+)= dY[M,N] (ldd) · W[N,K] (ldw)
int t2l_blk_ft_lin_dx(const float* dY, int64_t ldd, int M, int N, const float* W, int64_t ldw, int K, float* dX, int64_t ldx, int acc) {
  const std::string who = "t2l_blk_ft_lin_dx";
  if (!dY || !W || !dX) return blk_refuse(who + ": null pointer");
  if (M < 1 || N < 1 || K < 1 || ldd < N || ldw < K || ldx < K) return blk_refuse(who + ": need M, N, K >= 1 and ldd >= N, ldw, ldx >= K");
  lin_dx(nullptr, dY, ldd, M, N, W, ldw, K, dX, ldx, acc != 0);
  return blk_finish("t2l_blk_ft_lin_dx");
}

// dW[N,K] (ldw) += dY[M,N]ᵀ (ldd) · X[M,K] (ldx), db[N] += the column sums of dY; either of dW, db may be null
int t2l_blk_ft_lin_dw(const float* dY, int64_t ldd, const float* X, int64_t ldx, int M, int N, int K, float* dW, int64_t ldw, float* db) {
  const std::string who = "t2l_blk_ft_lin_dw";
  if (!dY || (dW && !X) || (!dW && !db)) return blk_refuse(who + ": null dY, dW without X, or neither dW nor db");
  if (M < 1 || N < 1 || K < 1 || ldd < N || (dW && (ldx < K || ldw < K))) return blk_refuse(who + ": need M, N, K >= 1 and ldd >= N, ldx, ldw >= K");
  lin_dw(nullptr, dY, ldd, X, ldx, M, N, K, dW, ldw, db);
  return blk_finish("t2l_blk_ft_lin_dw");
}

// BatchNorm1d + ReLU over Y[M,N]: x̂ in place, out, rstd written; rm / rv (nullable) updated
int t2l_blk_ft_bn_fwd(float* Y, int M, int N, const float* g, const float* b, float* rm, float* rv, float* rstd, float* out) {
  const std::string who = "t2l_blk_ft_bn_fwd";
  if (!Y || !g || !b || !rstd || !out) return blk_refuse(who + ": null pointer");
  if (M < 1 || N < 1) return blk_refuse(who + ": need M, N >= 1");
  hipLaunchKernelGGL(k_bn_fwd, dim3(N), dim3(256), 0, nullptr, Y, M, N, g, b, rm, rv, rstd, out);
  return blk_finish("t2l_blk_ft_bn_fwd");
}

// its backward: dy written, dg / db (nullable) added to
int t2l_blk_ft_bn_bwd(const float* dout, const float* out, const float* xhat, const float* rstd, const float* g, int M, int N, float* dg,
                      float* db, float* dy) {
  const std::string who = "t2l_blk_ft_bn_bwd";
  if (!dout || !out || !xhat || !rstd || !g || !dy) return blk_refuse(who + ": null pointer");
  if (M < 1 || N < 1) return blk_refuse(who + ": need M, N >= 1");
  hipLaunchKernelGGL(k_bn_bwd, dim3(N), dim3(256), 0, nullptr, dout, out, xhat, rstd, g, M, N, dg, db, dy);
  return blk_finish("t2l_blk_ft_bn_bwd");
}

// ---- the phased BatchNorm (cross-rank statistics) with the ranks emulated in one process: the M rows are `parts` consecutive parts of
// rows[p] rows (a host array). Each part's statistics launch goes into the part's own accumulator slot, the slots are added up on the
// device in the callback's place (every slot then holds the total, as after an all_reduce), each part's apply launch reads its slot.
// The slots start out as NaN: a launch must store whatever it later reads. Through the product's launchers (bn_stats_* / bn_apply_*).
__global__ void k_blk_slot_sum(double* slots, int parts) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= kBnStride) return;
  double t = 0.0;
  for (int p = 0; p < parts; ++p) t += slots[(size_t)p * kBnStride + i];
  for (int p = 0; p < parts; ++p) slots[(size_t)p * kBnStride + i] = t;
}
static int blk_sync_parts(const std::string& who, const int32_t* rows, int parts, int N, double** slots) {
  if (!rows || parts < 1 || parts > 16) return blk_refuse(who + ": need 1..16 parts");
  if (N < 1 || N > 1024) return blk_refuse(who + ": need 1 <= N <= 1024 (a slot holds 2 x 1024 column sums)");
  for (int p = 0; p < parts; ++p)
    if (rows[p] < 1) return blk_refuse(who + ": every part needs at least one row");
  const size_t bytes = sizeof(double) * (size_t)parts * kBnStride;
  if (hipMalloc(slots, bytes) != hipSuccess || hipMemset(*slots, 0xFF, bytes) != hipSuccess) return blk_refuse(who + ": no memory for the slots");
  return 0;
}
static void blk_slot_sum(double* slots, int parts) {
  hipLaunchKernelGGL(k_blk_slot_sum, dim3((kBnStride + 255) / 256), dim3(256), 0, nullptr, slots, parts);
}

// forward: Y [M,N] pre-BN in, x̂ out in place; out, rstd written; rm / rv (nullable) updated once (a rank's own copy: the first part's)
int t2l_blk_ft_bn_sync_fwd(float* Y, const int32_t* rows, int parts, int N, const float* g, const float* b, float* rm, float* rv,
                           float* rstd, float* out) {
  const std::string who = "t2l_blk_ft_bn_sync_fwd";
  if (!Y || !g || !b || !rstd || !out) return blk_refuse(who + ": null pointer");
  double* slots = nullptr;
  if (int rc = blk_sync_parts(who, rows, parts, N, &slots)) return rc;
  int64_t r0 = 0;
  for (int p = 0; p < parts; r0 += rows[p++]) bn_stats_fwd_launch(Y + r0 * N, rows[p], N, slots + (size_t)p * kBnStride, nullptr);
  blk_slot_sum(slots, parts);
  r0 = 0;
  for (int p = 0; p < parts; r0 += rows[p++])
    bn_apply_fwd_launch(Y + r0 * N, rows[p], N, g, b, p ? nullptr : rm, p ? nullptr : rv, rstd, out + r0 * N, slots + (size_t)p * kBnStride,
                        nullptr);
  const int rc = blk_finish("t2l_blk_ft_bn_sync_fwd");
  (void)hipFree(slots);
  return rc;
}

// backward: dy written; dg / db (nullable) get every part's own sums added (what the gradient all_reduce makes of the ranks')
int t2l_blk_ft_bn_sync_bwd(const float* dout, const float* out, const float* xhat, const float* rstd, const float* g, const int32_t* rows,
                           int parts, int N, float* dg, float* db, float* dy) {
  const std::string who = "t2l_blk_ft_bn_sync_bwd";
  if (!dout || !out || !xhat || !rstd || !g || !dy) return blk_refuse(who + ": null pointer");
  double* slots = nullptr;
  if (int rc = blk_sync_parts(who, rows, parts, N, &slots)) return rc;
  int64_t r0 = 0;
  for (int p = 0; p < parts; r0 += rows[p++])
    bn_stats_bwd_launch(dout + r0 * N, out + r0 * N, xhat + r0 * N, rows[p], N, dg, db, slots + (size_t)p * kBnStride, nullptr);
  blk_slot_sum(slots, parts);
  r0 = 0;
  for (int p = 0; p < parts; r0 += rows[p++])
    bn_apply_bwd_launch(dout + r0 * N, out + r0 * N, xhat + r0 * N, rstd, g, rows[p], N, slots + (size_t)p * kBnStride, dy + r0 * N, nullptr);
  const int rc = blk_finish("t2l_blk_ft_bn_sync_bwd");
  (void)hipFree(slots);
  return rc;
}

static int blk_attn_shape(const std::string& who, int Tq, int Tk, int pairs, float p) {
  if (Tq < 1 || Tq > kObj || Tk < 1 || Tk > kObj) return blk_refuse(who + ": Tq and Tk must be 1..16");
  if (pairs < 1 || pairs > (1 << 20)) return blk_refuse(who + ": pairs must be 1..2^20");
  if (blk_bad_p(p)) return blk_refuse(who + ": p must be in [0, 1)");
  return 0;
}

// cross-attention of `pairs` pairs, four heads of 32: Q[pairs*Tq] (ldq), K / V[pairs*Tk] (ldk / ldv) -> P[pairs,4,Tq,Tk] (before
// dropout), O[pairs*Tq] (ldo); (seed, site, p): the dropout site on the probabilities, through make_drop as dec_fwd does
int t2l_blk_ft_attn_fwd(const float* Q, int64_t ldq, const float* K, int64_t ldk, const float* V, int64_t ldv, int Tq, int Tk, int pairs,
                        float* P, float* O, int64_t ldo, uint32_t seed, int site, float p) {
  const std::string who = "t2l_blk_ft_attn_fwd";
  if (int rc = blk_attn_shape(who, Tq, Tk, pairs, p)) return rc;
  if (!Q || !K || !V || !P || !O) return blk_refuse(who + ": null pointer");
  if (ldq < kW || ldk < kW || ldv < kW || ldo < kW) return blk_refuse(who + ": every row stride must be >= 128");
  hipLaunchKernelGGL(k_attn_fwd, dim3(pairs * kHeads), dim3(256), 0, nullptr, Q, ldq, K, ldk, V, ldv, Tq, Tk, P, O, ldo, make_drop(seed, site, p));
  return blk_finish("t2l_blk_ft_attn_fwd");
}

int t2l_blk_ft_attn_bwd(const float* Q, int64_t ldq, const float* K, int64_t ldk, const float* V, int64_t ldv, const float* P, const float* dO,
                        int64_t lddo, float* dQ, int64_t lddq, float* dK, int64_t lddk, float* dV, int64_t lddv, int Tq, int Tk, int pairs,
                        uint32_t seed, int site, float p) {
  const std::string who = "t2l_blk_ft_attn_bwd";
  if (int rc = blk_attn_shape(who, Tq, Tk, pairs, p)) return rc;
  if (!Q || !K || !V || !P || !dO || !dQ || !dK || !dV) return blk_refuse(who + ": null pointer");
  if (ldq < kW || ldk < kW || ldv < kW || lddo < kW || lddq < kW || lddk < kW || lddv < kW)
    return blk_refuse(who + ": every row stride must be >= 128");
  hipLaunchKernelGGL(k_attn_bwd, dim3(pairs * kHeads), dim3(256), 0, nullptr, Q, ldq, K, ldk, V, ldv, P, dO, lddo, dQ, lddq, dK, lddk, dV, lddv,
                     Tq, Tk, make_drop(seed, site, p));
  return blk_finish("t2l_blk_ft_attn_bwd");
}

// out[M,128] = table[idx[m]] (a zero row for an index outside 0..rows-1)
int t2l_blk_ft_gather(const float* table, int rows, const int32_t* idx, int M, float* out) {
  const std::string who = "t2l_blk_ft_gather";
  if (!idx || !out) return blk_refuse(who + ": null idx / out");
  if (!table) return blk_refuse(who + ": an index array without a table");
  if (rows < 1 || M < 1) return blk_refuse(who + ": need rows, M >= 1");
  hipLaunchKernelGGL(k_gather, dim3(nblk((int64_t)M * kW, 256)), dim3(256), 0, nullptr, table, rows, idx, M, out);
  return blk_finish("t2l_blk_ft_gather");
}

// grad[idx[m]] += dY[m] for 0 < idx[m] < rows
int t2l_blk_ft_scatter_add(const float* dY, int rows, const int32_t* idx, int M, float* grad) {
  const std::string who = "t2l_blk_ft_scatter_add";
  if (!idx || !dY) return blk_refuse(who + ": null idx / dY");
  if (!grad) return blk_refuse(who + ": an index array without a table");
  if (rows < 1 || M < 1) return blk_refuse(who + ": need rows, M >= 1");
  hipLaunchKernelGGL(k_scatter_add, dim3(nblk((int64_t)M * kW, 256)), dim3(256), 0, nullptr, dY, rows, idx, M, grad);
  return blk_finish("t2l_blk_ft_scatter_add");
}

int t2l_blk_ft_num_in(const float* n_pts, int M, float* out) {
  const std::string who = "t2l_blk_ft_num_in";
  if (!n_pts || !out) return blk_refuse(who + ": null pointer");
  if (M < 1) return blk_refuse(who + ": need M >= 1");
  hipLaunchKernelGGL(k_num_in, dim3(nblk(M, 256)), dim3(256), 0, nullptr, n_pts, M, out);
  return blk_finish("t2l_blk_ft_num_in");
}

// One saved activation of the last forward: layer >= 0 a decoder layer in cascade order (qkv, Ps, os, xh1, r1, x1, q2, kv2, Pc, oc, xh2,
// r2, x2, h1, h1d, xh3, r3, out), layer -1 the encoder (class. / color. / position. / num. + raw | in | <i>.xhat | <i>.out | <i>.rstd |
// nrm; E, merge.*, pn_only.*, D0, nrm0, pool, arg (int32), a1). numel: the size the product planned (4-byte elements); dst holds cap.
int t2l_blk_ft_saved(t2l_ctx* ctx, int layer, const char* field, void* dst, int64_t cap, int64_t* numel) {
  const std::string who = "t2l_blk_ft_saved";
  if (!field || !numel) return blk_refuse(who + ": null field / numel");
  FineTrain* st = blk_state(who, ctx, layer, true);
  if (!st) return -1;
  const void* src = nullptr;
  int64_t n = 0;
  if (!blk_field(st, layer, field, &src, &n) || !src) return blk_refuse(who + ": this configuration has no field " + field);
  *numel = n;
  if (!dst) return 0;  // the size alone
  if (cap < n) return blk_refuse(who + ": dst is too small for " + field);
  if (hipSetDevice(ctx->device) != hipSuccess) return blk_refuse(who + ": no device");
  if (hipStreamSynchronize(nullptr) != hipSuccess || hipMemcpy(dst, src, (size_t)n * 4, hipMemcpyDeviceToDevice) != hipSuccess) {
    blk_refuse(who + ": copy failed");
    return -2;
  }
  return blk_finish("t2l_blk_ft_saved");
}

// the product's dec_bwd on decoder layer `layer` of the bound state with the last forward's (seed, p): dx [P*Tq,128] written,
// d mem ADDED into dmem [P*Tk,128], the layer's parameter gradients ADDED into the bound .grad tensors
int t2l_blk_ft_dec_bwd(t2l_ctx* ctx, int layer, const float* dout, float* dx, float* dmem) {
  const std::string who = "t2l_blk_ft_dec_bwd";
  FineTrain* st = blk_state(who, ctx, layer, false);
  if (!st) return -1;
  if (!dout || !dx || !dmem) return blk_refuse(who + ": null pointer");
  if (hipSetDevice(ctx->device) != hipSuccess) return blk_refuse(who + ": no device");
  if (!dec_bwd(st, st->dec[layer], st->p, st->seed, dout, dx, dmem, nullptr)) return blk_refuse(who + ": a row kernel has no instance of width 128");
  return blk_finish("t2l_blk_ft_dec_bwd");
}

}  // extern "C"
