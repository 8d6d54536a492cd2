// Pretraining the PointNet++ object backbone as a classifier: the two Linear(256, .) heads over features2
// (models/pointcloud/pointnet2.py:64-65, 91-92: class_pred = class_classifier(features2), color_pred = color_classifier(features2)),
// their softmax cross-entropy, and the backward of both — ONE launch (heads_kernel), forward + backward, as the contrastive and
// ranking losses are (loss.hip): n is a host argument, so the mean's 1/n is known ahead. The step is latency bound
// (2 * n * 256 * 30 FLOP); a workgroup of 256 threads owns kClsRows rows and keeps BOTH weight matrices (30 KB today) and its rows
// of features2 in LDS.
//
//   logits[r][c]  = b[c] + sum_k x[r][k] W[c][k]                          (class head: columns 0..C1-1, colour head: C1..C1+C2-1)
//   per head h:     m = max_c l, Z = sum_c exp(l - m), CE_r = log Z + m - l[label_r]; first arg-max == label_r -> correct[h] += 1
//   loss[h]       = (1/n) sum_r CE_r                                       float64 partial per workgroup, fixed-order final sum
//   G[r][c]       = w_h (exp(l - m) / Z - [c == label_r]) / n             = d (w_class loss[0] + w_color loss[1]) / d logits
//   d features2   = G W;   dW += G^T x;   db += column sums of G
//
// dW and db are reduced over the workgroup's rows before anything leaves it; the sum over workgroups is unsafeAtomicAdd into the bound
// gradient buffers (as train_kernels.h does), so with more than kClsRows rows the LAST BITS of the four head gradients depend on the
// run. Everything else has a fixed order: logits, loss, counts and d features2 are the same bits every run (the loss and the counts
// are per-workgroup partials, summed in workgroup order by whichever workgroup arrives last).
//
// The t2l_pointnet_cls_* entry points are at the end: a ClsTrain owns its own PnTrain (pointnet_train.h, through the
// pn_train_*_on doors), as ft::FineTrain does; the state of t2l_train_bind is never touched.
#include <math.h>
#include <string.h>

#include "t2l_internal.h"

namespace t2l {
namespace cls {

constexpr int kClsRows = 32;                 // rows of features2 per workgroup
constexpr int kClsMaxC = T2L_CLS_MAX_CLASSES;  // classes per head (2 <= C <= 32)
constexpr int kCt = 2 * kClsMaxC;            // logit columns held per row (both heads; unused ones are zero)
constexpr int kLd = 257;                     // row stride of the [.][256] LDS planes: column reads of consecutive rows hit distinct banks
constexpr int kLdg = kCt + 1;
constexpr size_t kClsLds = sizeof(float) * ((size_t)kCt * kLd + (size_t)kClsRows * kLd + (size_t)kClsRows * kLdg + kCt) +
                           sizeof(double) * 2 * kClsRows + sizeof(int) * (2 * kClsRows + 1);

struct HeadsArgs {
  const float* x;                 // features2 [n][256]
  const float *wc, *bc, *wk, *bk;  // class_classifier / color_classifier weight [C][256], bias [C]
  float *gwc, *gbc, *gwk, *gbk;   // their gradient buffers (read only when dx != nullptr)
  const int32_t *lc, *lk;         // labels [n] (device copies of the checked host arrays)
  int n, c1, c2;
  float w1, w2, inv_n;
  float* logits;                  // [n][c1 + c2] or nullptr
  float* loss;                    // [2]
  int32_t* correct;               // [2]
  float* dx;                      // [n][256] or nullptr (forward only: no gradient buffer is touched)
  double* part_loss;              // [grid][2]
  int32_t* part_ok;               // [grid][2]
  unsigned* ticket;               // zero before the launch
};

__global__ __launch_bounds__(256, 1) void heads_kernel(HeadsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sW = smem;                        // [kCt][kLd]: rows 0..c1-1 class, c1..ct-1 colour, the rest zero
  float* sX = sW + kCt * kLd;              // [kClsRows][kLd], rows past n zero
  float* sG = sX + kClsRows * kLd;         // [kClsRows][kLdg]: logits, then G (columns past ct and rows past n zero)
  float* sB = sG + kClsRows * kLdg;        // [kCt]
  double* sCe = reinterpret_cast<double*>(sB + kCt);  // [kClsRows][2]
  int* sOk = reinterpret_cast<int*>(sCe + 2 * kClsRows);  // [kClsRows][2]
  int* sLast = sOk + 2 * kClsRows;
  const int tid = threadIdx.x, ct = a.c1 + a.c2;
  const int r0 = blockIdx.x * kClsRows, nr = min(kClsRows, a.n - r0);

  // 1. operands into LDS (global reads coalesced along k)
  for (int c = tid >> 6; c < kCt; c += 4) {
    const float* src = c < a.c1 ? a.wc + (size_t)c * 256 : c < ct ? a.wk + (size_t)(c - a.c1) * 256 : nullptr;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = (tid & 63) + 64 * q;
      sW[c * kLd + k] = src ? src[k] : 0.f;
    }
  }
  for (int r = tid >> 6; r < kClsRows; r += 4) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = (tid & 63) + 64 * q;
      sX[r * kLd + k] = r < nr ? a.x[(size_t)(r0 + r) * 256 + k] : 0.f;
    }
  }
  if (tid < kCt) sB[tid] = tid < a.c1 ? a.bc[tid] : tid < ct ? a.bk[tid - a.c1] : 0.f;
  __syncthreads();

  // 2. logits: lane = column (a row of W per lane, bank c + k), wave w takes rows w, w + 4, ...
  {
    const int c = tid & 63;
    const float* wrow = sW + c * kLd;
    for (int r = tid >> 6; r < kClsRows; r += 4) {
      const float* xrow = sX + r * kLd;
      float acc = 0.f;
#pragma unroll 16
      for (int k = 0; k < 256; ++k) acc = __fmaf_rn(xrow[k], wrow[k], acc);
      const float l = acc + sB[c];
      sG[r * kLdg + c] = l;
      if (a.logits && r < nr && c < ct) a.logits[(size_t)(r0 + r) * ct + c] = l;
    }
  }
  __syncthreads();

  // 3. softmax cross-entropy of one (row, head) per thread; G over the logits
  if (tid < 2 * kClsRows) {
    const int r = tid >> 1, h = tid & 1;
    const int lo = h ? a.c1 : 0, C = h ? a.c2 : a.c1;
    float* g = sG + r * kLdg + lo;
    double ce = 0.0;
    int ok = 0;
    if (r < nr) {
      const int label = h ? a.lk[r0 + r] : a.lc[r0 + r];
      float m = g[0];
      int am = 0;
      for (int c = 1; c < C; ++c)
        if (g[c] > m) {  // first maximum: ties go to the lower index
          m = g[c];
          am = c;
        }
      float z = 0.f;
      for (int c = 0; c < C; ++c) z += expf(g[c] - m);
      ce = (double)(logf(z) + (m - g[label]));
      ok = am == label;
      const float sc = (h ? a.w2 : a.w1) * a.inv_n, iz = 1.f / z;
      for (int c = 0; c < C; ++c) g[c] = (expf(g[c] - m) * iz - (c == label ? 1.f : 0.f)) * sc;
    } else {
      for (int c = 0; c < C; ++c) g[c] = 0.f;
    }
    if (h)
      for (int c = ct; c < kCt; ++c) sG[r * kLdg + c] = 0.f;
    sCe[2 * r + h] = ce;
    sOk[2 * r + h] = ok;
  }
  __syncthreads();

  // loss and counts: this workgroup's partial in row order; the last workgroup to arrive adds the partials in workgroup order
  if (tid < 2) {
    double s = 0.0;
    int k = 0;
    for (int r = 0; r < kClsRows; ++r) {
      s += sCe[2 * r + tid];
      k += sOk[2 * r + tid];
    }
    a.part_loss[2 * blockIdx.x + tid] = s;
    a.part_ok[2 * blockIdx.x + tid] = k;
    __threadfence();
  }
  __syncthreads();
  if (tid == 0) sLast[0] = atomicAdd(a.ticket, 1u) == gridDim.x - 1;
  __syncthreads();
  if (sLast[0] && tid < 2) {
    __threadfence();
    double s = 0.0;
    int k = 0;
    for (unsigned b = 0; b < gridDim.x; ++b) {
      s += __hip_atomic_load(a.part_loss + 2 * b + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      k += __hip_atomic_load(a.part_ok + 2 * b + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    a.loss[tid] = (float)(s * (double)a.inv_n);
    a.correct[tid] = k;
  }
  if (!a.dx) return;

  // 4. d features2 = G W: thread = column k with W's column in registers, G broadcast from LDS
  {
    float wcol[kCt];
#pragma unroll
    for (int c = 0; c < kCt; ++c) wcol[c] = sW[c * kLd + tid];
    for (int r = 0; r < nr; ++r) {
      const float* g = sG + r * kLdg;
      float acc = 0.f;
#pragma unroll
      for (int c = 0; c < kCt; ++c) acc = __fmaf_rn(g[c], wcol[c], acc);
      a.dx[(size_t)(r0 + r) * 256 + tid] = acc;
    }
  }
  // 5. dW += G^T x (this workgroup's rows summed first), db += column sums of G
  {
    float xcol[kClsRows];
#pragma unroll
    for (int r = 0; r < kClsRows; ++r) xcol[r] = sX[r * kLd + tid];
    for (int c = 0; c < ct; ++c) {
      float acc = 0.f;
#pragma unroll
      for (int r = 0; r < kClsRows; ++r) acc = __fmaf_rn(sG[r * kLdg + c], xcol[r], acc);
      float* dst = c < a.c1 ? a.gwc + (size_t)c * 256 : a.gwk + (size_t)(c - a.c1) * 256;
      unsafeAtomicAdd(dst + tid, acc);
    }
    if (tid < ct) {
      float acc = 0.f;
      for (int r = 0; r < kClsRows; ++r) acc += sG[r * kLdg + tid];
      unsafeAtomicAdd(tid < a.c1 ? a.gbc + tid : a.gbk + (tid - a.c1), acc);
    }
  }
}

struct Head {
  float *w = nullptr, *b = nullptr, *gw = nullptr, *gb = nullptr;
  int c = 0;
};

struct ClsTrain {
  PnTrain* pn = nullptr;
  Head h[2];  // class_classifier, color_classifier
  char* ws = nullptr;  // [grid][2] float64 + [grid][2] int32 partials, then the ticket
  size_t ws_cap = 0;
  int n_fwd = 0;  // objects of the last t2l_pointnet_cls_forward (0: none to differentiate)
};

static ClsTrain* cls_state(t2l_ctx* ctx) { return reinterpret_cast<ClsTrain*>(ctx->cls_train); }

static void free_cls(ClsTrain* st) {
  if (!st) return;
  pn_train_release(st->pn);
  if (st->ws) (void)hipFree(st->ws);
  delete st;
}

}  // namespace cls

void free_cls_train(t2l_ctx* ctx) {
  cls::free_cls(cls::cls_state(ctx));
  ctx->cls_train = nullptr;
}

int cls_bind_impl(t2l_ctx* ctx, const t2l_train_tensor* tensors, int n) {
  using namespace cls;
  const std::string who = "t2l_pointnet_cls_bind";
  if (!tensors || n <= 0) return fail(ctx, T2L_EINVAL, who + ": null/empty arguments");
  const std::string P = "object_encoder.pointnet.";
  const char* heads[2] = {"class_classifier", "color_classifier"};
  auto* st = new ClsTrain();
  auto refuse = [&](int rc, const std::string& msg) {  // the previous binding stays as it is
    free_cls(st);
    return msg.empty() ? rc : fail(ctx, rc, msg);
  };
  for (int h = 0; h < 2; ++h) {
    const t2l_train_tensor *w = nullptr, *b = nullptr;
    for (int i = 0; i < n; ++i) {
      if (!tensors[i].name || !tensors[i].data) continue;
      if (P + heads[h] + ".weight" == tensors[i].name) w = &tensors[i];
      if (P + heads[h] + ".bias" == tensors[i].name) b = &tensors[i];
    }
    if (!w || !b) return refuse(T2L_EINVAL, who + ": missing tensor '" + P + heads[h] + (w ? ".bias'" : ".weight'"));
    if (!w->grad || !b->grad)
      return refuse(T2L_EINVAL, who + ": '" + P + heads[h] + ".*' must be bound with gradient buffers (the heads are what this step trains)");
    const int64_t C = b->numel;
    if (C < 2 || C > kClsMaxC)
      return refuse(T2L_EINVAL, who + ": '" + P + heads[h] + ".bias' has " + std::to_string(C) + " elements; a head has 2 <= C <= " +
                                    std::to_string(kClsMaxC) + " classes");
    if (w->numel != C * 256)
      return refuse(T2L_EINVAL, who + ": '" + P + heads[h] + ".weight' has " + std::to_string(w->numel) + " elements, expected " +
                                    std::to_string(C * 256));
    st->h[h] = Head{w->data, b->data, w->grad, b->grad, (int)C};
  }
  if (int rc = pn_train_bind_group(ctx, tensors, n, who.c_str(), &st->pn)) return refuse(rc, "");
  if (!st->pn)
    return refuse(T2L_EINVAL, who + ": object_encoder.pointnet.* must be bound completely — every sa*/ga/lin1/lin2 tensor, all of them with "
                                    "gradient buffers or none (a frozen backbone trains the heads only)");
  T2L_HIP(ctx, hipDeviceSynchronize());  // nothing of the old binding is in flight when it goes
  free_cls_train(ctx);
  ctx->cls_train = st;
  return T2L_OK;
}

int cls_forward_impl(t2l_ctx* ctx, const float* pos, const float* rgb, int n_objects, float* out_f2, hipStream_t s) {
  using namespace cls;
  ClsTrain* st = cls_state(ctx);
  if (!st) return fail(ctx, T2L_ESTATE, "t2l_pointnet_cls_forward: bind the backbone and the heads first (t2l_pointnet_cls_bind)");
  if (!pos || !rgb || !out_f2 || n_objects <= 0) return fail(ctx, T2L_EINVAL, "t2l_pointnet_cls_forward: bad arguments");
  st->n_fwd = 0;
  const int32_t offs[2] = {0, n_objects};  // ONE segment: every BatchNorm sees the whole batch, one running-statistics update
  const float* f2 = nullptr;
  if (int rc = pn_train_forward_on(ctx, st->pn, "t2l_pointnet_cls_forward", pos, rgb, offs, 1, &f2, s)) return rc;
  T2L_HIP(ctx, hipMemcpyAsync(out_f2, f2, sizeof(float) * (size_t)n_objects * 256, hipMemcpyDeviceToDevice, s));
  st->n_fwd = n_objects;
  return T2L_OK;
}

int cls_heads_impl(t2l_ctx* ctx, const float* f2, int n, const int32_t* class_labels, const int32_t* color_labels, float w_class,
                   float w_color, float* out_logits, float* out_loss, int32_t* out_correct, float* grad_f2, hipStream_t s) {
  using namespace cls;
  const char* who = "t2l_pointnet_cls_heads: ";
  ClsTrain* st = cls_state(ctx);
  if (!st) return fail(ctx, T2L_ESTATE, std::string(who) + "bind the backbone and the heads first (t2l_pointnet_cls_bind)");
  if (n <= 0) return fail(ctx, T2L_EINVAL, std::string(who) + "need n >= 1");
  if (!f2 || !class_labels || !color_labels || !out_loss || !out_correct) return fail(ctx, T2L_EINVAL, std::string(who) + "null argument");
  if (!isfinite(w_class) || !isfinite(w_color)) return fail(ctx, T2L_EINVAL, std::string(who) + "w_class and w_color must be finite");
  if (((uintptr_t)f2 | (uintptr_t)out_logits | (uintptr_t)out_loss | (uintptr_t)out_correct | (uintptr_t)grad_f2) % 4 != 0)
    return fail(ctx, T2L_EINVAL, std::string(who) + "device arrays must be 4-byte aligned");
  const int32_t* lab[2] = {class_labels, color_labels};
  const char* lname[2] = {"class_labels", "color_labels"};
  for (int h = 0; h < 2; ++h)
    for (int r = 0; r < n; ++r)
      if (lab[h][r] < 0 || lab[h][r] >= st->h[h].c)
        return fail(ctx, T2L_EINVAL, std::string(who) + lname[h] + "[" + std::to_string(r) + "] = " + std::to_string(lab[h][r]) +
                                         " is outside [0, " + std::to_string(st->h[h].c) + ")");
  const int grid = (n + kClsRows - 1) / kClsRows;
  const size_t need = (size_t)grid * (2 * sizeof(double) + 2 * sizeof(int32_t)) + 256;
  if (need > st->ws_cap) {
    T2L_HIP(ctx, hipStreamSynchronize(s));
    if (st->ws) (void)hipFree(st->ws);
    st->ws = nullptr;
    st->ws_cap = 0;
    T2L_HIP(ctx, hipMalloc(&st->ws, need * 2));
    st->ws_cap = need * 2;
  }
  static PerDeviceOnce attr_done;
  if (attr_done.need(ctx->device)) {
    T2L_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&heads_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kClsLds));
    attr_done.mark(ctx->device);
  }
  const int32_t* d_lc;
  const uint32_t* d_lk;
  const uint8_t* unused;
  if (int rc = stage_rows(ctx, who, class_labels, reinterpret_cast<const uint32_t*>(color_labels), nullptr, n, s, &d_lc, &d_lk, &unused)) return rc;
  HeadsArgs a;
  a.x = f2;
  a.wc = st->h[0].w; a.bc = st->h[0].b; a.wk = st->h[1].w; a.bk = st->h[1].b;
  a.gwc = st->h[0].gw; a.gbc = st->h[0].gb; a.gwk = st->h[1].gw; a.gbk = st->h[1].gb;
  a.lc = d_lc;
  a.lk = reinterpret_cast<const int32_t*>(d_lk);
  a.n = n; a.c1 = st->h[0].c; a.c2 = st->h[1].c;
  a.w1 = w_class; a.w2 = w_color; a.inv_n = 1.0f / (float)n;
  a.logits = out_logits; a.loss = out_loss; a.correct = out_correct; a.dx = grad_f2;
  a.part_loss = reinterpret_cast<double*>(st->ws);
  a.part_ok = reinterpret_cast<int32_t*>(st->ws + (size_t)grid * 2 * sizeof(double));
  a.ticket = reinterpret_cast<unsigned*>(st->ws + (size_t)grid * (2 * sizeof(double) + 2 * sizeof(int32_t)));
  T2L_HIP(ctx, hipMemsetAsync(a.ticket, 0, sizeof(unsigned), s));
  event_begin(ctx, "pointnet_cls_heads", s);
  hipLaunchKernelGGL(heads_kernel, dim3(grid), dim3(256), kClsLds, s, a);
  event_end(ctx, "pointnet_cls_heads", s);
  return stage_rows_done(ctx, s);
}

int cls_backward_impl(t2l_ctx* ctx, const float* grad_f2, hipStream_t s) {
  using namespace cls;
  ClsTrain* st = cls_state(ctx);
  if (!st) return fail(ctx, T2L_ESTATE, "t2l_pointnet_cls_backward: bind the backbone and the heads first (t2l_pointnet_cls_bind)");
  if (!st->n_fwd) return fail(ctx, T2L_ESTATE, "t2l_pointnet_cls_backward: no t2l_pointnet_cls_forward to differentiate");
  return pn_train_backward_on(ctx, st->pn, "t2l_pointnet_cls_backward", grad_f2, s);
}

}  // namespace t2l
