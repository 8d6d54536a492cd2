// C ABI of libt2l.so (see include/t2l.h): context, database shard, options, timing.
#include <limits.h>
#include <math.h>
#include <string.h>

#include "t2l_internal.h"

namespace t2l {

int fail(t2l_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  return code;
}

void event_begin(t2l_ctx* ctx, const char* name, hipStream_t s) {
  if (!ctx->profile_events) return;
  EventRing& e = ctx->events[name];
  if (e.a.empty()) {
    e.a.resize(kEventRing);
    e.b.resize(kEventRing);
    for (int i = 0; i < kEventRing; ++i) {
      (void)hipEventCreate(&e.a[i]);
      (void)hipEventCreate(&e.b[i]);
    }
  }
  e.open = (e.calls++ % ctx->profile_events) == 0;
  if (e.open) (void)hipEventRecord(e.a[e.head], s);
}

// The cheap form for a SINGLE kernel: hand the pair to hipExtLaunchKernelGGL, which stamps the dispatch itself (start / end
// of the kernel from its completion signal) instead of putting two marker packets around it on the stream — markers break
// back-to-back dispatch (~3.5 us each beside a 50 us step). Returns false when this launch is not a sampled one.
bool event_pair(t2l_ctx* ctx, const char* name, hipEvent_t* a, hipEvent_t* b) {
  if (!ctx->profile_events) return false;
  EventRing& e = ctx->events[name];
  if (e.a.empty()) {
    e.a.resize(kEventRing);
    e.b.resize(kEventRing);
    for (int i = 0; i < kEventRing; ++i) {
      (void)hipEventCreate(&e.a[i]);
      (void)hipEventCreate(&e.b[i]);
    }
  }
  if ((e.calls++ % ctx->profile_events) != 0) return false;
  *a = e.a[e.head];
  *b = e.b[e.head];
  e.head = (e.head + 1) % kEventRing;
  if (e.count < kEventRing) ++e.count;
  return true;
}

void event_end(t2l_ctx* ctx, const char* name, hipStream_t s) {
  if (!ctx->profile_events) return;
  EventRing& e = ctx->events[name];
  if (!e.open) return;
  e.open = false;
  (void)hipEventRecord(e.b[e.head], s);
  e.head = (e.head + 1) % kEventRing;
  if (e.count < kEventRing) ++e.count;
}

int upload_staging(t2l_ctx* ctx, const char* who, const Staging& st, char** blob) {
  char* d = nullptr;
  if (hipMalloc(&d, st.bytes()) != hipSuccess) return fail(ctx, T2L_ENOMEM, std::string(who) + ": hipMalloc of " + std::to_string(st.bytes()) + " bytes failed");
  if (hipMemcpy(d, st.data(), st.bytes(), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(d);
    return fail(ctx, T2L_EHIP, std::string(who) + ": upload failed");
  }
  st.bind(d);
  *blob = d;
  return T2L_OK;
}

// A state dict's optional object_encoder.pointnet.* group is validated before `load` (which validates, then commits its own part)
// and committed after it: a list either part refuses changes neither.
template <typename Load>
int load_with_backbone(t2l_ctx* ctx, const char* who, const t2l_weight_desc* w, int n, Load load) {
  PointNetStaged* pn = nullptr;
  int rc = pointnet_stage(ctx, who, w, n, &pn);
  if (rc) return rc;
  if ((rc = load())) {
    pointnet_discard(pn);
    return rc;
  }
  return pointnet_commit(ctx, who, pn);
}

}  // namespace t2l

using namespace t2l;

extern "C" {

int t2l_abi_version(void) { return T2L_ABI_VERSION; }

int t2l_create(t2l_ctx** out, int device_id) {
  if (!out) return T2L_EINVAL;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device_id < 0 || device_id >= n) return T2L_EHIP;
  if (hipSetDevice(device_id) != hipSuccess) return T2L_EHIP;
  t2l_ctx* ctx = new t2l_ctx();
  ctx->device = device_id;
  if (hipMalloc(&ctx->db_norm_max, (2 + 256) * sizeof(float)) != hipSuccess ||
      hipMalloc(&ctx->fb_count, 2 * kBankInts * sizeof(int32_t)) != hipSuccess) {
    delete ctx;
    return T2L_ENOMEM;
  }
  (void)hipMemset(ctx->db_norm_max, 0, (2 + 256) * sizeof(float));
  if (hipHostMalloc((void**)&ctx->host_stat, kStatInts * sizeof(int32_t), hipHostMallocMapped) == hipSuccess) {
    memset(ctx->host_stat, 0, kStatInts * sizeof(int32_t));
    if (hipHostGetDevicePointer((void**)&ctx->host_stat_dev, ctx->host_stat, 0) != hipSuccess) ctx->host_stat_dev = nullptr;
  }
  (void)hipMemset(ctx->fb_count, 0, 2 * kBankInts * sizeof(int32_t));
  ctx->fb_prev = ctx->fb_count + kBankInts;  // two banks (t2l_internal.h: CounterSlot)
  if (hipMalloc(&ctx->scan_span, sizeof(unsigned long long) * 2 * kSpanWgs * kSpanRing) == hipSuccess) {
    (void)hipMemset(ctx->scan_span, 0, sizeof(unsigned long long) * 2 * kSpanWgs * kSpanRing);
    ctx->span_grid = new unsigned[kSpanRing]();
  }
  else
    ctx->scan_span = nullptr;
  *out = ctx;
  return T2L_OK;
}

void t2l_destroy(t2l_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipDeviceSynchronize();
  free_weights(ctx);
  free_train(ctx);
  free_text_train(ctx);
  free_pointnet(ctx);
  free_sample_stage(ctx);
  free_fine(ctx);
  free_fine_train(ctx);
  free_cls_train(ctx);
  free_text_head(ctx);
  for (void* p : {(void*)ctx->db, (void*)ctx->db_split, (void*)ctx->db_half, (void*)ctx->db_norm_max, (void*)ctx->cand_score, (void*)ctx->seg_idx,
                  (void*)ctx->seg_score, (void*)ctx->flags, (void*)(ctx->fb_count < ctx->fb_prev ? ctx->fb_count : ctx->fb_prev), ctx->fast_ws, (void*)ctx->fast_zero, ctx->reduce_ws, ctx->loss_ws, (void*)ctx->small_ticket, ctx->small_part, (void*)ctx->scan_span})
    if (p) (void)hipFree(p);
  delete[] ctx->span_grid;
  if (ctx->host_stat) (void)hipHostFree(ctx->host_stat);
  free_lanes(ctx);
  for (auto& kv : ctx->events) {
    for (hipEvent_t ev : kv.second.a) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : kv.second.b) (void)hipEventDestroy(ev);
  }
  delete ctx;
}

const char* t2l_last_error(const t2l_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int t2l_load_weights(t2l_ctx* ctx, const t2l_weight_desc* w, int32_t n, const t2l_model_config* cfg) {
  if (!ctx) return T2L_EINVAL;
  if (!w || n <= 0 || !cfg) return fail(ctx, T2L_EINVAL, "t2l_load_weights: null/empty arguments");
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return load_with_backbone(ctx, "t2l_load_weights", w, n, [&] { return load_weights_impl(ctx, w, n, cfg, T2L_EMBED_DIM, T2L_OBJECT_SIZE); });
}

int t2l_load_weights_shaped(t2l_ctx* ctx, const t2l_weight_desc* w, int32_t n, const t2l_model_config* cfg, const t2l_model_shape* shape) {
  if (!ctx) return T2L_EINVAL;
  if (!w || n <= 0 || !cfg || !shape) return fail(ctx, T2L_EINVAL, "t2l_load_weights_shaped: null/empty arguments");
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return load_with_backbone(ctx, "t2l_load_weights", w, n,
                            [&] { return load_weights_impl(ctx, w, n, cfg, shape->embed_dim, shape->object_size); });
}

int t2l_embed_dim(const t2l_ctx* ctx) { return ctx ? encoder_embed_dim(ctx) : T2L_EINVAL; }

int t2l_sample_object_points(t2l_ctx* ctx, const float* xyz, const float* rgb, const int64_t* point_offsets, int32_t n_objects,
                             uint32_t seed, int32_t transform_flags, float rotate_deg, float* out_pos, float* out_rgb, void* stream) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return sample_points_impl(ctx, xyz, rgb, point_offsets, n_objects, seed, transform_flags, rotate_deg, out_pos, out_rgb, (hipStream_t)stream);
}

int t2l_sample_object_points_indexed(t2l_ctx* ctx, const float* xyz, const float* rgb, const int64_t* point_offsets, int32_t n_objects,
                                     const int32_t* object_ids, const uint32_t* salts, int32_t n_rows, uint32_t seed,
                                     int32_t transform_flags, float rotate_deg, float* out_pos, float* out_rgb, void* stream) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return sample_points_rows_impl(ctx, "t2l_sample_object_points_indexed: ", xyz, rgb, point_offsets, n_objects, object_ids, salts, nullptr,
                                 n_rows, seed, transform_flags, rotate_deg, out_pos, out_rgb, (hipStream_t)stream);
}

int t2l_sample_object_points_mirrored(t2l_ctx* ctx, const float* xyz, const float* rgb, const int64_t* point_offsets, int32_t n_objects,
                                      const int32_t* object_ids, const uint32_t* salts, const uint8_t* mirror, int32_t n_rows, uint32_t seed,
                                      int32_t transform_flags, float rotate_deg, float* out_pos, float* out_rgb, void* stream) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return sample_points_rows_impl(ctx, "t2l_sample_object_points_mirrored: ", xyz, rgb, point_offsets, n_objects, object_ids, salts, mirror,
                                 n_rows, seed, transform_flags, rotate_deg, out_pos, out_rgb, (hipStream_t)stream);
}

int t2l_gather_object_rows(t2l_ctx* ctx, const int32_t* class_idx, const int32_t* color_idx, const float* rgb, const float* center,
                           const float* n_pts, int32_t n_objects, const int32_t* object_ids, const uint8_t* mirror, int32_t n_rows,
                           int32_t* out_class_idx, int32_t* out_color_idx, float* out_rgb, float* out_center, float* out_n_pts,
                           void* stream) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return gather_rows_impl(ctx, class_idx, color_idx, rgb, center, n_pts, n_objects, object_ids, mirror, n_rows, out_class_idx,
                          out_color_idx, out_rgb, out_center, out_n_pts, (hipStream_t)stream);
}

int t2l_pointnet_features(t2l_ctx* ctx, const float* pos, const float* rgb, const int32_t* cell_offsets, int32_t n_cells,
                          float* out_features2, void* stream) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return pointnet_features_impl(ctx, pos, rgb, cell_offsets, n_cells, out_features2, (hipStream_t)stream);
}

int t2l_encode_cells(t2l_ctx* ctx, const t2l_packed_cells* in, float* out_emb, void* stream) {
  if (!ctx) return T2L_EINVAL;
  if (!in || in->n_cells < 0 || in->n_objects < 0) return fail(ctx, T2L_EINVAL, "t2l_encode_cells: bad arguments");
  if (in->n_cells == 0) return T2L_OK;
  if (!out_emb || !in->offsets) return fail(ctx, T2L_EINVAL, "t2l_encode_cells: null buffer");
  if (!ctx->enc) return fail(ctx, T2L_ESTATE, "t2l_encode_cells: weights not loaded (call t2l_load_weights)");
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return encode_impl(ctx, in, out_emb, (hipStream_t)stream);
}

int t2l_reduce_objects(t2l_ctx* ctx, const float* xyz, const float* rgb, const int64_t* point_offsets, int32_t n_objects,
                       const float* color_centers, const int32_t* color_rows, int32_t n_colors, float* out_rgb,
                       float* out_center, float* out_npts, int32_t* out_color_idx, void* stream) {
  if (!ctx) return T2L_EINVAL;
  if (n_objects < 0) return fail(ctx, T2L_EINVAL, "t2l_reduce_objects: n_objects < 0");
  if (n_objects == 0) return T2L_OK;
  if (!xyz || !rgb || !point_offsets || !color_centers || !color_rows || !out_rgb || !out_center || !out_npts ||
      !out_color_idx)
    return fail(ctx, T2L_EINVAL, "t2l_reduce_objects: null buffer");
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return reduce_impl(ctx, xyz, rgb, point_offsets, n_objects, color_centers, color_rows, n_colors, out_rgb, out_center,
                     out_npts, out_color_idx, (hipStream_t)stream);
}

int t2l_db_set(t2l_ctx* ctx, const float* emb, int64_t n_rows, int64_t row_offset, void* stream) {
  if (!ctx) return T2L_EINVAL;
  if (n_rows < 0 || (n_rows > 0 && !emb)) return fail(ctx, T2L_EINVAL, "t2l_db_set: bad arguments");
  if (n_rows + row_offset >= (int64_t)INT32_MAX) return fail(ctx, T2L_EINVAL, "t2l_db_set: row ids must fit int32");
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  {  // pipelined searches still in flight read the planes this call rewrites
    const int rc = search_join_impl(ctx, s);
    if (rc != T2L_OK) return rc;
  }
  const int64_t pad = (n_rows + kTileRows - 1) / kTileRows * kTileRows;
  if (pad > ctx->db_cap) {
    T2L_HIP(ctx, hipStreamSynchronize(s));
    if (ctx->db) (void)hipFree(ctx->db);
    if (ctx->db_split) (void)hipFree(ctx->db_split);
    if (ctx->db_half) (void)hipFree(ctx->db_half);
    ctx->db = nullptr;
    ctx->db_split = nullptr;
    ctx->db_half = nullptr;
    ctx->db_cap = 0;
    T2L_HIP(ctx, hipMalloc(&ctx->db, (size_t)pad * kD * sizeof(float)));
    T2L_HIP(ctx, hipMalloc(&ctx->db_split, (size_t)pad * kD * sizeof(float)));
    T2L_HIP(ctx, hipMalloc(&ctx->db_half, (size_t)pad * kD * 2));
    ctx->db_cap = pad;
  }
  ctx->db_rows = n_rows;
  // a new database: what earlier report cards said about the previous one (split-bf16 stand-in, heavy / all-exact mode) is void,
  // and so is every report of a search still in flight
  if (ctx->search_auto) ctx->policy.reset(true);  // (the NEXT call's re-rank still publishes the report of the last call on the old rows)
  ctx->db_pad = pad;
  ctx->row_offset = row_offset;
  if (n_rows > 0) {
    T2L_HIP(ctx, hipMemcpyAsync(ctx->db, emb, (size_t)n_rows * kD * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (pad > n_rows)
      T2L_HIP(ctx, hipMemsetAsync(ctx->db + (size_t)n_rows * kD, 0, (size_t)(pad - n_rows) * kD * sizeof(float), s));
  }
  int rc = db_norm_impl(ctx, s);
  if (rc != T2L_OK) return rc;
  T2L_HIP(ctx, hipStreamSynchronize(s));
  // A PRIOR for the first searches on this database (round 5). db_norm_impl left the sum S of up to 1,024 sampled rows, each
  // normalised: (|S|^2 - n) / (n (n - 1)) is the sample's mean pairwise cosine. Above 0.9 the rows are nearly parallel — what an
  // untrained encoder produces over overlapping cells, i.e. every validation pass of the first training epochs — and the f16
  // certificates fail wholesale: without a prior the first call on such a database sends ~4,000 of 4,096 queries to the re-rank
  // workgroups' own exact scans (3.3 ms; measured on bench.py's cold end-to-end line: 6.8 ms per encode + db_set + search against
  // 3.4 with the prior), and t2l_db_set voids the report cards that would have said so. The prior only picks the starting MODE
  // (split-bf16 stand-in scan, unsettled queries deferred to the float64 MFMA stage); results are exact in every mode and the first
  // report cards correct a wrong guess within two calls (cost of a wrong guess: one near-empty launch per call).
  if (ctx->search_auto && ctx->knobs.search_mode == 0 && n_rows >= 64) {
    float cols[256];
    T2L_HIP(ctx, hipMemcpy(cols, ctx->db_norm_max + 2, sizeof(cols), hipMemcpyDeviceToHost));
    double ss = 0.0;
    for (float c : cols) ss += (double)c * c;
    const double n = (double)std::min<int64_t>(n_rows, 1024);
    const double mean_cos = (ss - n) / (n * (n - 1.0));
    ctx->policy.seed_from_prior(mean_cos);
  }
  return T2L_OK;
}

int64_t t2l_db_rows(const t2l_ctx* ctx) { return ctx ? ctx->db_rows : -1; }

int t2l_search(t2l_ctx* ctx, const float* queries, int32_t n_queries, int32_t k, int32_t* out_idx, double* out_score,
               void* stream) {
  if (!ctx) return T2L_EINVAL;
  if (n_queries < 0 || k < 1 || k > T2L_MAX_TOPK)
    return fail(ctx, T2L_EINVAL, "t2l_search: need n_queries >= 0 and 1 <= k <= T2L_MAX_TOPK");
  if (n_queries == 0) return T2L_OK;
  if (!queries || !out_idx) return fail(ctx, T2L_EINVAL, "t2l_search: null buffer");
  if (ctx->db_pad == 0 && ctx->db_rows == 0 && !ctx->db) {
    // an empty shard is legal (ragged sharding); it answers -1 / -inf everywhere
  }
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return search_lanes_impl(ctx, queries, n_queries, k, out_idx, out_score, (hipStream_t)stream);
}

int t2l_search_many(t2l_ctx* ctx, const float* queries, int32_t n_batches, int32_t n_queries, int32_t k, int32_t* out_idx, double* out_score,
                    void* stream) {
  if (!ctx) return T2L_EINVAL;
  if (n_batches < 0 || n_queries < 0 || k < 1 || k > T2L_MAX_TOPK)
    return fail(ctx, T2L_EINVAL, "t2l_search_many: need n_batches >= 0, n_queries >= 0 and 1 <= k <= T2L_MAX_TOPK");
  if (n_batches == 0 || n_queries == 0) return T2L_OK;
  if (!queries || !out_idx) return fail(ctx, T2L_EINVAL, "t2l_search_many: null buffer");
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  for (int32_t b = 0; b < n_batches; ++b) {  // independent searches, enqueued back to back from C (no per-call binding cost)
    const size_t o = (size_t)b * n_queries;
    const int rc = search_lanes_impl(ctx, queries + o * kD, n_queries, k, out_idx + o * k, out_score ? out_score + o * k : nullptr,
                                     (hipStream_t)stream);
    if (rc != T2L_OK) return rc;
  }
  return T2L_OK;
}

int t2l_search_ordered(t2l_ctx* ctx, const float* queries, int32_t n_queries, int32_t k, int32_t* out_idx, double* out_score,
                       void* stream) {
  if (!ctx) return T2L_EINVAL;
  if (n_queries < 0 || k < 1 || k > T2L_MAX_TOPK)
    return fail(ctx, T2L_EINVAL, "t2l_search_ordered: need n_queries >= 0 and 1 <= k <= T2L_MAX_TOPK");
  if (n_queries == 0) return T2L_OK;
  if (!queries || !out_idx) return fail(ctx, T2L_EINVAL, "t2l_search_ordered: null buffer");
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  const int rc = search_join_impl(ctx, (hipStream_t)stream);  // anything still pipelined is ordered first
  return rc != T2L_OK ? rc : search_impl(ctx, queries, n_queries, k, out_idx, out_score, (hipStream_t)stream);
}

int t2l_search_join(t2l_ctx* ctx, void* stream) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return search_join_impl(ctx, (hipStream_t)stream);
}

int t2l_merge_topk(t2l_ctx* ctx, const int32_t* idx, const double* score, int32_t parts, int32_t n_queries, int32_t k,
                   int32_t* out_idx, double* out_score, void* stream) {
  if (!ctx) return T2L_EINVAL;
  if (parts < 1 || n_queries < 0 || k < 1 || k > T2L_MAX_TOPK)
    return fail(ctx, T2L_EINVAL, "t2l_merge_topk: bad parts / n_queries / k");
  if (n_queries == 0) return T2L_OK;
  if (!idx || !score || !out_idx) return fail(ctx, T2L_EINVAL, "t2l_merge_topk: null buffer");
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return merge_impl(ctx, idx, score, parts, n_queries, k, out_idx, out_score, (hipStream_t)stream);
}

int t2l_pack_pairs(t2l_ctx* ctx, const int32_t* idx, const double* score, int32_t n_queries, int32_t k, double* pairs,
                   void* stream) {
  if (!ctx) return T2L_EINVAL;
  if (n_queries < 0 || k < 1) return fail(ctx, T2L_EINVAL, "t2l_pack_pairs: bad n_queries / k");
  if (n_queries == 0) return T2L_OK;
  if (!idx || !score || !pairs) return fail(ctx, T2L_EINVAL, "t2l_pack_pairs: null buffer");
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return pack_impl(ctx, idx, score, n_queries * k, pairs, (hipStream_t)stream);
}

int t2l_merge_pairs(t2l_ctx* ctx, const double* pairs, int32_t parts, int32_t n_queries, int32_t k, int32_t* out_idx,
                    double* out_score, void* stream) {
  if (!ctx) return T2L_EINVAL;
  if (parts < 1 || n_queries < 0 || k < 1 || k > T2L_MAX_TOPK)
    return fail(ctx, T2L_EINVAL, "t2l_merge_pairs: bad parts / n_queries / k");
  if (n_queries == 0) return T2L_OK;
  if (!pairs || !out_idx) return fail(ctx, T2L_EINVAL, "t2l_merge_pairs: null buffer");
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return merge_pairs_impl(ctx, pairs, parts, n_queries, k, out_idx, out_score, (hipStream_t)stream);
}

int t2l_merge_gathered(t2l_ctx* ctx, const void* blocks, int64_t block_bytes, int64_t score_offset, int32_t parts, int32_t n_queries,
                       int32_t k, int32_t* out_idx, double* out_score, void* stream) {
  if (!ctx) return T2L_EINVAL;
  if (parts < 1 || n_queries < 0 || k < 1 || k > T2L_MAX_TOPK)
    return fail(ctx, T2L_EINVAL, "t2l_merge_gathered: bad parts / n_queries / k");
  if (n_queries == 0) return T2L_OK;
  if (!blocks || !out_idx) return fail(ctx, T2L_EINVAL, "t2l_merge_gathered: null buffer");
  if (reinterpret_cast<uintptr_t>(blocks) % 8)  // (int32 ids and float64 scores are read out of a byte buffer)
    return fail(ctx, T2L_EINVAL, "t2l_merge_gathered: blocks must start on an 8-byte boundary");
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return merge_gathered_impl(ctx, blocks, block_bytes, score_offset, parts, n_queries, k, out_idx, out_score, (hipStream_t)stream);
}

// counters of the last search of the context's own scratch set, or — with lanes — of the last search of EVERY lane, summed
static hipError_t read_counters(t2l_ctx* ctx, int32_t* out8) {
  if (ctx->last_search_small) {  // exact from the start: nothing failed a certificate, nothing fell back
    for (int i = 0; i < 8; ++i) out8[i] = 0;
    return hipSuccess;
  }
  hipError_t e = hipMemcpy(out8, ctx->fb_count, 8 * sizeof(int32_t), hipMemcpyDeviceToHost);
  if (e != hipSuccess || ctx->n_lanes <= 1) return e;
  for (int i = 0; i < 8; ++i) out8[i] = 0;
  for (int l = 0; l < ctx->n_lanes; ++l) {
    if (!ctx->lanes[l].ready) continue;
    int32_t c[8];
    if ((e = hipMemcpy(c, ctx->lanes[l].fb_count, sizeof(c), hipMemcpyDeviceToHost)) != hipSuccess) return e;
    for (int i = 0; i < 8; ++i) out8[i] += c[i];
  }
  return hipSuccess;
}

int t2l_search_fallbacks(t2l_ctx* ctx, int32_t* out_count) {
  if (!ctx || !out_count) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  T2L_HIP(ctx, hipDeviceSynchronize());
  int32_t c[8];
  T2L_HIP(ctx, read_counters(ctx, c));
  *out_count = c[kCntExactScan] + (c[kCntExactServed] - c[kCntExactUncert]);  // float64 VALU scans + queries the float64 MFMA stage certified (search_exact.hip)
  return T2L_OK;
}

#ifdef T2L_STAMPS
int t2l_debug_stamps(t2l_ctx* ctx, long long* out24) {  // dev builds only: s_memrealtime stamps a kernel left in fb_count[16..63]
  T2L_HIP(ctx, hipDeviceSynchronize());
  T2L_HIP(ctx, hipMemcpy(out24, ctx->fb_count + 16, 24 * sizeof(long long), hipMemcpyDeviceToHost));
  const long long init[8] = {0, 0, 0, 0, LLONG_MAX, 0, LLONG_MAX, 0};  // re-arm the min / max slots
  T2L_HIP(ctx, hipMemcpy(ctx->fb_count + 16, init, sizeof(init), hipMemcpyHostToDevice));
  return T2L_OK;
}
#endif

int t2l_search_counters(t2l_ctx* ctx, int32_t* out8) {
  if (!ctx || !out8) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  T2L_HIP(ctx, hipDeviceSynchronize());
  T2L_HIP(ctx, read_counters(ctx, out8));
  return T2L_OK;
}

int t2l_search_rescored(t2l_ctx* ctx, int32_t* out_count) {
  if (!ctx || !out_count) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  T2L_HIP(ctx, hipDeviceSynchronize());
  int32_t c[8];
  T2L_HIP(ctx, read_counters(ctx, c));
  *out_count = c[kCntRescored];
  return T2L_OK;
}

int t2l_contrastive_loss(t2l_ctx* ctx, const float* anchor, const float* positive, int32_t batch, float temperature,
                         float* loss, float* grad_anchor, float* grad_positive, void* stream) {
  if (!ctx) return T2L_EINVAL;
  if (batch < 1 || batch > T2L_MAX_LOSS_BATCH || !(temperature > 0.f))
    return fail(ctx, T2L_EINVAL, "t2l_contrastive_loss: need 1 <= batch <= 1024 and temperature > 0");
  if (!anchor || !positive || !loss) return fail(ctx, T2L_EINVAL, "t2l_contrastive_loss: null buffer");
  if ((grad_anchor == nullptr) != (grad_positive == nullptr))
    return fail(ctx, T2L_EINVAL, "t2l_contrastive_loss: pass both gradients or neither");
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return loss_impl(ctx, anchor, positive, batch, temperature, loss, grad_anchor, grad_positive, (hipStream_t)stream);
}

int t2l_ranking_loss(t2l_ctx* ctx, const float* im, const float* s, int32_t batch, int32_t kind, float margin, float scale,
                     float* out_loss, float* grad_im, float* grad_s, void* stream) {
  if (!ctx) return T2L_EINVAL;
  if (batch < 1 || batch > T2L_MAX_LOSS_BATCH) return fail(ctx, T2L_EINVAL, "t2l_ranking_loss: need 1 <= batch <= 1024");
  if (kind != T2L_RANK_PAIRWISE && kind != T2L_RANK_HARDEST)
    return fail(ctx, T2L_EINVAL, "t2l_ranking_loss: unknown kind (T2L_RANK_PAIRWISE or T2L_RANK_HARDEST)");
  if (!(margin >= 0.f) || !isfinite(margin)) return fail(ctx, T2L_EINVAL, "t2l_ranking_loss: margin must be finite and >= 0");
  if (!isfinite(scale)) return fail(ctx, T2L_EINVAL, "t2l_ranking_loss: scale must be finite");
  if (!im || !s || !out_loss) return fail(ctx, T2L_EINVAL, "t2l_ranking_loss: null buffer");
  if ((grad_im == nullptr) != (grad_s == nullptr)) return fail(ctx, T2L_EINVAL, "t2l_ranking_loss: pass both gradients or neither");
  // rows are read as float4 (sim_tiles_lds, sim_tile, cl_norm_kernel); everything else one float at a time
  if (((uintptr_t)im | (uintptr_t)s) % 16 != 0) return fail(ctx, T2L_EINVAL, "t2l_ranking_loss: im and s must be 16-byte aligned");
  if (((uintptr_t)out_loss | (uintptr_t)grad_im | (uintptr_t)grad_s) % 4 != 0)
    return fail(ctx, T2L_EINVAL, "t2l_ranking_loss: out_loss, grad_im and grad_s must be 4-byte aligned");
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return ranking_loss_impl(ctx, im, s, batch, kind, margin, scale, out_loss, grad_im, grad_s, (hipStream_t)stream);
}

int t2l_text_head_load_weights(t2l_ctx* ctx, const t2l_weight_desc* w, int32_t n, const char* prefix) {
  return t2l_text_head_load_weights_heads(ctx, w, n, prefix, 4);
}

int t2l_text_head_load_weights_heads(t2l_ctx* ctx, const t2l_weight_desc* w, int32_t n, const char* prefix, int32_t inter_num_heads) {
  if (!ctx) return T2L_EINVAL;
  if (!w || n <= 0) return fail(ctx, T2L_EINVAL, "t2l_text_head_load_weights: null/empty arguments");
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return text_head_load_impl(ctx, w, n, prefix, inter_num_heads);
}

int t2l_text_head(t2l_ctx* ctx, const float* hidden, int32_t n_sentences, int32_t n_tokens, float* out, int32_t* overflow, void* stream) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return text_head_impl(ctx, hidden, n_sentences, n_tokens, out, overflow, (hipStream_t)stream);
}

int t2l_text_train_bind(t2l_ctx* ctx, const t2l_train_tensor* tensors, int32_t n, const char* prefix) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return text_train_bind_impl(ctx, tensors, n, prefix);
}

int t2l_fine_train_bind(t2l_ctx* ctx, const t2l_train_tensor* tensors, int32_t n, const t2l_model_config* cfg) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return fine_train_bind_impl(ctx, tensors, n, cfg);
}

int t2l_fine_train_forward(t2l_ctx* ctx, const t2l_packed_cells* in, const float* pn_feat, const float* hint_desc, int32_t n_pairs,
                           int32_t n_hints, float dropout_p, uint32_t seed, float* out_offsets, void* stream) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return fine_train_forward_impl(ctx, in, pn_feat, hint_desc, n_pairs, n_hints, dropout_p, seed, out_offsets, (hipStream_t)stream);
}

int t2l_fine_train_forward_points(t2l_ctx* ctx, const t2l_packed_cells* in, const float* pos, const float* rgb, const float* hint_desc,
                                  int32_t n_pairs, int32_t n_hints, float dropout_p, uint32_t seed, float* out_offsets, void* stream) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return fine_train_forward_points_impl(ctx, in, pos, rgb, hint_desc, n_pairs, n_hints, dropout_p, seed, out_offsets, (hipStream_t)stream);
}

int t2l_fine_train_backward(t2l_ctx* ctx, const float* grad_offsets, float* grad_hint_desc, float* grad_pn_feat, void* stream) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return fine_train_backward_impl(ctx, grad_offsets, grad_hint_desc, grad_pn_feat, (hipStream_t)stream);
}

int t2l_fine_adam_step(t2l_ctx* ctx, float lr, float beta1, float beta2, float eps, void* stream) {
  if (!ctx) return T2L_EINVAL;
  if (!(lr >= 0.f) || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(eps >= 0.f))
    return fail(ctx, T2L_EINVAL, "t2l_fine_adam_step: need lr >= 0, 0 <= beta < 1, eps >= 0");
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return fine_adam_step_impl(ctx, lr, beta1, beta2, eps, (hipStream_t)stream);
}

int t2l_fine_zero_grad(t2l_ctx* ctx, void* stream) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return fine_zero_grad_impl(ctx, (hipStream_t)stream);
}

int t2l_fine_adam_state(t2l_ctx* ctx, int32_t set, float* m, float* v, int64_t* step, int64_t* numel, void* stream) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return fine_adam_state_impl(ctx, set, m, v, step, numel, (hipStream_t)stream);
}

int t2l_text_head_train(t2l_ctx* ctx, const float* hidden, int32_t n_sentences, int32_t n_tokens, int32_t n_descriptions, float dropout_p,
                        uint32_t seed, float* out, void* stream) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return text_train_forward_impl(ctx, hidden, n_sentences, n_tokens, n_descriptions, dropout_p, seed, out, (hipStream_t)stream);
}

int t2l_text_head_backward(t2l_ctx* ctx, const float* grad_out, void* stream) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return text_train_backward_impl(ctx, grad_out, (hipStream_t)stream);
}

int t2l_text_adam_step(t2l_ctx* ctx, float lr, float beta1, float beta2, float eps, void* stream) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return text_adam_step_impl(ctx, lr, beta1, beta2, eps, (hipStream_t)stream);
}

int t2l_text_zero_grad(t2l_ctx* ctx, void* stream) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return text_zero_grad_impl(ctx, (hipStream_t)stream);
}

int t2l_text_adam_state(t2l_ctx* ctx, int32_t set, float* m, float* v, int64_t* step, int64_t* numel, void* stream) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return text_adam_state_impl(ctx, set, m, v, step, numel, (hipStream_t)stream);
}

int64_t t2l_train_sync_bn_doubles(void) { return train_sync_bn_doubles(); }

int t2l_train_sync_bn(t2l_ctx* ctx, double* buf, int64_t n_doubles, t2l_allreduce_fn fn, void* user) {
  if (!ctx) return T2L_EINVAL;
  if (fn && (!buf || n_doubles < train_sync_bn_doubles()))
    return fail(ctx, T2L_EINVAL, "t2l_train_sync_bn: buf must hold t2l_train_sync_bn_doubles() float64 values");
  ctx->sync_fn = fn;
  ctx->sync_user = fn ? user : nullptr;
  ctx->sync_buf = fn ? buf : nullptr;
  ctx->sync_failed = false;
  train_sync_changed(ctx);
  return T2L_OK;
}

int t2l_text_inter(t2l_ctx* ctx, const float* sent, int32_t n_descriptions, int32_t n_sentences_per, float* out, int32_t* overflow, void* stream) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return text_inter_impl(ctx, sent, n_descriptions, n_sentences_per, out, overflow, (hipStream_t)stream);
}

int t2l_fine_load_weights(t2l_ctx* ctx, const t2l_weight_desc* w, int32_t n, const t2l_model_config* cfg) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  if (!w || n <= 0 || !cfg) return fail(ctx, T2L_EINVAL, "t2l_fine_load_weights: null argument");
  // the fine checkpoint carries its own object_encoder.pointnet.* (optional group)
  return load_with_backbone(ctx, "t2l_fine_load_weights", w, n, [&] { return fine_load_impl(ctx, w, n, cfg); });
}

int t2l_fine_encode_objects(t2l_ctx* ctx, const t2l_packed_cells* in, float* out_desc, void* stream) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return fine_encode_impl(ctx, in, out_desc, (hipStream_t)stream);
}

int t2l_fine_match(t2l_ctx* ctx, const float* cell_desc, const int32_t* cell_index, const float* hint_desc,
                   const int32_t* hint_index, int32_t n_pairs, int32_t n_hints, float* out_offsets, void* stream) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return fine_match_impl(ctx, cell_desc, cell_index, hint_desc, hint_index, n_pairs, n_hints, out_offsets, (hipStream_t)stream);
}

int t2l_train_bind(t2l_ctx* ctx, const t2l_train_tensor* tensors, int32_t n, const t2l_model_config* cfg) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return train_bind_impl(ctx, tensors, n, cfg);
}

int t2l_encode_cells_train(t2l_ctx* ctx, const t2l_packed_cells* in, float dropout_p, uint32_t seed, float* out_emb,
                           void* stream) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return train_forward_impl(ctx, in, dropout_p, seed, out_emb, (hipStream_t)stream);
}

int t2l_encode_cells_backward(t2l_ctx* ctx, const float* grad_emb, float* grad_pn_feat, void* stream) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return train_backward_impl(ctx, grad_emb, grad_pn_feat, (hipStream_t)stream);
}

int t2l_pointnet_features_train(t2l_ctx* ctx, const float* pos, const float* rgb, const int32_t* cell_offsets, int32_t n_cells,
                                float* out_features2, void* stream) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return pn_train_forward_impl(ctx, pos, rgb, cell_offsets, n_cells, out_features2, (hipStream_t)stream);
}

int t2l_pointnet_backward(t2l_ctx* ctx, const float* grad_features2, void* stream) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return pn_train_backward_impl(ctx, grad_features2, (hipStream_t)stream);
}

int t2l_pointnet_load_weights(t2l_ctx* ctx, const t2l_weight_desc* w, int32_t n) {
  if (!ctx) return T2L_EINVAL;
  if (!w || n <= 0) return fail(ctx, T2L_EINVAL, "t2l_pointnet_load_weights: null/empty arguments");
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  PointNetStaged* pn = nullptr;
  if (int rc = pointnet_stage(ctx, "t2l_pointnet_load_weights", w, n, &pn)) return rc;
  if (!pn) return fail(ctx, T2L_EINVAL, "t2l_pointnet_load_weights: the list holds no object_encoder.pointnet.* tensor");
  return pointnet_commit(ctx, "t2l_pointnet_load_weights", pn);
}

int t2l_pointnet_cls_bind(t2l_ctx* ctx, const t2l_train_tensor* tensors, int32_t n) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return cls_bind_impl(ctx, tensors, n);
}

int t2l_pointnet_cls_forward(t2l_ctx* ctx, const float* pos, const float* rgb, int32_t n_objects, float* out_features2, void* stream) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return cls_forward_impl(ctx, pos, rgb, n_objects, out_features2, (hipStream_t)stream);
}

int t2l_pointnet_cls_heads(t2l_ctx* ctx, const float* features2, int32_t n, const int32_t* class_labels, const int32_t* color_labels,
                           float w_class, float w_color, float* out_logits, float* out_loss, int32_t* out_correct, float* grad_features2,
                           void* stream) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return cls_heads_impl(ctx, features2, n, class_labels, color_labels, w_class, w_color, out_logits, out_loss, out_correct, grad_features2,
                        (hipStream_t)stream);
}

int t2l_pointnet_cls_backward(t2l_ctx* ctx, const float* grad_features2, void* stream) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return cls_backward_impl(ctx, grad_features2, (hipStream_t)stream);
}

int t2l_zero_grad(t2l_ctx* ctx, void* stream) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return zero_grad_impl(ctx, (hipStream_t)stream);
}

int t2l_adam_step(t2l_ctx* ctx, float lr, float beta1, float beta2, float eps, void* stream) {
  if (!ctx) return T2L_EINVAL;
  if (!(lr >= 0.f) || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(eps >= 0.f))
    return fail(ctx, T2L_EINVAL, "t2l_adam_step: need lr >= 0, 0 <= beta < 1, eps >= 0");
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return adam_step_impl(ctx, lr, beta1, beta2, eps, (hipStream_t)stream);
}

int t2l_adam_state(t2l_ctx* ctx, int32_t set, float* m, float* v, int64_t* step, int64_t* numel, void* stream) {
  if (!ctx) return T2L_EINVAL;
  T2L_HIP(ctx, hipSetDevice(ctx->device));
  return adam_state_impl(ctx, set, m, v, step, numel, (hipStream_t)stream);
}

int t2l_set_option(t2l_ctx* ctx, const char* name, double value) {
  if (!ctx || !name) return T2L_EINVAL;
  if (!strcmp(name, "certify_eps_scale")) {
    if (!(value >= 0)) return fail(ctx, T2L_EINVAL, "certify_eps_scale must be >= 0");
    ctx->knobs.eps_scale = value;
  } else if (!strcmp(name, "search_nsplit")) {
    if (value < 0 || value > kMaxParts / 2) return fail(ctx, T2L_EINVAL, "search_nsplit out of range [0,32]");
    ctx->knobs.nsplit_override = (int)value;
  } else if (!strcmp(name, "search_mode")) {
    if (value != 0 && value != 2)
      return fail(ctx, T2L_EINVAL, "search_mode must be 0 (f16 scan) or 2 (split-bf16 scan); 1 (the exact-f32 MFMA scan: 7x slower, same results) was removed in round 5");
    ctx->knobs.search_mode = (int)value;
  } else if (!strcmp(name, "encoder_f32")) {
    ctx->encoder_f32 = value != 0;
  } else if (!strcmp(name, "encoder_f16")) {
    ctx->encoder_f16 = value != 0;
  } else if (!strcmp(name, "text_head_rows")) {
    if (value < 0 || value > (1 << 18)) return fail(ctx, T2L_EINVAL, "text_head_rows: 0 (default) .. 262144");
    ctx->text_head_rows = (int)value;
  } else if (!strcmp(name, "search_auto")) {
    ctx->search_auto = value != 0;
    if (!ctx->search_auto) ctx->policy.reset(false);  // forget the state and every report of a search launched so far
  } else if (!strcmp(name, "search_heavy")) {  // force (1) / release (0) the float64 MFMA exact stage (tests)
    ctx->policy.heavy = value != 0;
  } else if (!strcmp(name, "search_small")) {
    ctx->search_small = value != 0;
  } else if (!strcmp(name, "search_small_wgs")) {
    if (value < 0 || value > 256) return fail(ctx, T2L_EINVAL, "search_small_wgs: 0 (default by query count: 128 or 192) .. 256 workgroups per slice");
    ctx->search_small_wgs = (int)value;
  } else if (!strcmp(name, "search_xcd_qgroups")) {
    if (value != 1 && value != 2 && value != 4 && value != 8) return fail(ctx, T2L_EINVAL, "search_xcd_qgroups must be 1, 2, 4 or 8");
    ctx->knobs.xcd_qgroups = (int)value;
  } else if (!strcmp(name, "text_train_bf16")) {
    // (0 = f32 MFMA operands was an option until round 5: 7.6 ms per step against 5.6 ms for PyTorch on the same GPU — a trap, removed.
    // Split-bf16 is the f32-class arithmetic of the head: relative product error <= 2^-16 + 2^-18, meets the f32 goldens to 1e-4.)
    if (value != 1 && value != 2)
      return fail(ctx, T2L_EINVAL, "text_train_bf16: 2 (default: split-bf16, the f32-class arithmetic) or 1 (bf16 operands); the f32-MFMA "
                                   "form (0) was removed in round 5 — it measured slower than PyTorch's f32 step");
    ctx->text_train_bf16 = (int)value;
  } else if (!strcmp(name, "encoder_two_cells")) {
    ctx->encoder_two_cells = value != 0;
  } else if (!strcmp(name, "search_merge_lists")) {
    if (value != 0 && value != 1 && value != 2) return fail(ctx, T2L_EINVAL, "search_merge_lists: 0 (plain lists), 1 (merged records), 2 (default: by report card)");
    ctx->knobs.search_merge = (int)value;
    ctx->policy.merge_live = true;
  } else if (!strcmp(name, "search_wide_repair")) {
    if (value < 0 || value > 1024) return fail(ctx, T2L_EINVAL, "search_wide_repair: 0 (off) .. 1024 rows");
    ctx->knobs.wide_repair = (int)value;
  } else if (!strcmp(name, "search_tile_sel")) {
    ctx->knobs.search_tile_sel = value != 0;
  } else if (!strcmp(name, "search_epilogue")) {
    if (value != 0 && value != 1) return fail(ctx, T2L_EINVAL, "search_epilogue: 0 (round 6's epilogue and record layout) or 1 (default)");
    ctx->knobs.search_epilogue = (int)value;
  } else if (!strcmp(name, "search_rerank_form")) {
#ifdef T2L_RERANK_PARTS  // dev build: 2 = the row-local merge alone, 3 = the one round trip alone
    if (value == 2 || value == 3) {
      ctx->knobs.rerank_form = (int)value;
      return T2L_OK;
    }
#endif
    if (value != 0 && value != 1) return fail(ctx, T2L_EINVAL, "search_rerank_form: 0 (round 7's re-rank of merged records) or 1 (default: row-local merge, one gather round trip)");
    ctx->knobs.rerank_form = (int)value;
  } else if (!strcmp(name, "search_pair_ll")) {
    if (value != 5 && value != 6) return fail(ctx, T2L_EINVAL, "search_pair_ll must be 5 or 6");
    ctx->knobs.pair_ll = (int)value;
  } else if (!strcmp(name, "train_gemm_block")) {
    if (value != 0 && value != 32 && value != 64) return fail(ctx, T2L_EINVAL, "train_gemm_block must be 0 (auto), 32 or 64");
    ctx->train_gemm_block = (int)value;
  } else if (!strcmp(name, "train_bf16")) {
    if (value != 0 && value != 1 && value != 2) return fail(ctx, T2L_EINVAL, "train_bf16: 0 (f32 MFMA), 1 (bf16 operands) or 2 (split-bf16, three products)");
    ctx->train_bf16 = (int)value;
  } else if (!strcmp(name, "train_keep_adam_state")) {
    ctx->train_keep_adam = value != 0;
  } else if (!strcmp(name, "profile_rerank")) {
    ctx->knobs.profile_rerank = value != 0;
  } else if (!strcmp(name, "stats_reset")) {  // forget every kernel-time sample so far (host-only: no stream operation, no sync)
    for (auto& kv : ctx->events) {
      kv.second.count = 0;
      kv.second.calls = 0;
      kv.second.open = false;
    }
    ctx->span_read = ctx->busy_read = ctx->span_seq;
  } else if (!strcmp(name, "search_lanes")) {
    if (value < 1 || value > t2l_ctx::kMaxLanes) return fail(ctx, T2L_EINVAL, "search_lanes must be 1..4");
    T2L_HIP(ctx, hipDeviceSynchronize());
    for (auto& L : ctx->lanes) L.pending = false;
    ctx->n_lanes = (int)value;
  } else if (!strcmp(name, "stream_min_rows")) {
    ctx->stream_min_rows = (int)value;
  } else if (!strcmp(name, "pointnet_pyg_self_loops")) {
    ctx->pn_self_loops = value != 0;
  } else if (!strcmp(name, "profile_events")) {
    if (value < 0) return fail(ctx, T2L_EINVAL, "profile_events must be >= 0");
    ctx->profile_events = (int)value;
    for (auto& kv : ctx->events) kv.second.calls = 0;  // the next launch of every kernel is a bracketed one
  } else {
    return fail(ctx, T2L_EINVAL, std::string("unknown option: ") + name);
  }
  return T2L_OK;
}

int t2l_kernel_stats(t2l_ctx* ctx, const char* name, float* out_avg_ms, int32_t* out_count) {
  if (!ctx || !name || !out_avg_ms || !out_count) return T2L_EINVAL;
  *out_avg_ms = 0.f;
  *out_count = 0;
  const bool busy = !strcmp(name, "search_scan_busy");
  if (busy || !strcmp(name, "search_scan_span")) {
    // in-kernel stamps of the paired scan. span: first workgroup start -> last workgroup end of a launch; busy: the sum of its
    // workgroups' own durations / grid = the GPU time it used (equal to the span when it has the chip to itself, the one
    // that still means something when launches of several lanes overlap). Each name keeps its own read cursor.
    unsigned& cursor = busy ? ctx->busy_read : ctx->span_read;
    if (!ctx->scan_span || ctx->span_seq == cursor) return T2L_OK;
    T2L_HIP(ctx, hipDeviceSynchronize());
    std::vector<unsigned long long> h((size_t)2 * kSpanWgs * kSpanRing);
    T2L_HIP(ctx, hipMemcpy(h.data(), ctx->scan_span, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost));
    const unsigned first = ctx->span_seq - cursor > (unsigned)kSpanRing ? ctx->span_seq - kSpanRing + 1 : cursor + 1;
    double sum = 0.0;
    int n = 0;
    const unsigned long long tmask = (1ull << 40) - 1;
    for (unsigned q = first; q <= ctx->span_seq; ++q) {
      const unsigned long long* e = &h[(size_t)2 * kSpanWgs * (q % kSpanRing)];
      const unsigned grid = ctx->span_grid[q % kSpanRing];
      if (!grid) continue;
      unsigned long long t_min = ~0ull, t_max = 0, total = 0;
      bool ok = true;
      for (unsigned w = 0; w < grid && ok; ++w) {
        const unsigned long long a = e[2 * w], b = e[2 * w + 1];
        ok = (a >> 40) == (q & 0xFFFFFFu) && (b >> 40) == (q & 0xFFFFFFu);  // else: slot overwritten or launch not finished
        t_min = std::min(t_min, a & tmask);
        t_max = std::max(t_max, b & tmask);
        total += ((b & tmask) - (a & tmask)) & tmask;
      }
      if (!ok) continue;
      sum += (busy ? (double)total / grid : (double)((t_max - t_min) & tmask)) * 1e-5;  // 100 MHz ticks -> ms
      ++n;
    }
    cursor = ctx->span_seq;
    if (n) *out_avg_ms = (float)(sum / n);
    *out_count = n;
    return T2L_OK;
  }
  auto it = ctx->events.find(name);
  if (it == ctx->events.end() || it->second.count == 0) return T2L_OK;
  EventRing& e = it->second;
  double sum = 0.0;
  for (int i = 0; i < e.count; ++i) {
    const int slot = ((e.head - 1 - i) % kEventRing + kEventRing) % kEventRing;
    T2L_HIP(ctx, hipEventSynchronize(e.b[slot]));
    float ms = 0.f;
    T2L_HIP(ctx, hipEventElapsedTime(&ms, e.a[slot], e.b[slot]));
    sum += ms;
  }
  *out_avg_ms = (float)(sum / e.count);
  *out_count = e.count;
  e.count = 0;
  return T2L_OK;
}

}  // extern "C"

