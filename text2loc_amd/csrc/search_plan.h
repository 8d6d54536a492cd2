// The host side of a batched search, as plain C++ (no HIP, no t2l_ctx, no allocation): which kernels a (Q, k, rows, options) call
// launches and with what (plan_segment), and the report-card state machine that picks the mode of the next call (SearchPolicy).
// search.hip launches what the plan says; tests/search_plan_check.cpp drives both without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace t2l {

// ---- search geometry -------------------------------------------------------------------------
constexpr int kScanDim = 256;                      // = kD (t2l_internal.h asserts it)
constexpr int kTileRows = 32;                      // DB rows per LDS tile (one 32x32 MFMA row block)
constexpr int kRowStrideF = kScanDim + 4;          // LDS row stride in floats (1040 B): ds_read_b128 conflict-free
constexpr int kTileFloats = kTileRows * kRowStrideF;
constexpr int kHalfTileBytes = kTileRows * 512;    // 32 rows x 256 f16 = 16 KiB, tile-chunk-major (search_dev.h)
constexpr int kMaxParts = 64;                      // per-query candidate partitions (= 2 * nsplit) the re-rank merges
constexpr int kMaxPerTiles = 512;                  // tiles per split of one scan launch (13 key code bits)
constexpr int kSegmentRows = (kMaxParts / 2) * kMaxPerTiles * 32;  // rows one scan launch covers (524,288); also the unit inside which the f16 plane deals rows to tiles strided
constexpr int kWideQPerWave = 64;
constexpr int kWideQPerBlock = 4 * kWideQPerWave;  // queries per scan workgroup (scanw / scanh / scanp)
constexpr int kMergedLL = 8;                       // floats of a merged record (search.hip: MERGE)
constexpr int kWideCap = 1024;                     // rows one wave re-scores in a WIDE repair (rerank_kernel) before the query is handed to an exact scan of the whole shard

// The options a plan reads (t2l_set_option names in brackets).
struct SearchKnobs {
  double eps_scale = 1.0;   // [certify_eps_scale]
  int nsplit_override = 0;  // [search_nsplit]
  int search_mode = 0;      // [search_mode] 0 = f16 MFMA scan (default), 2 = split-bf16 MFMA scan
  // mode 0 watches how many queries of a batch its certificate sends to the second stage (the re-rank writes the
  // count to mapped host memory; no stream operation, no synchronisation) and, when that is more than one in eight —
  // scores packed tighter than the f16 error band — searches with the split-bf16 scan (50x tighter bound) until fewer than
  // one in sixteen would be flagged again (SearchPolicy below)
  int pair_ll = 6;          // [search_pair_ll] per-lane list length of the paired scan (5 or 6)
  int search_epilogue = 1;  // [search_epilogue] paired scan: 1 = the short epilogue + records laid out by XCD (scanp_kernel<..., SEL = 1>, record_slot), 0 = round 6's (SEL = 2)
  int search_tile_sel = 1;  // [search_tile_sel] paired scan with the tile-local top-3 selection (scanp_kernel<..., SEL = 1>; merged records only)
  int wide_repair = 512;    // [search_wide_repair] rows a re-rank wave may re-score in a wide repair before the query goes to an exact scan (0: never)
  int search_merge = 2;     // [search_merge_lists] the paired scan merges a workgroup's four lists per query into one 32-byte record (search.hip: MERGE / MG):
                            // 0 never, 1 always, 2 while the f16 report cards show next to no failed first certificates (a repair behind
                            // a merged record re-scores 4x the rows of a plain list's)
  int xcd_qgroups = 4;      // [search_xcd_qgroups] paired scan: query-block groups per XCD rectangle (1 = every XCD sees all queries and 1/8 of the splits;
                            // 4 = a quarter of the queries and half of the splits: -1.3 us of scan span at Q = 4096 x N = 11,259, measured)
  int profile_rerank = 1;   // [profile_rerank] 0: sampled launches bracket the scan only (an event pair costs the stream ~6 us per kernel)
  int rerank_form = 1;      // [search_rerank_form] re-rank of merged records of the tile-local selection: 1 = the merge reduces over the 16-lane row that holds
                            // the records and all twelve early row fetches are issued before the first wait (rerank_kernel<..., FORM = 1>), 0 = round 7's form
};

// ---- the report card ---------------------------------------------------------------------------
// Fields of the mapped host int32[8] a call's re-rank publishes about the call BEFORE it (search.hip: publish_report).
enum ReportField {
  kStatSeq = 0,       // sequence number of the call that published (written last, release; read first, acquire)
  kStatFlagged = 1,   // f16-certificate failures the wave could not settle (or the probe's count of what the f16 band would flag)
  kStatTotal = 2,     // Q of the reported call (0: a call that keeps no report card)
  kStatExact = 3,     // queries that ended in an exact stage
  kStatMode = 4,      // 0: not an f16-certificate count, 1: the f16 scan's own, 2: the split-bf16 stand-in's probe
  kStatRescored = 5,  // first-certificate failures (settled in the wave or not)
  kStatInts = 8,
};

// What the report cards of earlier calls on this database say about the next one. One per context; the lanes of pipelined
// searches share it except for `stat_seen`, which travels with a lane's own report card (search.hip: swap_lane).
struct SearchPolicy {
  bool escalated = false;   // the split-bf16 scan is standing in (it counts what the f16 band would still flag)
  bool heavy = false;       // the database defeats the certificates: flagged queries go to the float64 MFMA stage
  bool all_exact = false;   // ... and nearly all of them: EVERY query goes there, no candidate scan (search_impl)
  bool merge_live = true;   // (search_merge == 2) what the report cards say right now
  unsigned all_exact_calls = 0;
  int stat_seq = 0, stat_seen = 0;  // sequence number of the last call launched / of the last report read

  // Forget the state and every report of a search launched so far. keep_in_flight_report = false: exactly that (option
  // "search_auto" = 0). true (a new database): the NEXT call's re-rank still publishes the report of the last call on the old
  // rows, so that one is void as well.
  void reset(bool keep_in_flight_report) {
    escalated = false;
    heavy = false;
    all_exact = false;
    merge_live = true;
    stat_seen = keep_in_flight_report ? stat_seq + 1 : stat_seq;
  }

  // The prior of t2l_db_set (capi.hip): a sample's mean pairwise cosine above 0.9 starts on the split-bf16 stand-in with the
  // unsettled queries deferred to the float64 MFMA stage.
  void seed_from_prior(double mean_cos) {
    if (mean_cos > 0.9) {  // (NaN compares false)
      escalated = true;
      heavy = true;
    }
  }

  // the f16 scan's report card of an earlier call on this DB: more than 1 in 8 queries flagged ->
  // the split-bf16 scan from now on
  // ... and back when fewer than 1 in 16 would be (the stand-in counts them, rerank_kernel)
  // ... and its exact-stage count: when more than 1 in 64 queries of a call ended in the float64 scan, the database
  // defeats the certificates wholesale ("heavy"): later calls defer those queries to the float64 MFMA stage
  // (search_exact.hip) instead of the fallback kernel's VALU scan, until fewer than 1 in 256 need it
  void observe(const int32_t report[kStatInts], int search_mode, bool search_auto) {
    const int done = report[kStatSeq];
    if (done > stat_seen) {
      stat_seen = done;
      const int64_t flagged = report[kStatFlagged], total = report[kStatTotal], exact_prev = report[kStatExact],
                    rescored = report[kStatRescored];
      const int stat = report[kStatMode];
      // (total == 0: the bank of a call that keeps no report card — the streaming scan clears its bank and counts its exact scans
      // only — or of no call at all: nothing to learn from)
      const bool counted = total > 0;
      if (counted && search_mode == 0 && search_auto && stat) {
        // ... or more than 1 in 2 failed the first certificate: the in-wave repairs settle them, but a wide repair re-scores
        // dozens to hundreds of rows per query — measured on a clustered database with 92 % of the queries repaired: 185 us per
        // step on the f16 scan against 133 us on the split-bf16 scan, whose 50x tighter band certifies them outright
        // (a report is two calls old: only a report of the f16 scan escalates, only one of the stand-in's probe releases —
        // an f16 report that arrives after the switch must not undo it)
        if (stat == 1 && !escalated && (flagged * 8 > total || rescored * 2 > total)) escalated = true;
        else if (stat == 2 && escalated && flagged * 16 < total) escalated = false;
      }
      // merged candidate records pay while repairs are rare: more than 1 query in 64 failing its first certificate -> plain lists
      // (their repairs re-score a quarter of the rows), back below 1 in 256
      if (counted && stat == 1) {
        if (merge_live && rescored * 64 > total) merge_live = false;
        else if (!merge_live && rescored * 256 <= total) merge_live = true;
      }
      if (counted && search_auto) {
        if (!heavy && exact_prev * 64 > total) heavy = true;
        else if (heavy && exact_prev * 256 < total) heavy = false;
        // 7 in 8 queries end in the exact stage whatever the candidate scan says: stop paying for the scan and the re-rank
        // (0.26 ms of a 1.0 ms step on such a database) and hand EVERY query to the float64 MFMA stage; one call in 8 still
        // takes the long way and its report decides whether that remains true
        // (only on the word of the split-bf16 stand-in, whose band is the tightest a candidate scan has: a database that defeats
        // the f16 scan alone gets the stand-in first; reports of all-exact calls themselves carry no scan and change nothing)
        if (stat == 2) all_exact = heavy && exact_prev * 8 >= total * 7;
        else if (stat == 1) all_exact = false;
      }
    }
  }

  // the scan this call runs
  int eff_mode(int search_mode) const { return (search_mode == 0 && escalated) ? 2 : search_mode; }

  // All-exact mode skips the scan and the re-rank of a single-segment shard seven calls in eight. (`all_exact` is only ever set
  // by observe() with search_auto on, and turning search_auto off resets it: no separate test of the option here.)
  bool take_all_exact(int n_seg) { return heavy && all_exact && n_seg == 1 && (all_exact_calls++ & 7) != 7; }
};

// ---- the launch plan ---------------------------------------------------------------------------
// Segments of a shard (one scan launch covers kSegmentRows rows); too_large: more than 256 / K of them (search_merge.hip's limit).
struct Segments {
  int n_seg;
  bool too_large;
};
inline Segments segments_of(int n_rows, int K) {
  int n_seg = (n_rows + kSegmentRows - 1) / kSegmentRows;
  if (n_seg < 1) n_seg = 1;
  return {n_seg, n_seg * K > 256};
}

enum class ScanKernel {
  kWaveF16,       // scanh_kernel<LL>: one wave per SIMD, f16 operands
  kWaveBf16,      // scanw_kernel<LL, 4>: one wave per SIMD, split-bf16 operands
  kPair5,         // scanp_kernel<5, 4>: paired, plain lists
  kPair6,         // scanp_kernel<6, 4>
  kPairMerged0,   // scanp_kernel<6, 4, true, 0>: merged records, per-score insertion
  kPairMerged1,   // scanp_kernel<6, 4, true, 1>: ... tile-local selection, short epilogue (the default)
  kPairMerged2,   // scanp_kernel<6, 4, true, 2>: ... tile-local selection, round 6's epilogue
};
enum class RerankKernel {
  kLists5,   // rerank_kernel<5, 16>
  kLists6,   // rerank_kernel<6, 16>
  kLists8,   // rerank_kernel<8, 16>
  kLists16,  // rerank_kernel<16, 16>
  kLists32,  // rerank_kernel<32, 32>
  kRecords,  // rerank_kernel<kMergedLL, 16, true>
};

// Everything between "rows of this segment" and "launch". LL = per-lane list length the scan keeps, L = rows the re-rank
// re-scores per query.
struct SegmentPlan {
  int L, n_tiles, nsplit, per, code_bits, LL;
  bool pair;          // the paired scan: `nsplit` counts VIRTUAL splits then, the kernel takes physical ones (scan_nsplit)
  size_t cand_bytes;  // candidate workspace
  ScanKernel scan;
  unsigned grid, block;
  size_t lds;
  int scan_nsplit;    // the scan kernel's `nsplit` argument
  int xq, slot_bits;  // paired scan: XCD rectangle, record layout (record_slot)
  bool merged;        // the candidate lists are merged records (scanp_kernel<..., MERGE>)
  float eps_rel, eps_probe;
  int half_mode, stat_mode, defer;
  RerankKernel rerank;
  int rerank_parts, rec6, rerank_slot_bits, wide_cap;
  bool time_rerank;   // sampled launches bracket the re-rank too
  int rerank_form;    // kRecords: rerank_kernel<kMergedLL, 16, true, rerank_form> (1 needs the six-key records of the tile-local selection: rec6)
};

inline SegmentPlan plan_segment(const SearchKnobs& k, int eff_mode, bool merge_live, bool heavy, int Q, int K, int rows) {
  SegmentPlan p{};
  const int qpb = kWideQPerBlock;
  const int n_qblocks = (Q + qpb - 1) / qpb;
  // rows re-scored per query: K + margin (the margin only has to absorb key-truncation ties; the certificate catches
  // the rest). (L = 12 was measured: second-stage re-scores multiply.)
  const int L = (K <= 10) ? 16 : 32;
  const int n_tiles = ((rows > 0 ? rows : 0) + kTileRows - 1) / kTileRows;
  auto imax = [](int a, int b) { return a > b ? a : b; };
  auto imin = [](int a, int b) { return a < b ? a : b; };
  // the paired scan (two waves per SIMD, scanp_kernel) serves the f16 mode whenever the shard gives every query at least
  // 32 per-lane lists (>= 8 physical splits: 256+ rows); its splits below are VIRTUAL ones (two per workgroup)
  // (small batches keep the one-wave-per-SIMD kernel: twice the workgroups, and its prologue is the shorter one)
  const bool pair_ok = eff_mode == 0 && L == 16 && n_tiles >= 16 && Q >= 256;
  int nsplit = k.nsplit_override;
  if (nsplit <= 0) {
    // fill 256 CUs with one (wide scan) or two workgroups each; multiples of 8 keep a split on one XCD's L2
    nsplit = (256 + n_qblocks - 1) / n_qblocks;
    nsplit = ((nsplit + 7) / 8) * 8;
  }
  nsplit = imax(1, imin(nsplit, kMaxParts / 2));
  nsplit = imax(1, imin(nsplit, imax(1, n_tiles)));
  nsplit = imax(nsplit, (n_tiles + kMaxPerTiles - 1) / kMaxPerTiles);  // keep the key code within 13 bits
  bool pair = pair_ok;
  if (pair) {  // physical splits = workgroups per query block (<= 16), virtual = twice that
    int phys = k.nsplit_override > 0 ? imax(1, k.nsplit_override / 2) : imin(16, nsplit);
    phys = imax(phys, (n_tiles + 2 * kMaxPerTiles - 1) / (2 * kMaxPerTiles));
    phys = imin(phys, 16);
    if (2 * phys > n_tiles || 4 * phys < 32) pair = false;
    else nsplit = 2 * phys;
  }
  const int per = imax(1, (n_tiles + nsplit - 1) / nsplit);
  int code_bits = 4;
  while ((1 << code_bits) < per * 16) ++code_bits;
  // per-lane list length of the wide scan: the global top-L spreads over 2*nsplit lists (tiles are dealt round-robin
  // to the splits, 4-row groups alternate between the lane halves), so 8 per list hold it unless more than 8 of a
  // query's best 16 fall into ONE list — with >= 16 lists a ~1e-8 event on unstructured data; the certificate
  // (floors of full lists) catches it and the fallback re-scores. Few lists (tiny shards): keep 16.
  const int LL = pair ? k.pair_ll : (L == 32 ? 32 : (2 * nsplit >= 16 ? 8 : 16));
  p.L = L;
  p.n_tiles = n_tiles;
  p.nsplit = nsplit;
  p.pair = pair;
  p.per = per;
  p.code_bits = code_bits;
  p.LL = LL;
  p.cand_bytes = (size_t)n_qblocks * qpb * 2 * nsplit * LL * sizeof(float);

  p.half_mode = eff_mode == 0;
  const bool probing = k.search_mode == 0 && eff_mode == 2;  // standing in for the f16 scan (SearchPolicy)
  // f32 dot-product error bound: gamma_n * |a||b| with n = 256 terms (+ slack for the MFMA's k order), plus the operand
  // rounding of the scan that produced the keys: f16 (RNE, both operands) 2^-10 + 2^-21 and 2^-20 for denormal
  // elements, rounded up to 9.85e-4; split-bf16 2^-16 + 2^-18, rounded up to 2e-5; f32: none
  const double operand_eps = eff_mode == 0 ? 9.85e-4 : (eff_mode == 2 ? 2.0e-5 : 0.0);
  p.eps_rel = (float)(k.eps_scale * ((kScanDim + 8) * 5.9604644775390625e-08 + operand_eps));
  p.eps_probe = probing ? (float)(k.eps_scale * ((kScanDim + 8) * 5.9604644775390625e-08 + 9.85e-4)) : 0.f;
  p.stat_mode = probing ? 2 : (p.half_mode ? 1 : 0);
  p.defer = heavy ? 1 : 0;
  p.wide_cap = imin(k.wide_repair, kWideCap);
  p.time_rerank = k.profile_rerank != 0;
  p.xq = 1;
  if (pair) {  // paired f16 MFMA scan (default): one 512-thread workgroup per CU, 256 queries each
    p.scan_nsplit = nsplit / 2;
    p.grid = (unsigned)(n_qblocks * (nsplit / 2));
    p.block = 512;
    // (the tile ring + the merged records' exchange area: 256 records of 11 floats)
    p.lds = (size_t)4 * 2 * kHalfTileBytes + (size_t)256 * (kMergedLL + 3) * sizeof(float);
    // the XCD rectangle needs whole query-block groups and split groups on every XCD (else: splits only)
    int xq = k.xcd_qgroups;
    {
      const int nqb = n_qblocks, ns = nsplit / 2;
      if (xq < 2 || 8 % xq || nqb % xq || ns % (8 / xq) || (nqb * ns) % 8) xq = 1;
    }
    // option "search_epilogue" = 1: the splits one XCD owns for a query block (sp % GS == x / GQ, GS = 8 / GQ of them interleaved) are
    // contiguous in the query's records — every 128-byte line of the record buffer is written by ONE XCD's L2 (record_slot)
    int slot_bits = 0;
    if (k.search_epilogue && xq > 1)
      for (int gs = 8 / xq; gs > 1; gs >>= 1) ++slot_bits;
    p.xq = xq;
    p.slot_bits = slot_bits;
    // merged records (option "search_merge_lists"): the workgroup's four lists per query leave as one 32-byte record
    // (two more code bits come out of the key's score: kept to shards whose keys still hold 12 score bits below the exponent)
    p.merged = LL == 6 && (k.search_merge == 1 || (k.search_merge == 2 && merge_live && !heavy)) && code_bits <= 9;
    if (p.merged) p.scan = k.search_tile_sel ? (k.search_epilogue ? ScanKernel::kPairMerged1 : ScanKernel::kPairMerged2) : ScanKernel::kPairMerged0;
    else p.scan = LL == 6 ? ScanKernel::kPair6 : ScanKernel::kPair5;
  } else {  // one wave per SIMD (tiny shards, small batches, k > 10, the split-bf16 scan): 256 queries per workgroup
    p.scan_nsplit = nsplit;
    p.grid = (unsigned)(n_qblocks * nsplit);
    p.block = 256;
    p.scan = eff_mode == 0 ? ScanKernel::kWaveF16 : ScanKernel::kWaveBf16;
    p.lds = eff_mode == 0 ? (size_t)4 * kHalfTileBytes : (size_t)4 * kTileFloats * sizeof(float);
  }
  if (p.merged) {  // one record per (query, physical split)
    p.rerank = RerankKernel::kRecords;
    p.rerank_parts = nsplit / 2;
    p.rec6 = k.search_tile_sel ? 1 : 0;
    p.rerank_slot_bits = p.slot_bits;
    p.rerank_form = p.rec6 ? k.rerank_form : 0;
  } else {
    p.rerank = LL == 5 ? RerankKernel::kLists5 : LL == 6 ? RerankKernel::kLists6 : LL == 8 ? RerankKernel::kLists8
             : LL == 16 ? RerankKernel::kLists16 : RerankKernel::kLists32;
    p.rerank_parts = 2 * nsplit;
  }
  return p;
}

}  // namespace t2l
