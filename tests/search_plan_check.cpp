// CPU check of the search host path (text2loc_amd/csrc/search_plan.h): the launch plan of a (Q, k, rows, options) call as a table,
// and the report-card state machine fed hand-written report cards. Built and run by tests/test_search_plan.py; no GPU, no HIP.
#include <math.h>
#include <stdio.h>

#include "search_plan.h"

using namespace t2l;

static int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
      ++failures;                                                    \
    }                                                                \
  } while (0)

// ---- the plan table ----------------------------------------------------------------------------
struct Row {
  const char* what;
  int Q, K, rows;
  int n_tiles, nsplit;
  bool pair;
  int code_bits, LL, L;
  ScanKernel scan;
  unsigned grid;
  int xq, slot_bits;  // (-1: not a paired launch, the plan leaves xq = 1 and slot_bits = 0)
  size_t cand_floats;
};

static SegmentPlan plan(const SearchKnobs& k, int eff_mode, bool merge_live, bool heavy, int Q, int K, int rows) {
  return plan_segment(k, eff_mode, merge_live, heavy, Q, K, rows);
}

static void check_row(const Row& r, const SegmentPlan& p) {
  const bool ok = p.n_tiles == r.n_tiles && p.nsplit == r.nsplit && p.pair == r.pair && p.code_bits == r.code_bits && p.LL == r.LL &&
                  p.L == r.L && p.scan == r.scan && p.grid == r.grid && p.xq == (r.xq < 0 ? 1 : r.xq) &&
                  p.slot_bits == (r.slot_bits < 0 ? 0 : r.slot_bits) && p.cand_bytes == r.cand_floats * sizeof(float) &&
                  p.per == (r.n_tiles + r.nsplit - 1) / r.nsplit && p.block == (r.pair ? 512u : 256u);
  if (!ok) {
    printf("FAIL plan row '%s': n_tiles %d nsplit %d pair %d code_bits %d LL %d L %d scan %d grid %u xq %d slot_bits %d cand %zu per %d\n", r.what,
           p.n_tiles, p.nsplit, (int)p.pair, p.code_bits, p.LL, p.L, (int)p.scan, p.grid, p.xq, p.slot_bits, p.cand_bytes / sizeof(float), p.per);
    ++failures;
  }
}

static void plan_table() {
  const SearchKnobs d;  // the defaults: pair_ll 6, search_merge 2, tile_sel 1, epilogue 1, xcd_qgroups 4, f16 mode
  using S = ScanKernel;
  check_row({"4096 x 11259", 4096, 10, 11259, 352, 32, true, 8, 6, 16, S::kPairMerged1, 256, 4, 1, 1572864}, plan(d, 0, true, false, 4096, 10, 11259));
  check_row({"merge_live false", 4096, 10, 11259, 352, 32, true, 8, 6, 16, S::kPair6, 256, 4, 1, 1572864}, plan(d, 0, false, false, 4096, 10, 11259));
  {
    SearchKnobs k;
    k.pair_ll = 5;
    check_row({"pair_ll 5", 4096, 10, 11259, 352, 32, true, 8, 5, 16, S::kPair5, 256, 4, 1, 1310720}, plan(k, 0, true, false, 4096, 10, 11259));
  }
  {
    SearchKnobs k;
    k.search_mode = 2;
    const SegmentPlan p = plan(k, 2, true, false, 4096, 10, 11259);
    check_row({"split-bf16 mode", 4096, 10, 11259, 352, 16, false, 9, 8, 16, S::kWaveBf16, 256, -1, -1, 1048576}, p);
    CHECK(p.lds == (size_t)4 * kTileFloats * sizeof(float) && p.scan_nsplit == 16 && p.half_mode == 0 && p.stat_mode == 0 && p.eps_probe == 0.f);
    CHECK(fabs(p.eps_rel - 3.5735626e-5) < 1e-11);  // 264 * 2^-24 + 2e-5
    CHECK(p.rerank == RerankKernel::kLists8 && p.rerank_parts == 32);
  }
  {
    SearchKnobs k;
    k.nsplit_override = 8;
    check_row({"search_nsplit 8", 4096, 10, 11259, 352, 8, false, 10, 8, 16, S::kWaveF16, 128, -1, -1, 524288}, plan(k, 0, true, false, 4096, 10, 11259));
  }
  {
    const SegmentPlan p = plan(d, 0, true, false, 4096, 26, 11259);
    check_row({"k 26", 4096, 26, 11259, 352, 16, false, 9, 32, 32, S::kWaveF16, 256, -1, -1, 4194304}, p);
    CHECK(p.rerank == RerankKernel::kLists32 && p.rerank_parts == 32);
  }
  check_row({"Q 300", 300, 10, 11259, 352, 32, true, 8, 6, 16, S::kPairMerged1, 32, 1, 0, 196608}, plan(d, 0, true, false, 300, 10, 11259));
  check_row({"Q 255", 255, 10, 11259, 352, 32, false, 8, 8, 16, S::kWaveF16, 32, -1, -1, 131072}, plan(d, 0, true, false, 255, 10, 11259));
  check_row({"256 x 512", 256, 10, 512, 16, 16, false, 4, 8, 16, S::kWaveF16, 16, -1, -1, 65536}, plan(d, 0, true, false, 256, 10, 512));
  check_row({"256 x 480", 256, 10, 480, 15, 15, false, 4, 8, 16, S::kWaveF16, 15, -1, -1, 61440}, plan(d, 0, true, false, 256, 10, 480));
  {
    const SegmentPlan p = plan(d, 0, true, false, 17, 10, 33);
    check_row({"17 x 33", 17, 10, 33, 2, 2, false, 4, 16, 16, S::kWaveF16, 2, -1, -1, 16384}, p);
    CHECK(p.rerank == RerankKernel::kLists16 && p.rerank_parts == 4 && p.lds == (size_t)4 * kHalfTileBytes);
  }
  check_row({"65 x 70000", 65, 10, 70000, 2188, 32, false, 11, 8, 16, S::kWaveF16, 32, -1, -1, 131072}, plan(d, 0, true, false, 65, 10, 70000));
  {  // more than 9 code bits: the records are not merged
    const SegmentPlan p = plan(d, 0, true, false, 2048, 10, 400000);
    check_row({"2048 x 400000", 2048, 10, 400000, 12500, 32, true, 13, 6, 16, S::kPair6, 128, 4, 1, 786432}, p);
    CHECK(!p.merged && p.rerank == RerankKernel::kLists6 && p.rerank_parts == 64 && p.rec6 == 0 && p.rerank_slot_bits == 0);
  }
  {  // two segments: a full one, then one row
    const Segments s = segments_of(524289, 10);
    CHECK(s.n_seg == 2 && !s.too_large);
    check_row({"segment 0 of 524289", 4096, 10, kSegmentRows, 16384, 32, true, 13, 6, 16, S::kPair6, 256, 4, 1, 1572864},
              plan(d, 0, true, false, 4096, 10, kSegmentRows));
    check_row({"segment 1 of 524289", 4096, 10, 1, 1, 1, false, 4, 16, 16, S::kWaveF16, 16, -1, -1, 131072}, plan(d, 0, true, false, 4096, 10, 1));
  }

  // the smallest paired shard at Q = 256: 32 tiles without an override, 16 tiles with search_nsplit 16
  CHECK(plan(d, 0, true, false, 256, 10, 993).pair && plan(d, 0, true, false, 256, 10, 993).n_tiles == 32);
  CHECK(!plan(d, 0, true, false, 256, 10, 992).pair);
  {
    SearchKnobs k;
    k.nsplit_override = 16;
    const SegmentPlan p = plan(k, 0, true, false, 256, 10, 481);
    CHECK(p.pair && p.n_tiles == 16 && p.nsplit == 16 && p.scan_nsplit == 8 && p.grid == 8);
    CHECK(!plan(k, 0, true, false, 256, 10, 480).pair);
    // the key code stays within 13 bits: an override too small for the shard is raised (paired: physical splits; one-wave: splits)
    const SegmentPlan big = plan(k, 0, true, false, 2048, 10, 400000);
    CHECK(big.pair && big.nsplit == 26 && big.scan_nsplit == 13 && big.xq == 1 && big.slot_bits == 0 && big.code_bits == 13);
    k.nsplit_override = 8;
    const SegmentPlan wave = plan(k, 0, true, false, 100, 10, 400000);
    CHECK(!wave.pair && wave.nsplit == 25 && wave.per == 500 && wave.code_bits == 13);
  }
  // segments_of: too large above 256 / K segments, not one segment below
  CHECK(segments_of(1, 10).n_seg == 1 && segments_of(kSegmentRows, 10).n_seg == 1 && segments_of(kSegmentRows + 1, 10).n_seg == 2);
  CHECK(!segments_of(25 * kSegmentRows, 10).too_large && segments_of(25 * kSegmentRows + 1, 10).too_large);
  CHECK(!segments_of(256 * kSegmentRows, 1).too_large && segments_of(256 * kSegmentRows + 1, 1).too_large);

  // ---- the remaining branches: what the default launch hands its two kernels
  {
    const SegmentPlan p = plan(d, 0, true, false, 4096, 10, 11259);
    CHECK(p.merged && p.rerank == RerankKernel::kRecords && p.rerank_parts == 16 && p.rec6 == 1 && p.rerank_slot_bits == 1 && p.scan_nsplit == 16);
    CHECK(p.lds == (size_t)4 * 2 * kHalfTileBytes + (size_t)256 * 11 * sizeof(float));
    CHECK(p.half_mode == 1 && p.stat_mode == 1 && p.defer == 0 && p.eps_probe == 0.f && p.wide_cap == 512 && p.time_rerank);
    CHECK(fabs(p.eps_rel - 1.0007356e-3) < 1e-10);  // 264 * 2^-24 + 9.85e-4
  }
  {  // heavy: plain lists, unsettled queries deferred
    const SegmentPlan p = plan(d, 0, true, true, 4096, 10, 11259);
    CHECK(!p.merged && p.scan == ScanKernel::kPair6 && p.defer == 1 && p.rerank == RerankKernel::kLists6);
  }
  {  // the split-bf16 scan standing in for the f16 scan: it probes with the f16 band
    const SegmentPlan p = plan(d, 2, true, false, 4096, 10, 11259);
    CHECK(p.scan == ScanKernel::kWaveBf16 && p.stat_mode == 2 && p.half_mode == 0);
    CHECK(fabs(p.eps_probe - 1.0007356e-3) < 1e-10 && fabs(p.eps_rel - 3.5735626e-5) < 1e-11);
  }
  {
    SearchKnobs k;
    k.search_merge = 0;
    CHECK(plan(k, 0, true, false, 4096, 10, 11259).scan == ScanKernel::kPair6);
    k.search_merge = 1;  // always: whatever the report cards say, but not past 9 code bits
    CHECK(plan(k, 0, false, true, 4096, 10, 11259).scan == ScanKernel::kPairMerged1);
    CHECK(plan(k, 0, true, false, 2048, 10, 400000).scan == ScanKernel::kPair6);
    k.pair_ll = 5;
    CHECK(plan(k, 0, true, false, 4096, 10, 11259).scan == ScanKernel::kPair5 && !plan(k, 0, true, false, 4096, 10, 11259).merged);
  }
  {
    SearchKnobs k;
    k.search_tile_sel = 0;
    const SegmentPlan p0 = plan(k, 0, true, false, 4096, 10, 11259);
    CHECK(p0.scan == ScanKernel::kPairMerged0 && p0.rec6 == 0 && p0.slot_bits == 1);
    k.search_epilogue = 0;
    CHECK(plan(k, 0, true, false, 4096, 10, 11259).scan == ScanKernel::kPairMerged0);
    k.search_tile_sel = 1;
    const SegmentPlan p2 = plan(k, 0, true, false, 4096, 10, 11259);
    CHECK(p2.scan == ScanKernel::kPairMerged2 && p2.rec6 == 1 && p2.xq == 4 && p2.slot_bits == 0 && p2.rerank_slot_bits == 0);
  }
  {
    SearchKnobs k;
    k.xcd_qgroups = 1;
    CHECK(plan(k, 0, true, false, 4096, 10, 11259).xq == 1 && plan(k, 0, true, false, 4096, 10, 11259).slot_bits == 0);
    k.xcd_qgroups = 2;
    CHECK(plan(k, 0, true, false, 4096, 10, 11259).xq == 2 && plan(k, 0, true, false, 4096, 10, 11259).slot_bits == 2);
    k.xcd_qgroups = 8;
    CHECK(plan(k, 0, true, false, 4096, 10, 11259).xq == 8 && plan(k, 0, true, false, 4096, 10, 11259).slot_bits == 0);
    CHECK(plan(k, 0, true, false, 1024, 10, 11259).xq == 1);  // 4 query blocks: no whole group of 8
    k.wide_repair = 0;
    k.profile_rerank = 0;
    k.eps_scale = 2.0;
    const SegmentPlan p = plan(k, 0, true, false, 4096, 10, 11259);
    CHECK(p.wide_cap == 0 && !p.time_rerank && fabs(p.eps_rel - 2.0014712e-3) < 2e-10);
    k.wide_repair = 4096;
    CHECK(plan(k, 0, true, false, 4096, 10, 11259).wide_cap == kWideCap);
  }
}

// ---- the policy ----------------------------------------------------------------------------------
struct Card {
  int32_t v[kStatInts];
};
static Card card(int seq, int stat, int total, int flagged, int rescored, int exact) {
  Card c{};
  c.v[kStatSeq] = seq;
  c.v[kStatMode] = stat;
  c.v[kStatTotal] = total;
  c.v[kStatFlagged] = flagged;
  c.v[kStatRescored] = rescored;
  c.v[kStatExact] = exact;
  return c;
}

static void policy_sequences() {
  {  // f16 reports: more than 1 in 8 flagged escalates
    SearchPolicy p;
    p.observe(card(1, 1, 4096, 512, 0, 0).v, 0, true);  // flagged * 8 == total
    CHECK(!p.escalated && p.stat_seen == 1 && p.eff_mode(0) == 0);
    p.observe(card(2, 1, 4096, 513, 0, 0).v, 0, true);  // flagged * 8 == total + 8
    CHECK(p.escalated && p.eff_mode(0) == 2 && p.eff_mode(2) == 2);
  }
  {  // ... or more than 1 in 2 failing the first certificate, alone
    SearchPolicy p;
    p.observe(card(1, 1, 4096, 0, 2048, 0).v, 0, true);
    CHECK(!p.escalated);
    p.observe(card(2, 1, 4096, 0, 2049, 0).v, 0, true);
    CHECK(p.escalated);
  }
  {  // neither with search_auto off or search_mode 2
    SearchPolicy p;
    p.observe(card(1, 1, 4096, 4096, 4096, 0).v, 0, false);
    CHECK(!p.escalated && p.stat_seen == 1);
    p.observe(card(2, 1, 4096, 4096, 4096, 0).v, 2, true);
    CHECK(!p.escalated && p.stat_seen == 2 && p.eff_mode(2) == 2);
  }
  {  // an f16 report arriving after escalation does not release it; a probe report does, below 1 in 16
    SearchPolicy p;
    p.observe(card(1, 1, 4096, 4096, 0, 0).v, 0, true);
    CHECK(p.escalated);
    p.observe(card(2, 1, 4096, 0, 0, 0).v, 0, true);
    CHECK(p.escalated);
    p.observe(card(3, 2, 4096, 256, 256, 0).v, 0, true);  // flagged * 16 == total
    CHECK(p.escalated);
    p.observe(card(4, 2, 4096, 255, 255, 0).v, 0, true);
    CHECK(!p.escalated);
    p.observe(card(5, 2, 4096, 4096, 4096, 0).v, 0, true);  // a probe report never escalates
    CHECK(!p.escalated);
  }
  {  // merge_live: drops above 1 in 64, returns at 1 in 256 or below, only on f16 reports (search_auto or not)
    SearchPolicy p;
    p.observe(card(1, 1, 4096, 0, 64, 0).v, 0, true);
    CHECK(p.merge_live);
    p.observe(card(2, 2, 4096, 0, 4096, 0).v, 0, true);
    CHECK(p.merge_live);
    p.observe(card(3, 0, 4096, 0, 4096, 0).v, 0, true);
    CHECK(p.merge_live);
    p.observe(card(4, 1, 4096, 0, 65, 0).v, 0, false);
    CHECK(!p.merge_live);
    p.observe(card(5, 1, 4096, 0, 17, 0).v, 0, true);
    CHECK(!p.merge_live);
    p.observe(card(6, 2, 4096, 0, 0, 0).v, 0, true);
    CHECK(!p.merge_live);
    p.observe(card(7, 1, 4096, 0, 16, 0).v, 0, true);  // rescored * 256 == total
    CHECK(p.merge_live);
  }
  {  // heavy: on above 1 in 64 in an exact stage, off below 1 in 256
    SearchPolicy p;
    p.observe(card(1, 1, 4096, 0, 0, 64).v, 0, true);
    CHECK(!p.heavy);
    p.observe(card(2, 1, 4096, 0, 0, 65).v, 0, true);
    CHECK(p.heavy);
    p.observe(card(3, 1, 4096, 0, 0, 16).v, 0, true);  // exact * 256 == total
    CHECK(p.heavy);
    p.observe(card(4, 0, 4096, 0, 0, 15).v, 0, true);  // (any counted report: an all-exact call's included)
    CHECK(!p.heavy);
    p.observe(card(5, 1, 4096, 0, 0, 4096).v, 0, false);  // not with search_auto off
    CHECK(!p.heavy);
  }
  {  // all_exact: only a probe report with heavy (as that report leaves it) and 7 in 8 in the exact stage; any f16 report clears it
    SearchPolicy p;
    p.observe(card(1, 2, 4096, 0, 0, 3584).v, 0, true);  // exact * 8 == total * 7; the same report turns heavy on
    CHECK(p.heavy && p.all_exact);
    p.observe(card(2, 0, 4096, 0, 0, 4096).v, 0, true);  // an all-exact call's own report changes nothing
    CHECK(p.all_exact);
    p.observe(card(3, 1, 4096, 0, 0, 4096).v, 0, true);
    CHECK(p.heavy && !p.all_exact);
    p.observe(card(4, 2, 4096, 0, 0, 3583).v, 0, true);
    CHECK(p.heavy && !p.all_exact);
    p.observe(card(5, 1, 4096, 0, 0, 4096).v, 0, true);  // an f16 report never sets it
    CHECK(!p.all_exact);
    p.observe(card(6, 2, 4096, 0, 0, 4096).v, 0, true);
    CHECK(p.all_exact);
    p.observe(card(7, 2, 4096, 0, 0, 15).v, 0, true);  // heavy released by the same report: not all-exact
    CHECK(!p.heavy && !p.all_exact);
    SearchPolicy off;
    off.heavy = true;  // (option "search_heavy")
    off.observe(card(1, 2, 4096, 0, 0, 4096).v, 0, false);
    CHECK(off.heavy && !off.all_exact);
  }
  {  // total == 0 teaches nothing; a sequence number not above stat_seen is ignored
    SearchPolicy p;
    p.observe(card(1, 1, 0, 4096, 4096, 4096).v, 0, true);
    CHECK(!p.escalated && !p.heavy && p.merge_live && !p.all_exact && p.stat_seen == 1);
    p.observe(card(1, 1, 4096, 4096, 4096, 4096).v, 0, true);
    CHECK(!p.escalated && !p.heavy && p.merge_live && p.stat_seen == 1);
    p.observe(card(0, 1, 4096, 4096, 4096, 4096).v, 0, true);
    CHECK(!p.escalated && !p.heavy && p.merge_live && p.stat_seen == 1);
    p.observe(card(2, 1, 4096, 4096, 4096, 4096).v, 0, true);
    CHECK(p.escalated && p.heavy && !p.merge_live && p.stat_seen == 2);
  }
  {  // reset(true) ignores the next-numbered report, reset(false) does not
    SearchPolicy p;
    p.stat_seq = 5;
    p.observe(card(5, 1, 4096, 4096, 4096, 4096).v, 0, true);
    CHECK(p.escalated && p.heavy && !p.merge_live);
    p.all_exact = true;
    p.reset(true);
    CHECK(!p.escalated && !p.heavy && !p.all_exact && p.merge_live && p.stat_seen == 6 && p.stat_seq == 5);
    p.observe(card(6, 1, 4096, 4096, 4096, 4096).v, 0, true);
    CHECK(!p.escalated && !p.heavy && p.merge_live);
    p.observe(card(7, 1, 4096, 4096, 4096, 4096).v, 0, true);
    CHECK(p.escalated && p.heavy && !p.merge_live);
    p.stat_seq = 7;
    p.reset(false);
    CHECK(!p.escalated && !p.heavy && p.merge_live && p.stat_seen == 7);
    p.observe(card(7, 1, 4096, 4096, 4096, 4096).v, 0, true);
    CHECK(!p.escalated);
    p.observe(card(8, 1, 4096, 4096, 4096, 4096).v, 0, true);
    CHECK(p.escalated && p.heavy);
  }
  {  // the prior
    SearchPolicy a, b, c;
    a.seed_from_prior(0.91);
    b.seed_from_prior(0.9);
    c.seed_from_prior(nan(""));
    CHECK(a.escalated && a.heavy && !a.all_exact && a.merge_live);
    CHECK(!b.escalated && !b.heavy && !c.escalated && !c.heavy);
  }
  {  // take_all_exact: seven calls in eight, never with more than one segment, never without heavy and all_exact
    SearchPolicy p;
    CHECK(!p.take_all_exact(1));
    p.heavy = true;
    CHECK(!p.take_all_exact(1));
    p.all_exact = true;
    CHECK(p.all_exact_calls == 0);  // (calls that do not qualify do not advance the cadence)
    for (int i = 0; i < 24; ++i) CHECK(p.take_all_exact(1) == ((i & 7) != 7));
    for (int i = 0; i < 16; ++i) CHECK(!p.take_all_exact(2));
    CHECK(p.all_exact_calls == 24);
    p.heavy = false;
    CHECK(!p.take_all_exact(1));
  }
}

int main() {
  plan_table();
  policy_sequences();
  if (failures) {
    printf("%d check(s) failed\n", failures);
    return 1;
  }
  printf("search_plan_check: ok\n");
  return 0;
}
