// Host-only: the plans of the shapes tests/test_gpu_rerank_form.py runs (search_auto 0, search_merge_lists 1) — each must reach the
// merged-record re-rank, rerank_kernel<kMergedLL, 16, true, FORM>, with the record count the test's docstrings state, and the
// option "search_rerank_form" must pick the instance there and nowhere else. Includes search_plan.h alone.
#include <stdio.h>

#include <initializer_list>

#include "search_plan.h"

using namespace t2l;

static int failures = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      printf("FAILED line %d: %s\n", __LINE__, #c);                \
      ++failures;                                                  \
    }                                                              \
  } while (0)

int main() {
  SearchKnobs k;
  k.search_merge = 1;
  CHECK(k.rerank_form == 1);  // the default
  CHECK(k.nsplit_override == 0 && k.wide_repair == 512);  // the defaults test_gpu_rerank_form.py restores
  for (int K : {1, 10}) {     // N = 1,100, Q = 259: 35 tiles, 16 physical splits -> 16 records per query (lanes 0..15 of the row all hold one)
    const SegmentPlan p = plan_segment(k, 0, true, false, 259, K, 1100);
    CHECK(p.n_tiles == 35 && p.pair && p.merged && p.scan == ScanKernel::kPairMerged1 && p.scan_nsplit == 16);
    CHECK(p.rerank == RerankKernel::kRecords && p.rerank_parts == 16 && p.rec6 == 1 && p.L == 16 && p.rerank_form == 1);
    CHECK(p.grid == 2 * 16);  // two query blocks: the second holds 3 queries, i.e. the last re-rank workgroup has one dead wave
  }
  {  // search_nsplit = 16: 8 physical splits -> 8 records per query (lanes 8..15 of the row hold -inf lists)
    SearchKnobs k8 = k;
    k8.nsplit_override = 16;
    const SegmentPlan p = plan_segment(k8, 0, true, false, 259, 10, 1100);
    CHECK(p.pair && p.merged && p.rerank == RerankKernel::kRecords && p.rerank_parts == 8 && p.rec6 == 1 && p.rerank_form == 1);
  }
  {  // the option: 0 = round 7's instance
    SearchKnobs k0 = k;
    k0.rerank_form = 0;
    const SegmentPlan p = plan_segment(k0, 0, true, false, 259, 10, 1100);
    CHECK(p.rerank == RerankKernel::kRecords && p.rerank_parts == 16 && p.rerank_form == 0);
  }
  {  // records of the per-score insertion carry 7 keys (rec6 = 0): always round 7's instance
    SearchKnobs k7 = k;
    k7.search_tile_sel = 0;
    const SegmentPlan p = plan_segment(k7, 0, true, false, 259, 10, 1100);
    CHECK(p.rerank == RerankKernel::kRecords && p.rec6 == 0 && p.rerank_form == 0);
  }
  {  // plain lists: the option does not apply
    SearchKnobs kl = k;
    kl.search_merge = 0;
    const SegmentPlan p = plan_segment(kl, 0, true, false, 259, 10, 1100);
    CHECK(!p.merged && p.rerank == RerankKernel::kLists6 && p.rerank_form == 0);
  }
  {  // the headline shape under the defaults
    const SearchKnobs d;
    const SegmentPlan p = plan_segment(d, 0, true, false, 4096, 10, 11259);
    CHECK(p.rerank == RerankKernel::kRecords && p.rerank_parts == 16 && p.rerank_form == 1);
  }
  if (failures) return 1;
  printf("rerank_form_plan_check: ok\n");
  return 0;
}
