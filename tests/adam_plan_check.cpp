// CPU check of the optimizer-state layout (text2loc_amd/csrc/adam_plan.h): offsets, chunk table, the backbone's split point, and the
// keep decision of a re-bind. Built and run by tests/test_adam_plan.py; no GPU, no HIP.
#include <stdio.h>

#include "adam_plan.h"

using namespace t2l;

static int failures = 0;
#define CHECK(cond)                                          \
  do {                                                       \
    if (!(cond)) {                                           \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                            \
    }                                                        \
  } while (0)

int main() {
  using V = std::vector<int64_t>;
  using I = std::vector<int32_t>;
  using N = std::vector<std::string>;
  {  // 1, 1023, 1024 -> one chunk each; 1025 -> two; 0 -> none
    const AdamPlan p = adam_plan(V{1, 1023, 1024, 1025, 0});
    CHECK(p.total == 3073 && p.n_chunks() == 5);
    CHECK((p.offset == V{0, 1, 1024, 2048, 3073}));
    CHECK((p.chunk_tensor == I{0, 1, 2, 3, 3}) && (p.chunk_first == I{0, 0, 0, 0, 1}));
    CHECK((p.chunk0 == I{0, 1, 2, 3, 5, 5}));
  }
  {  // the split point: first chunk of the first backbone tensor
    const AdamPlan p = adam_plan(V{2048, 5, 3000, 1});
    CHECK(p.n_chunks() == 7);
    CHECK(p.first_chunk(4) == 7 && p.first_chunk(9) == 7);  // no backbone tensors
    CHECK(p.first_chunk(2) == 3 && p.first_chunk(3) == 6);  // the backbone is the last 2 / the last tensor
    CHECK(p.first_chunk(0) == 0);
    const AdamPlan z = adam_plan(V{2048, 0, 7});  // a backbone whose first tensor has 0 elements: its chunks start at the next one's
    CHECK(z.first_chunk(1) == 2 && z.first_chunk(2) == 2 && z.n_chunks() == 3);
    CHECK(adam_plan(V{4, 0}).first_chunk(1) == 1 && adam_plan(V{}).first_chunk(0) == 0);  // ... or = the chunk count
  }
  {  // the keep decision
    const N ab{"a", "b"}, ba{"b", "a"};
    const V s{3, 4};
    CHECK(!adam_keep(false, true, ab, s, ab, s));           // option off
    CHECK(!adam_keep(true, false, ab, s, ab, s));           // no old state
    CHECK(!adam_keep(true, true, ab, s, ba, s));            // the same names in a different order
    CHECK(!adam_keep(true, true, ab, s, ab, V{3, 5}));      // one size changed
    CHECK(!adam_keep(true, true, ab, s, N{"a"}, V{3}));     // a shorter list
    CHECK(adam_keep(true, true, ab, s, ab, s));             // equal lists
  }
  if (failures) return 1;
  printf("adam_plan_check: ok\n");
  return 0;
}
