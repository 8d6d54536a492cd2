// CPU check of what every eval-mode weight loader runs before it touches the device (text2loc_amd/csrc/weight_table.h): the name table
// of a descriptor list with its two error texts, and the host image of a model part's one device blob. Built and run by
// tests/test_weight_table.py; no GPU, no HIP.
#include <stdio.h>

#include "weight_table.h"

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
  float a[6] = {1, 2, 3, 4, 5, 6}, b[2] = {7, 8}, a2[6] = {9, 9, 9, 9, 9, 9};
  {  // a found tensor, the optional lookup, any-size lookups, and the two error texts
    const t2l_weight_desc list[] = {{"enc.w", a, 6}, {"enc.b", b, 2}};
    WeightTable T("t2l_some_load", list, 2);
    CHECK(T.ok() && !T.empty() && T.error().empty());
    CHECK(T.need("enc.w", 6) == a && T.need("enc.b", 2) == b && T.need("enc.b", 0) == b);
    CHECK(T.find("enc.w") == &list[0] && T.find("enc.w")->numel == 6 && T.find("enc.x") == nullptr);
    CHECK(T.ok());  // find() of an absent tensor is no error
    CHECK(T.need("enc.x", 3) == nullptr && !T.ok());
    CHECK(T.error() == "t2l_some_load: missing tensor 'enc.x'");
    // after an error the table keeps answering and keeps reporting that FIRST error
    CHECK(T.need("enc.w", 6) == a);
    CHECK(T.need("enc.b", 3) == nullptr && T.need("enc.y", 0) == nullptr && T.refuse("something else") == nullptr);
    CHECK(T.error() == "t2l_some_load: missing tensor 'enc.x'");
    WeightTable U("t2l_other_load", list, 2);
    CHECK(U.need("enc.b", 3) == nullptr);
    CHECK(U.error() == "t2l_other_load: wrong size for 'enc.b' (has 2 elements, needs 3)");
    CHECK(U.need("enc.x", 1) == nullptr && U.error() == "t2l_other_load: wrong size for 'enc.b' (has 2 elements, needs 3)");
    WeightTable V("t2l_other_load", list, 2);  // a size that is a rule, not a number: an embedding table of however many rows
    int64_t rows = 0;
    CHECK(V.need_rows("enc.w", 3, &rows) == a && rows == 2 && V.need_rows("enc.w", 6, &rows) == a && rows == 1 && V.ok());
    CHECK(V.need_rows("enc.w", 4, &rows) == nullptr && rows == 1);
    CHECK(V.error() == "t2l_other_load: wrong size for 'enc.w' (has 6 elements, needs a multiple of 4)");
    WeightTable X("t2l_other_load", list, 2);
    CHECK(X.need_rows("enc.x", 4, &rows) == nullptr && X.error() == "t2l_other_load: missing tensor 'enc.x'");
  }
  {  // a null name, null data and a non-positive numel are refused once, at construction — also behind good tensors
    const t2l_weight_desc null_name[] = {{"ok", a, 6}, {nullptr, b, 2}};
    const t2l_weight_desc null_data[] = {{"ok", a, 6}, {"bad", nullptr, 2}};
    const t2l_weight_desc zero[] = {{"bad", b, 0}}, negative[] = {{"bad", b, -2}};
    WeightTable N("who", null_name, 2), D("who", null_data, 2), Z("who", zero, 1), M("who", negative, 1);
    CHECK(!N.ok() && N.error() == "who: tensor 1 has a null name, null data or numel <= 0");
    CHECK(!D.ok() && D.error() == "who: tensor 1 ('bad') has a null name, null data or numel <= 0");
    CHECK(!Z.ok() && Z.error() == "who: tensor 0 ('bad') has a null name, null data or numel <= 0");
    CHECK(!M.ok() && M.error() == Z.error());
    CHECK(D.need("nothing", 1) == nullptr && D.error() == "who: tensor 1 ('bad') has a null name, null data or numel <= 0");
    WeightTable E("who", nullptr, 0);  // an empty list is a table without tensors, not an error
    CHECK(E.ok() && E.empty());
  }
  {  // of two tensors of one name the later one counts
    const t2l_weight_desc list[] = {{"w", a, 6}, {"v", b, 2}, {"w", a2, 6}, {"v", a, 6}};
    WeightTable T("who", list, 4);
    CHECK(T.ok() && T.need("w", 6) == a2 && T.need("v", 6) == a && T.need("v", 2) == nullptr);
    CHECK(T.error() == "who: wrong size for 'v' (has 6 elements, needs 2)");
  }
  {  // the prefix filter: only names under it are in the table; a list with none of them is an empty table
    const t2l_weight_desc list[] = {{"net.pointnet.w", a, 6}, {"net.other.w", b, 2}, {"net.pointnet", a2, 6}};
    WeightTable T("who", list, 3, "net.pointnet.");
    CHECK(T.ok() && !T.empty());
    CHECK(T.need("net.pointnet.w", 6) == a && T.find("net.other.w") == nullptr && T.find("net.pointnet") == nullptr);
    WeightTable O("who", list, 3, "net.absent.");
    CHECK(O.ok() && O.empty());
    const t2l_weight_desc bad[] = {{"net.other.w", nullptr, 2}};  // the refusal covers the whole list, whatever the prefix
    CHECK(!WeightTable("who", bad, 1, "net.pointnet.").ok());
  }
  {  // Staging: offsets at the requested alignment (16: the cell encoder; 256, the default: everything else), zero fill, round trip
    Staging s;
    const std::vector<float> v3{1.5f, -2.f, 3.25f}, v5{5, 6, 7, 8, 9};
    const std::vector<uint16_t> h{0x3c00, 0xbc00, 0x7bff};
    CHECK(s.bytes() == 0);
    CHECK(s.add(v3, 16) == 0 && s.bytes() == 12);
    CHECK(s.add(v5, 16) == 16 && s.bytes() == 36);
    CHECK(s.add(h, 16) == 48 && s.bytes() == 54);
    CHECK(s.add(v3) == 256 && s.bytes() == 268);             // the default alignment
    CHECK(s.add(b, sizeof(b), 256) == 512 && s.bytes() == 520);
    CHECK(s.add(v5.data(), 0, 16) == 528 && s.bytes() == 528);  // an empty array still gets an aligned offset
    const unsigned char* d = static_cast<const unsigned char*>(s.data());
    CHECK(!memcmp(d, v3.data(), 12) && !memcmp(d + 16, v5.data(), 20) && !memcmp(d + 48, h.data(), 6) && !memcmp(d + 256, v3.data(), 12) &&
          !memcmp(d + 512, b, 8));
    bool zero = true;
    for (size_t i : {12u, 15u, 36u, 47u, 54u, 255u, 268u, 511u, 520u, 527u}) zero = zero && d[i] == 0;
    CHECK(zero);
  }
  {  // place + bind: the pointer fields of a parameter struct end up at base + offset, of whatever pointer type they are
    struct Params {
      const float* w = nullptr;
      const uint16_t* h = nullptr;
      char* plane = nullptr;
      const float* untouched = nullptr;
    } P;
    Staging s;
    const std::vector<float> v{1, 2, 3};
    const std::vector<uint16_t> h{4, 5};
    s.place(&P.w, v);
    s.place(&P.h, h, 16);
    s.place(&P.plane, a, 6);
    CHECK(P.w == nullptr && P.h == nullptr && P.plane == nullptr);  // nothing points anywhere before the blob has an address
    std::vector<unsigned char> device(s.bytes());  // stands in for the device copy
    memcpy(device.data(), s.data(), s.bytes());
    char* base = reinterpret_cast<char*>(device.data());
    s.bind(base);
    CHECK((const char*)P.w == base && (const char*)P.h == base + 16 && P.plane == base + 256 && P.untouched == nullptr);
    CHECK(P.w[2] == 3.f && P.h[1] == 5 && !memcmp(P.plane, a, sizeof(a)));
  }
  if (failures) return 1;
  printf("weight_table_check: ok\n");
  return 0;
}
