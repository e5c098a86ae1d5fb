// Host test of vimo_clip_amd/csrc/weight_tile.h: the record sizes the ABI documents, the search for the record that owns a block
// against a linear scan (tile0 of the descriptors, block0 of the ranges), and the truth table of the vector-path predicate.  Built
// with g++ by tests/test_host_weight_tile.py.
#include <cstdio>
#include <vector>

#include "../../vimo_clip_amd/csrc/weight_tile.h"

static int fails = 0, cases = 0;
#define CHECK(c, ...) do { ++cases; if (!(c)) { if (fails < 30) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++fails; } } while (0)

// the owner of block b by definition: the last record that starts at or before it
template <typename R>
static int scan(const std::vector<R>& rec, int b) {
  int own = 0;
  for (int i = 0; i < (int)rec.size(); ++i)
    if (first_block(rec[i]) <= b) own = i;
  return own;
}

// records of the given block counts, in both forms; every block of the grid is looked up
static void check_owner(const char* name, const std::vector<int>& counts) {
  std::vector<CastDesc> desc;
  std::vector<AdamRange> ranges;
  int total = 0;
  for (int c : counts) {
    CastDesc d = {};
    d.tile0 = total;
    desc.push_back(d);
    ranges.push_back(AdamRange{0ull, 1024 * c, total});
    total += c;
  }
  const int n = (int)counts.size();
  for (int b = 0; b < total; ++b) {
    const int want = scan(desc, b);
    CHECK(b >= desc[want].tile0 && b < desc[want].tile0 + counts[want], "%s: scan of block %d", name, b);
    CHECK(owner_of_block(desc.data(), n, b) == want, "%s: tile %d -> %d, want %d", name, b, owner_of_block(desc.data(), n, b), want);
    CHECK(owner_of_block(ranges.data(), n, b) == scan(ranges, b) && scan(ranges, b) == want, "%s: range block %d -> %d, want %d", name, b,
          owner_of_block(ranges.data(), n, b), want);
  }
}

static void test_owner() {
  check_owner("one record, one tile", {1});
  check_owner("one record", {35});
  check_owner("two records", {1, 1});
  check_owner("one tile each", std::vector<int>(17, 1));
  check_owner("one tile beside many", {1, 64, 1, 1, 9, 1, 128, 1});
  check_owner("many beside one tile", {48, 1, 1, 30, 1});
  std::vector<int> mixed;
  for (int i = 0; i < 150; ++i) mixed.push_back(i % 7 == 0 ? 1 : 1 + (i * 37) % 23);
  check_owner("150 records", mixed);
  for (int n = 1; n <= 9; ++n) check_owner("n records of 3", std::vector<int>(n, 3));      // every parity of the bisection
}

static CastDesc good() {
  CastDesc d = {};
  d.w = (const float*)0x10000;
  d.w16 = (uint16_t*)0x20000;
  d.w16t = (uint16_t*)0x30000;
  d.rows = 68, d.cols = 132, d.ld = 192, d.ldt = 128, d.tiles_x = 3;
  return d;
}

static void test_predicate() {
  CHECK(tile_vec_ok(good()), "aligned record");
  for (int off = 4; off < 16; off += 4) {      // a float pointer is 4-byte aligned at least
    CastDesc d = good();
    d.w = (const float*)(0x10000 + off);
    CHECK(!tile_vec_ok(d), "master off by %d bytes", off);
  }
  for (int k = 1; k < 4; ++k) {
    CastDesc d = good();
    d.rows += k;
    CHECK(!tile_vec_ok(d), "rows %d", d.rows);
    d = good();
    d.cols += k;
    CHECK(!tile_vec_ok(d), "cols %d", d.cols);
    d = good();
    d.ld += k;
    CHECK(!tile_vec_ok(d), "ld %d", d.ld);
    d = good();
    d.ldt += k;
    CHECK(!tile_vec_ok(d), "ldt %d", d.ldt);
  }
  for (int off = 2; off < 8; off += 2) {       // the copies: 8-byte stores
    CastDesc d = good();
    d.w16 = (uint16_t*)(0x20000 + off);
    CHECK(!tile_vec_ok(d), "w16 off by %d bytes", off);
    d = good();
    d.w16t = (uint16_t*)(0x30000 + off);
    CHECK(!tile_vec_ok(d), "w16t off by %d bytes", off);
  }
  {   // 8-byte aligned copies are enough
    CastDesc d = good();
    d.w16 = (uint16_t*)0x20008, d.w16t = (uint16_t*)0x30008;
    CHECK(tile_vec_ok(d), "copies at 8 mod 16");
  }
  {   // a missing copy: its stride and pointer do not count, the other copy's still do
    CastDesc d = good();
    d.w16 = nullptr, d.ld = 133;
    CHECK(tile_vec_ok(d), "w16 NULL with an odd ld");
    d.ldt = 130;
    CHECK(!tile_vec_ok(d), "w16 NULL, ldt 130");
    d = good();
    d.w16t = nullptr, d.ldt = 67;
    CHECK(tile_vec_ok(d), "w16t NULL with an odd ldt");
    d.w16 = (uint16_t*)0x20002;
    CHECK(!tile_vec_ok(d), "w16t NULL, w16 off by 2 bytes");
    d = good();
    d.w16 = nullptr, d.w16t = nullptr, d.ld = 1, d.ldt = 1;
    CHECK(tile_vec_ok(d), "both copies NULL");
    d.w = (const float*)0x10004;
    CHECK(!tile_vec_ok(d), "both copies NULL, master off by 4 bytes");
  }
}

int main() {
  CHECK(sizeof(CastDesc) == 48, "CastDesc is %zu bytes", sizeof(CastDesc));
  CHECK(sizeof(AdamRange) == 16, "AdamRange is %zu bytes", sizeof(AdamRange));
  test_owner();
  test_predicate();
  if (fails) {
    printf("%d of %d checks failed\n", fails, cases);
    return 1;
  }
  printf("OK %d checks\n", cases);
  return 0;
}
