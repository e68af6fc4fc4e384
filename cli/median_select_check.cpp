// cli/median_select_check.cpp -- host-only check of the selection core of the median layout (glia_amd/csrc/median_select.hpp):
// the order statistic of a multiset given as signed sorted runs against std::nth_element on the materialised set.
//   median_select_check [cases] [seed]     exit 0 and one summary line when every case agrees
// A case: up to 100 sorted runs; up to two of them are entered a second time with sign -1 (the multiset difference of the median
// layout: B(u + v) = B(u) + B(v) - (u -> v) - (v -> u)).  Values: quantised (many ties) or distinct f32; lengths 0, 1, 2, odd, even;
// all-equal runs; differences that leave one element or none.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../glia_amd/csrc/median_select.hpp"

using glia::SignedRun;

static uint64_t s_state;
static uint64_t rnd() { s_state ^= s_state << 13; s_state ^= s_state >> 7; s_state ^= s_state << 17; return s_state; }
static bool key_less(float a, float b) { return glia::float_ord(a) < glia::float_ord(b); }

int main(int argc, char** argv) {
  const long cases = argc > 1 ? atol(argv[1]) : 4000;
  s_state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 0x9E3779B97F4A7C15ull;
  long checked = 0, empty = 0, single = 0, with_diff = 0;
  for (long t = 0; t < cases; ++t) {
    const int mode = (int)(rnd() % 4);                   // 0 quantised, 1 distinct, 2 all-equal runs, 3 a difference that leaves <= 1 element
    int n_runs = mode == 3 ? 1 + (int)(rnd() % 2) : (int)(rnd() % 101);
    std::vector<std::vector<float>> runs(n_runs);
    uint32_t next_distinct = 0x3C000000u + (uint32_t)(rnd() % 1000);
    for (auto& r : runs) {
      static const int kLen[] = {0, 1, 2, 3, 4, 7, 8, 63, 64, 65};
      size_t len = rnd() % 3 ? (size_t)kLen[rnd() % 10] : (size_t)(rnd() % 300);
      if (mode == 3 && len == 0) len = 1 + rnd() % 5;
      r.resize(len);
      const float same = (float)(rnd() % 16) / 16.0f - 0.5f;
      for (float& x : r) {
        if (mode == 1) { const uint32_t u = (next_distinct += 1 + (uint32_t)(rnd() % 4096)); memcpy(&x, &u, 4); if (rnd() % 2) x = -x; }
        else if (mode == 2) x = same;
        else x = (float)(rnd() % 16) / 16.0f - 0.5f;      // Q4 around zero: ties within and across runs
      }
      std::sort(r.begin(), r.end(), key_less);
    }
    std::vector<SignedRun> desc;
    std::vector<float> all;
    for (auto& r : runs) { desc.push_back(SignedRun{r.data(), r.size(), 1}); all.insert(all.end(), r.begin(), r.end()); }
    // the subtracted runs: present in the set, each at most once
    std::vector<float> one_extra;
    int n_sub = 0;
    if (mode == 3) {
      // everything goes again ...                        (two runs at the most here)
      for (auto& r : runs) { desc.push_back(SignedRun{r.data(), r.size(), -1}); ++n_sub; }
      all.clear();
      // ... and in half of the cases one more element stays
      if (rnd() % 2) { one_extra.assign(1, (float)(rnd() % 16) / 16.0f - 0.5f); desc.push_back(SignedRun{one_extra.data(), 1, 1}); all.push_back(one_extra[0]); }
    } else if (n_runs) {
      n_sub = (int)(rnd() % 3);
      int a = (int)(rnd() % n_runs), b = (int)(rnd() % n_runs);
      if (n_sub == 2 && a == b) n_sub = 1;
      const int idx[2] = {a, b};
      for (int q = 0; q < n_sub; ++q) {
        desc.push_back(SignedRun{runs[idx[q]].data(), runs[idx[q]].size(), -1});
        for (float x : runs[idx[q]]) {                  // take one element with the same bits out of the materialised set
          auto it = std::find_if(all.begin(), all.end(), [&](float y) { return glia::float_ord(y) == glia::float_ord(x); });
          if (it == all.end()) { fprintf(stderr, "case %ld: the check's own bookkeeping failed\n", t); return 2; }
          *it = all.back(); all.pop_back();
        }
      }
    }
    if (n_sub) ++with_diff;
    if (all.empty()) { ++empty; continue; }             // the callers give 0 for an empty set without asking the core
    if (all.size() == 1) ++single;
    const size_t rank = all.size() / 2;
    std::nth_element(all.begin(), all.begin() + (long)rank, all.end(), key_less);
    const float want = all[rank];
    const float got = glia::median_select(glia::RunList{desc.data(), (int)desc.size()}, (long long)rank, glia::SelectAlone());
    if (glia::float_ord(got) != glia::float_ord(want)) {
      fprintf(stderr, "case %ld (mode %d, %d runs, %d subtracted, %zu elements): selected %.9g, nth_element %.9g\n", t, mode, n_runs, n_sub, all.size(), got, want);
      return 1;
    }
    ++checked;
  }
  printf("median_select_check: %ld cases agree with nth_element (%ld with subtracted runs, %ld one-element sets), %ld empty sets skipped\n", checked, with_diff, single, empty);
  return checked > 0 ? 0 : 1;
}
