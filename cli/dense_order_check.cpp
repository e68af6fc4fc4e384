// cli/dense_order_check.cpp -- host-only check of the merge-order validator of bc_feat and bc_label (glia_amd/csrc/dense_order.hpp)
// against a direct model: the set of live keys, updated merge by merge, and the set of keys any region ever had.
//   dense_order_check [random orders] [seed]     exit 0 and one summary line when everything agrees
// Orders: random valid ones over 1 to 64 leaves with sparse ascending labels (any number of merges up to R - 1, operands drawn from
// the live regions, created keys above or between the labels).  Every valid order is then corrupted in each way that applies to it:
// an operand no region has, an operand that is already merged, a created key an earlier merge created, a created key that is a leaf's
// label, and n == R.  Checked: the dense pairs on success; on failure the kind and the index of the first offending merge -- both
// against the model and against what the corruption was made to provoke.
//
// Second line: leaf_truth_counts of the same header, which turns the (label, truth) table of glia_hmt_label_overlap into the (leaf,
// truth) table of bc_label, against a std::map<label, leaf> lookup per entry.  Tables over labels drawn as above, ascending by (a, b),
// whose `a` is a region label, a value below the first, between two or above the last label, or the masked label 0xFFFFFFFF; truth
// labels include 0 and 0xFFFFFFFF, so the pair (0xFFFFFFFF, 0xFFFFFFFF) that label_overlap appends last occurs too.  Checked: the
// entries kept, with their leaves; strictly ascending (leaf, truth); the sum of the counts.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <vector>

#include "../glia_amd/csrc/dense_order.hpp"
#include "../include/glia_hmt.h"      // glia_hmt_overlap_entry

using glia::DenseOrderError;
using glia::DenseOrderResult;

static uint64_t s_state;
static uint64_t rnd() { s_state ^= s_state << 13; s_state ^= s_state >> 7; s_state ^= s_state << 17; return s_state; }

// the model: walk the merges with the keys that are alive and the keys that have ever existed
static DenseOrderResult model(const std::vector<uint32_t>& labels, const std::vector<uint32_t>& order, int64_t n, std::vector<uint32_t>* dense) {
  const int64_t R = (int64_t)labels.size();
  if (n && n >= R) return {glia::kDenseOrderTooMany, std::max<int64_t>(R - 1, 0)};      // the first merge that has no two regions to join
  std::map<uint32_t, uint32_t> id;      // every key ever -> dense id
  std::set<uint32_t> live;
  for (int64_t i = 0; i < R; ++i) { id[labels[i]] = (uint32_t)i; live.insert(labels[i]); }
  dense->assign((size_t)2 * n, 0);
  for (int64_t i = 0; i < n; ++i) {
    for (int s = 0; s < 2; ++s) {
      const uint32_t k = order[3 * i + s];
      if (!live.count(k)) return {glia::kDenseOrderOperand, i};
      live.erase(k);
      (*dense)[2 * i + s] = id[k];
    }
    const uint32_t created = order[3 * i + 2];
    if (id.count(created)) return {glia::kDenseOrderReusedKey, i};
    id[created] = (uint32_t)(R + i);
    live.insert(created);
  }
  return {glia::kDenseOrderOk, -1};
}

struct Counts { long orders = 0, merges = 0, by_kind[5] = {0, 0, 0, 0, 0}; };

// sparse ascending labels, with runs of neighbours
static std::vector<uint32_t> draw_labels() {
  const uint32_t R = 1 + (uint32_t)(rnd() % 64);
  std::vector<uint32_t> labels(R);
  uint32_t next = (uint32_t)(rnd() % 5);
  for (uint32_t i = 0; i < R; ++i) { labels[i] = next; next += (rnd() % 3) ? 1 + (uint32_t)(rnd() % 1000) : 1; }
  return labels;
}

// ---- leaf_truth_counts ----
constexpr uint32_t kMasked = 0xFFFFFFFFu;                               // kMaskedLabel (hmt_internal.hpp)
struct LeafCount { uint32_t leaf, truth; unsigned long long count; };   // TruthCount (hmt_internal.hpp)
struct TableCounts { long tables = 0, entries = 0, kept = 0, kept_truth0 = 0, kept_truth_max = 0, below = 0, between = 0, above = 0, masked = 0, reserved = 0; };

static bool check_table(const std::vector<uint32_t>& labels, TableCounts* tc) {
  const size_t R = labels.size();
  auto truth = [&]() { const uint64_t k = rnd() % 8; return k == 0 ? 0u : k == 1 ? kMasked : k == 2 ? (uint32_t)rnd() : 1 + (uint32_t)(rnd() % 6); };
  std::map<std::pair<uint32_t, uint32_t>, uint64_t> table;              // ascending by (a, b), as label_overlap returns it
  auto put = [&](uint32_t a) { for (int k = 1 + (int)(rnd() % 3); k > 0; --k) table[{a, truth()}] = 1 + rnd() % (1ull << 40); };
  for (size_t i = 0; i < R; ++i) {
    if (rnd() % 3) put(labels[i]);
    if (i == 0 && labels[0] > 0 && (rnd() & 1)) put((uint32_t)(rnd() % labels[0]));                                             // below the first label
    if (i + 1 < R && labels[i + 1] - labels[i] > 1 && rnd() % 4 == 0) put(labels[i] + 1 + (uint32_t)(rnd() % (labels[i + 1] - labels[i] - 1)));   // between two
  }
  if (rnd() & 1) put(labels[R - 1] + 1 + (uint32_t)(rnd() % 100000));    // above the last label
  if (rnd() & 1) put(kMasked);                                           // masked-out voxels; with truth 0xFFFFFFFF: the reserved pair, last
  std::vector<glia_hmt_overlap_entry> entries;
  for (const auto& e : table) entries.push_back(glia_hmt_overlap_entry{e.first.first, e.first.second, e.second});
  std::map<uint32_t, uint32_t> leaf_of;
  for (size_t i = 0; i < R; ++i) leaf_of[labels[i]] = (uint32_t)i;
  std::vector<LeafCount> want, got;
  unsigned long long want_sum = 0, got_sum = 0;
  for (const auto& e : entries) {
    auto it = leaf_of.find(e.a);
    if (e.a == kMasked && e.b == kMasked) ++tc->reserved;
    else if (e.a == kMasked) ++tc->masked;
    else if (it == leaf_of.end()) ++(e.a < labels[0] ? tc->below : e.a > labels[R - 1] ? tc->above : tc->between);
    else {
      want.push_back(LeafCount{it->second, e.b, e.count});
      want_sum += e.count;
      ++tc->kept; tc->kept_truth0 += e.b == 0; tc->kept_truth_max += e.b == kMasked;
    }
  }
  ++tc->tables; tc->entries += (long)entries.size();
  glia::leaf_truth_counts(entries.data(), entries.size(), labels.data(), (int64_t)R, kMasked, &got);
  if (got.size() != want.size()) { fprintf(stderr, "dense_order_check: leaf_truth_counts keeps %zu entries, the map lookup %zu\n", got.size(), want.size()); return false; }
  for (size_t i = 0; i < got.size(); ++i) {
    if (got[i].leaf != want[i].leaf || got[i].truth != want[i].truth || got[i].count != want[i].count) {
      fprintf(stderr, "dense_order_check: leaf_truth_counts entry %zu is (%u, %u, %llu), the map lookup gives (%u, %u, %llu)\n", i, got[i].leaf, got[i].truth,
              got[i].count, want[i].leaf, want[i].truth, want[i].count);
      return false;
    }
    if (i && !(got[i - 1].leaf < got[i].leaf || (got[i - 1].leaf == got[i].leaf && got[i - 1].truth < got[i].truth))) {
      fprintf(stderr, "dense_order_check: leaf_truth_counts entry %zu is not above entry %zu in (leaf, truth)\n", i, i - 1);
      return false;
    }
    got_sum += got[i].count;
  }
  if (got_sum != want_sum) { fprintf(stderr, "dense_order_check: leaf_truth_counts sums to %llu voxels, the kept entries to %llu\n", got_sum, want_sum); return false; }
  return true;
}

// want_error < 0: whatever the model says
static bool check(const char* what, const std::vector<uint32_t>& labels, const std::vector<uint32_t>& order, int64_t n, int want_error, int64_t want_merge) {
  std::vector<uint32_t> got_dense, want_dense;
  const DenseOrderResult got = glia::dense_order(labels.data(), (int64_t)labels.size(), order.data(), n, &got_dense);
  const DenseOrderResult want = model(labels, order, n, &want_dense);
  if (got.error != want.error || got.merge != want.merge) {
    fprintf(stderr, "dense_order_check: %s (R = %zu, n = %ld): validator says kind %d at merge %ld, the model kind %d at merge %ld\n", what, labels.size(), (long)n,
            (int)got.error, (long)got.merge, (int)want.error, (long)want.merge);
    return false;
  }
  if (want_error >= 0 && ((int)got.error != want_error || got.merge != want_merge)) {
    fprintf(stderr, "dense_order_check: %s (R = %zu, n = %ld): kind %d at merge %ld, but the corruption was made for kind %d at merge %ld\n", what, labels.size(), (long)n,
            (int)got.error, (long)got.merge, want_error, (long)want_merge);
    return false;
  }
  if (got.error == glia::kDenseOrderOk && got_dense != want_dense) { fprintf(stderr, "dense_order_check: %s: dense pairs differ from the model's\n", what); return false; }
  return true;
}

int main(int argc, char** argv) {
  const long n_random = argc > 1 ? atol(argv[1]) : 2000;
  s_state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 0x9E3779B97F4A7C15ull;
  Counts cnt;
  for (long t = 0; t < n_random; ++t) {
    const std::vector<uint32_t> labels = draw_labels();
    const uint32_t R = (uint32_t)labels.size();
    const uint32_t top = labels[R - 1];
    const int64_t n = (rnd() % 3) ? (int64_t)R - 1 : (int64_t)(rnd() % R);
    std::vector<uint32_t> order, live(labels);
    std::set<uint32_t> ever(labels.begin(), labels.end());
    for (int64_t i = 0; i < n; ++i) {
      const size_t a = rnd() % live.size(); size_t b = rnd() % (live.size() - 1); if (b >= a) ++b;
      uint32_t created;
      do created = (rnd() & 1) ? top + 1 + (uint32_t)(rnd() % 4096) : (uint32_t)(rnd() % (top + 1)); while (ever.count(created));      // above | between the labels
      order.insert(order.end(), {live[a], live[b], created});
      live.erase(live.begin() + (long)std::max(a, b)); live.erase(live.begin() + (long)std::min(a, b));
      live.push_back(created); ever.insert(created);
    }
    if (!check("valid order", labels, order, n, glia::kDenseOrderOk, -1)) return 1;
    ++cnt.orders; cnt.merges += n;
    uint32_t never;
    do never = (uint32_t)rnd(); while (ever.count(never));
    if (n >= 1) {      // an operand no region has
      std::vector<uint32_t> o(order);
      const int64_t m = (int64_t)(rnd() % n);
      o[3 * m + (rnd() & 1)] = never;
      if (!check("unknown region", labels, o, n, glia::kDenseOrderOperand, m)) return 1;
      ++cnt.by_kind[0];
    }
    if (n >= 2) {      // an operand an earlier merge took | a created key an earlier merge created
      std::vector<uint32_t> o(order);
      const int64_t m = 1 + (int64_t)(rnd() % (n - 1)), j = (int64_t)(rnd() % m);
      o[3 * m + (rnd() & 1)] = order[3 * j + (rnd() & 1)];
      if (!check("already merged", labels, o, n, glia::kDenseOrderOperand, m)) return 1;
      ++cnt.by_kind[1];
      o = order;
      o[3 * m + 2] = order[3 * j + 2];
      if (!check("reused created key", labels, o, n, glia::kDenseOrderReusedKey, m)) return 1;
      ++cnt.by_kind[2];
    }
    if (n >= 1) {      // a created key that is a leaf's label (merged by then or not)
      std::vector<uint32_t> o(order);
      const int64_t m = (int64_t)(rnd() % n);
      o[3 * m + 2] = labels[rnd() % R];
      if (!check("created key = a leaf", labels, o, n, glia::kDenseOrderReusedKey, m)) return 1;
      ++cnt.by_kind[3];
    }
    {                  // as many merges as regions: refused before any merge is looked at
      std::vector<uint32_t> o(order);
      o.resize((size_t)3 * R, never);
      if (!check("n == R", labels, o, (int64_t)R, glia::kDenseOrderTooMany, (int64_t)R - 1)) return 1;
      ++cnt.by_kind[4];
    }
  }
  // no regions, no merges; and merges without regions
  if (!check("empty", {}, {}, 0, glia::kDenseOrderOk, -1) || !check("no regions", {}, {1, 2, 3}, 1, glia::kDenseOrderTooMany, 0)) return 1;
  for (int k = 0; k < 5; ++k) if (n_random >= 100 && !cnt.by_kind[k]) { fprintf(stderr, "dense_order_check: corruption %d was never exercised\n", k); return 1; }
  printf("dense_order_check: %ld orders, %ld merges agree with the live-key model; corrupted: %ld unknown, %ld merged, %ld reused, %ld leaf key, %ld too many\n", cnt.orders,
         cnt.merges, cnt.by_kind[0], cnt.by_kind[1], cnt.by_kind[2], cnt.by_kind[3], cnt.by_kind[4]);
  TableCounts tc;
  for (long t = 0; t < n_random; ++t) if (!check_table(draw_labels(), &tc)) return 1;
  std::vector<LeafCount> none{LeafCount{1, 2, 3}};
  glia::leaf_truth_counts((const glia_hmt_overlap_entry*)nullptr, 0, (const uint32_t*)nullptr, 0, kMasked, &none);      // no entries, no regions
  if (!none.empty()) { fprintf(stderr, "dense_order_check: leaf_truth_counts of an empty table is not empty\n"); return 1; }
  printf("leaf_truth_counts: %ld tables, %ld entries agree with the map lookup; kept: %ld (%ld with truth 0, %ld with truth 0xFFFFFFFF); dropped: %ld below, "
         "%ld between, %ld above the labels, %ld masked, %ld reserved pair\n", tc.tables, tc.entries, tc.kept, tc.kept_truth0, tc.kept_truth_max, tc.below, tc.between,
         tc.above, tc.masked, tc.reserved);
  return 0;
}
