// cli/dense_order_check.cpp -- host-only check of the merge-order validator of bc_feat and bc_label (glia_amd/csrc/dense_order.hpp)
// against a direct model: the set of live keys, updated merge by merge, and the set of keys any region ever had.
//   dense_order_check [random orders] [seed]     exit 0 and one summary line when everything agrees
// Orders: random valid ones over 1 to 64 leaves with sparse ascending labels (any number of merges up to R - 1, operands drawn from
// the live regions, created keys above or between the labels).  Every valid order is then corrupted in each way that applies to it:
// an operand no region has, an operand that is already merged, a created key an earlier merge created, a created key that is a leaf's
// label, and n == R.  Checked: the dense pairs on success; on failure the kind and the index of the first offending merge -- both
// against the model and against what the corruption was made to provoke.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <vector>

#include "../glia_amd/csrc/dense_order.hpp"

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
    const uint32_t R = 1 + (uint32_t)(rnd() % 64);
    std::vector<uint32_t> labels(R);
    uint32_t next = (uint32_t)(rnd() % 5);
    for (uint32_t i = 0; i < R; ++i) { labels[i] = next; next += (rnd() % 3) ? 1 + (uint32_t)(rnd() % 1000) : 1; }      // sparse, with runs of neighbours
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
  return 0;
}
