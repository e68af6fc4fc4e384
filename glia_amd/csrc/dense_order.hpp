// glia_amd/csrc/dense_order.hpp -- a merge order in region keys -> dense ids, validated on the way.  Host only, no HIP (the pattern
// of tree_paths.hpp): cli/dense_order_check.cpp runs it against a set of live keys updated merge by merge.  Dense ids: leaf i = the
// i-th label ascending, the region merge k creates = R + k (RegionMap(seg, mask, order, false), type/region_map.hxx:42-48,67-68).
// leaf_truth_counts, below, applies the same leaf numbering to a contingency table (bc_label); the same program checks it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <unordered_map>
#include <vector>

namespace glia {

// a merge joins a key that is unknown or already merged | creates a key that a leaf or an earlier merge has | n >= R (checked first)
enum DenseOrderError { kDenseOrderOk = 0, kDenseOrderOperand, kDenseOrderReusedKey, kDenseOrderTooMany };
struct DenseOrderResult { DenseOrderError error; int64_t merge; };      // merge: the first offending one (too many: the first without regions to join, R - 1)

// labels [R] ascending, order [n][3] = (key, key, created key); *dense = [n][2] on success
inline DenseOrderResult dense_order(const uint32_t* labels, int64_t R, const uint32_t* order, int64_t n, std::vector<uint32_t>* dense) {
  if (n && n >= R) return {kDenseOrderTooMany, R > 0 ? R - 1 : 0};
  std::unordered_map<uint32_t, uint32_t> id;
  id.reserve((size_t)R * 2);
  for (int64_t i = 0; i < R; ++i) id[labels[i]] = (uint32_t)i;
  dense->assign((size_t)2 * n, 0);
  std::vector<uint8_t> used((size_t)R + n, 0);
  for (int64_t i = 0; i < n; ++i) {
    for (int s = 0; s < 2; ++s) {
      auto it = id.find(order[3 * i + s]);
      if (it == id.end() || used[it->second]) return {kDenseOrderOperand, i};
      used[it->second] = 1;
      (*dense)[2 * i + s] = it->second;
    }
    if (id.count(order[3 * i + 2])) return {kDenseOrderReusedKey, i};
    id[order[3 * i + 2]] = (uint32_t)(R + i);
  }
  return {kDenseOrderOk, -1};
}

// The contingency table of (label volume, truth volume) -> the table of bc_label.  entries [n]: (a, b, count) ascending by (a, b), as
// label_overlap returns them; labels [R] ascending; *out = (leaf, truth, count) with leaf = the index of a in labels, ascending by
// (leaf, truth) -- the order of the entries, so one cursor walks the labels and nothing is sorted or searched.  Dropped: a == masked
// (a masked-out voxel is in no region, util/struct.hxx:86-91; with masked = 0xFFFFFFFF this is also the pair (0xFFFFFFFF, 0xFFFFFFFF)
// that label_overlap appends last), and an `a` that is no region's label.  Truth 0 stays: it makes the region's size.
template <class Entry, class Count>
inline void leaf_truth_counts(const Entry* entries, size_t n, const uint32_t* labels, int64_t R, uint32_t masked, std::vector<Count>* out) {
  out->clear();
  int64_t leaf = 0;
  for (size_t i = 0; i < n; ++i) {
    const uint32_t a = entries[i].a;
    if (a == masked) continue;
    while (leaf < R && labels[leaf] < a) ++leaf;
    if (leaf < R && labels[leaf] == a) out->push_back(Count{(uint32_t)leaf, entries[i].b, entries[i].count});
  }
}

}  // namespace glia
