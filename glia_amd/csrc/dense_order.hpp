// glia_amd/csrc/dense_order.hpp -- a merge order in region keys -> dense ids, validated on the way.  Host only, no HIP (the pattern
// of tree_paths.hpp): cli/dense_order_check.cpp runs it against a set of live keys updated merge by merge.  Dense ids: leaf i = the
// i-th label ascending, the region merge k creates = R + k (RegionMap(seg, mask, order, false), type/region_map.hxx:42-48,67-68).
#pragma once
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

}  // namespace glia
