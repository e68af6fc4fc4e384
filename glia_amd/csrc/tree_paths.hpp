// glia_amd/csrc/tree_paths.hpp -- a KNOWN merge tree as tables, and updates along ancestor paths of it without walking them.
//
// bc_feat is given its merge order (hmt/main_bc_feat.cxx:27-112), so the tree exists before any statistic is combined: leaves
// 0 .. R-1, merge i creates node R + i from forced[2 i] and forced[2 i + 1].  Every directed boundary entry (a -> b) of the region
// map belongs to the boundary sets of the nodes on a PATH that starts at leaf a and runs upwards (TRegion::merge,
// type/region.hxx:66-75): a mutual entry up to, not including, the node that joins a and b; a non-mutual one up to and including the
// root.  Walking these paths costs O(entries x depth), and a pb-mean tree of 262 144 regions is thousands of levels deep.  Here:
//   * tree tables (host, O(R + M)): parent, depth-first leaf positions, the interval [lo, hi) of positions under a node, depth and
//     height -- shared with the host walk of median_feats.hip;
//   * ancestor tables anc[j][v] = the 2^j-th ancestor of v (kNoNode past a root), built by doubling;
//   * the join-node climb: from leaf a, jump by 2^j from the highest j down while the ancestor's interval does not hold pos(b).  It
//     ends at the child of the join node on a's side, after a known number of steps;
//   * the two-cover of a path: tables T[j][v] mean "applies to v and its next 2^j - 1 ancestors".  A path of k >= 1 nodes from a is
//     the union of two such blocks with j = floor(log2 k): the one at a and the one at a's (k - 2^j)-th ancestor;
//   * the push-down T[j] -> T[j - 1]: the block at v is the block of half the length at v and the one at v's 2^(j-1)-th ancestor.
// Plain C++ as well as HIP (the pattern of median_select.hpp): cli/tree_paths_check.cpp runs all of it on the host against
// parent-pointer walks.  The update operation is the caller's (a functor): integer min / max here, atomics on the device.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <utility>
#include <vector>

#include "median_select.hpp"   // GLIA_HD

namespace glia {
namespace tp {

constexpr uint32_t kNoNode = 0xFFFFFFFFu;

// table levels for paths of up to max_depth + 1 nodes (a leaf of that depth up to and including its root): the smallest L >= 1 with
// 2^L > max_depth + 1, so that floor(log2 k) < L for every path length k and every jump of a climb is below 2^L
GLIA_HD inline int levels_for(uint32_t max_depth) {
  int l = 1;
  while (l < 32 && (((unsigned long long)max_depth + 1) >> l) != 0) ++l;
  return l;
}
// one doubling step: anc[j][v] from anc[j - 1]
GLIA_HD inline uint32_t anc_double(const uint32_t* prev, uint32_t v) {
  const uint32_t u = prev[v];
  return u == kNoNode ? kNoNode : prev[u];
}
// the k-th ancestor of v (k = 0: v itself); kNoNode when the path leaves the tree.  k < 2^levels.
GLIA_HD inline uint32_t level_ancestor(const uint32_t* anc, size_t nn, int levels, uint32_t v, uint32_t k) {
  for (int j = 0; j < levels && v != kNoNode; ++j)
    if ((k >> j) & 1u) v = anc[(size_t)j * nn + v];
  return v;
}
// From leaf a towards the leaf at depth-first position pos_b (not under a): the highest ancestor-or-self of a whose interval does NOT
// hold pos_b, and the steps taken to reach it.  The join node of the two leaves is its parent (kNoNode: they are never joined).
struct Climb { uint32_t top, steps; };
GLIA_HD inline Climb climb_below(const uint32_t* anc, size_t nn, int levels, const uint32_t* lo, const uint32_t* hi, uint32_t a, uint32_t pos_b) {
  Climb c{a, 0};
  for (int j = levels - 1; j >= 0; --j) {
    const uint32_t y = anc[(size_t)j * nn + c.top];
    if (y != kNoNode && !(lo[y] <= pos_b && pos_b < hi[y])) { c.top = y; c.steps += 1u << j; }
  }
  return c;
}
// nodes on the path of a directed entry that starts at a leaf of depth `depth` (its distance from the root) and climbed `steps`
// nodes to the child of the join node: a mutual entry dies at the join node, a non-mutual one (and one never joined, for which the
// climb ends at the root) lives on to the root
GLIA_HD inline uint32_t path_nodes(bool mutual, uint32_t steps, uint32_t depth) { return mutual ? steps + 1 : depth + 1; }

// the two blocks that cover a path of k >= 1 nodes: both of 2^j nodes, the second one starts `second` nodes above the first
struct Cover { int j; uint32_t second; };
GLIA_HD inline Cover path_cover(uint32_t k) {
  const int j = 31 - __builtin_clz(k);
  return Cover{j, k - (1u << j)};
}
// upd(j, node): file the caller's value in T[j] at `node`, for the path of k nodes from a
template <class Upd>
GLIA_HD inline void path_update(const uint32_t* anc, size_t nn, int levels, uint32_t a, uint32_t k, Upd upd) {
  if (k == 0) return;
  const Cover c = path_cover(k);
  upd(c.j, a);
  const uint32_t u = level_ancestor(anc, nn, levels, a, c.second);
  if (u != kNoNode && u != a) upd(c.j, u);
}
// one node's share of the sweep T[j] -> T[j - 1] (j >= 1): get(j, v) reads, upd(j - 1, node, value) combines
template <class Get, class Upd>
GLIA_HD inline void push_down(const uint32_t* anc, size_t nn, int j, uint32_t v, Get get, Upd upd) {
  const auto val = get(j, v);
  upd(j - 1, v, val);
  const uint32_t u = anc[(size_t)(j - 1) * nn + v];
  if (u != kNoNode) upd(j - 1, u, val);
}

// ---- the tree tables (host, O(R + M)) ----
// parent (-1 at a root); depth-first positions of the leaves (pos), the leaf at a position (at), the interval [lo, hi) of positions
// under every node.  forced: [M][2] dense children, each created before the merge that takes it.
inline void tree_intervals(const uint32_t* forced, uint32_t R, int64_t M, std::vector<int64_t>* parent_o, std::vector<uint32_t>* pos_o,
                           std::vector<uint32_t>* at_o, std::vector<uint32_t>* lo_o, std::vector<uint32_t>* hi_o) {
  const size_t nn = (size_t)R + (size_t)M;
  std::vector<int64_t>& parent = *parent_o;
  std::vector<uint32_t>&pos = *pos_o, &at = *at_o, &lo = *lo_o, &hi = *hi_o;
  parent.assign(nn, -1);
  for (int64_t i = 0; i < M; ++i) { parent[forced[2 * i]] = (int64_t)R + i; parent[forced[2 * i + 1]] = (int64_t)R + i; }
  pos.assign(R, 0); at.assign(R, 0); lo.assign(nn, 0); hi.assign(nn, 0);
  uint32_t next = 0;
  std::vector<std::pair<size_t, int>> stack;
  for (size_t root = nn; root-- > 0;) {                        // (any order of the roots will do)
    if (parent[root] >= 0) continue;
    stack.push_back({root, 0});
    while (!stack.empty()) {
      auto& top = stack.back();
      const size_t x = top.first;
      if (x < R) { pos[x] = next; at[next] = (uint32_t)x; lo[x] = next; hi[x] = ++next; stack.pop_back(); continue; }
      if (top.second == 0) { lo[x] = next; top.second = 1; stack.push_back({forced[2 * (x - R)], 0}); continue; }
      if (top.second == 1) { top.second = 2; stack.push_back({forced[2 * (x - R) + 1], 0}); continue; }
      hi[x] = next; stack.pop_back();
    }
  }
}
// depth (distance from the root of its tree) and height (longest way down to a leaf) of every node; returns {max depth, max height}
inline std::pair<uint32_t, uint32_t> tree_depth_height(const uint32_t* forced, uint32_t R, int64_t M, const std::vector<int64_t>& parent,
                                                        std::vector<uint32_t>* depth_o, std::vector<uint32_t>* height_o) {
  const size_t nn = (size_t)R + (size_t)M;
  std::vector<uint32_t>&depth = *depth_o, &height = *height_o;
  depth.assign(nn, 0); height.assign(nn, 0);
  uint32_t max_d = 0, max_h = 0;
  for (int64_t i = 0; i < M; ++i) {                            // children come before their parent
    const uint32_t h = 1 + (height[forced[2 * i]] > height[forced[2 * i + 1]] ? height[forced[2 * i]] : height[forced[2 * i + 1]]);
    height[(size_t)R + i] = h;
    if (h > max_h) max_h = h;
  }
  for (size_t x = nn; x-- > 0;) {                              // a parent comes after its children
    if (parent[x] >= 0) depth[x] = depth[(size_t)parent[x]] + 1;
    if (depth[x] > max_d) max_d = depth[x];
  }
  return {max_d, max_h};
}

}  // namespace tp
}  // namespace glia
