// cli/tree_paths_check.cpp -- host-only check of the lifting primitives of the batch bc_feat route (glia_amd/csrc/tree_paths.hpp)
// against parent-pointer walks.
//   tree_paths_check [random trees] [seed]     exit 0 and one summary line when everything agrees
// Trees: a caterpillar of depth 200, a complete binary tree of 256 leaves, a forest of three trees plus leaves that are never merged,
// and random trees of at most 64 leaves (random merges among the current roots, any number of them).  Every tree gets a list of
// directed entries (a -> b, mutual or not).  Checked for every entry: the child of the join node the climb ends at, the join node,
// the number of nodes of the entry's path (a mutual entry: up to, not including, the join node; a non-mutual or never-joined one: up
// to and including the root).  Checked for every node: min and max over the entries whose EXPLICITLY enumerated path holds the node,
// against the tables T[0] after the two-block updates and the push-down sweeps.  The caterpillar and the complete tree carry every
// ordered leaf pair, so that path lengths 1, 2^j - 1, 2^j and 2^j + 1 all occur, with and without the root.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../glia_amd/csrc/tree_paths.hpp"

namespace tp = glia::tp;

static uint64_t s_state;
static uint64_t rnd() { s_state ^= s_state << 13; s_state ^= s_state >> 7; s_state ^= s_state << 17; return s_state; }

struct Entry { uint32_t a, b; bool mutual; uint32_t vmin, vmax; };
struct Counts { long trees = 0, entries = 0, nodes = 0, never_joined = 0, to_root = 0; bool len_seen[1100] = {false}; };

static bool fail(const char* what, const char* tree, long a, long b, long got, long want) {
  fprintf(stderr, "tree_paths_check: %s: %s (entry %ld -> %ld): got %ld, expected %ld\n", tree, what, a, b, got, want);
  return false;
}

// forced: [M][2] children of merge i (node R + i)
static bool check_tree(const char* name, uint32_t R, const std::vector<uint32_t>& forced, const std::vector<Entry>& entries, Counts* cnt) {
  const int64_t M = (int64_t)forced.size() / 2;
  const size_t nn = (size_t)R + (size_t)M;
  std::vector<int64_t> parent;
  std::vector<uint32_t> pos, at, lo, hi, depth, height;
  tp::tree_intervals(forced.data(), R, M, &parent, &pos, &at, &lo, &hi);
  const auto dh = tp::tree_depth_height(forced.data(), R, M, parent, &depth, &height);
  // brute depth / height
  uint32_t bd = 0, bh = 0;
  for (size_t x = 0; x < nn; ++x) {
    uint32_t d = 0;
    for (int64_t y = parent[x]; y >= 0; y = parent[y]) ++d;
    if (d != depth[x]) return fail("depth of a node", name, (long)x, -1, depth[x], d);
    bd = std::max(bd, d);
    if (x < R) { uint32_t up = 0; for (int64_t y = (int64_t)x; y >= 0; y = parent[y], ++up) if (height[y] < up) return fail("height below a leaf's distance", name, (long)x, (long)y, height[y], up); }
    bh = std::max(bh, height[x]);
  }
  if (dh.first != bd || dh.second != bh) return fail("max depth / height", name, -1, -1, dh.first, bd);
  for (int64_t i = 0; i < M; ++i)
    if (height[R + i] != 1 + std::max(height[forced[2 * i]], height[forced[2 * i + 1]])) return fail("height of a merge", name, (long)i, -1, height[R + i], -1);
  const int levels = tp::levels_for(dh.first);
  if (!((1ull << levels) > dh.first + 1ull) || (levels > 1 && (1ull << (levels - 1)) > dh.first + 1ull)) return fail("levels_for", name, -1, -1, levels, dh.first);
  std::vector<uint32_t> anc((size_t)levels * nn);
  for (size_t x = 0; x < nn; ++x) anc[x] = parent[x] < 0 ? tp::kNoNode : (uint32_t)parent[x];
  for (int j = 1; j < levels; ++j)
    for (size_t x = 0; x < nn; ++x) anc[(size_t)j * nn + x] = tp::anc_double(&anc[(size_t)(j - 1) * nn], (uint32_t)x);
  // level ancestors of every node
  for (size_t x = 0; x < nn; ++x) {
    int64_t y = (int64_t)x;
    for (uint32_t k = 0; k <= depth[x] + 1 && k < (1u << levels); ++k) {
      const uint32_t got = tp::level_ancestor(anc.data(), nn, levels, (uint32_t)x, k);
      const uint32_t want = y < 0 ? tp::kNoNode : (uint32_t)y;
      if (got != want) return fail("level ancestor", name, (long)x, (long)k, got, want);
      if (y >= 0) y = parent[y];
    }
  }
  // entries: join node, path; tables
  std::vector<uint32_t> Tmin((size_t)levels * nn, 0xFFFFFFFFu), Tmax((size_t)levels * nn, 0u), want_min(nn, 0xFFFFFFFFu), want_max(nn, 0u);
  for (const Entry& e : entries) {
    // brute force: walk up from a; is b below x?  (walk b's own ancestors)
    auto below = [&](uint32_t leaf, int64_t x) { for (int64_t y = leaf; y >= 0; y = parent[y]) if (y == x) return true; return false; };
    std::vector<uint32_t> path;
    int64_t x = e.a, join = -1, top = e.a;
    for (; x >= 0; x = parent[x]) {
      if (below(e.b, x)) { join = x; break; }
      top = x;
      path.push_back((uint32_t)x);
    }
    if (!e.mutual) for (; x >= 0; x = parent[x]) path.push_back((uint32_t)x);       // lives on to the root
    const tp::Climb c = tp::climb_below(anc.data(), nn, levels, lo.data(), hi.data(), e.a, pos[e.b]);
    if (c.top != (uint32_t)top) return fail("child of the join node", name, e.a, e.b, c.top, top);
    const uint32_t got_join = anc[c.top];
    if (got_join != (join < 0 ? tp::kNoNode : (uint32_t)join)) return fail("join node", name, e.a, e.b, got_join, join);
    if (c.steps != depth[e.a] - depth[top]) return fail("steps of the climb", name, e.a, e.b, c.steps, depth[e.a] - depth[top]);
    const uint32_t k = tp::path_nodes(e.mutual, c.steps, depth[e.a]);
    if (k != path.size()) return fail("nodes on the path", name, e.a, e.b, k, (long)path.size());
    if (k < 1100) cnt->len_seen[k] = true;
    if (join < 0) ++cnt->never_joined;
    if (parent[path.back()] < 0) ++cnt->to_root;
    for (uint32_t v : path) { want_min[v] = std::min(want_min[v], e.vmin); want_max[v] = std::max(want_max[v], e.vmax); }
    const tp::Cover cv = tp::path_cover(k);
    if (!((1u << cv.j) <= k && k < (2u << cv.j) && cv.second + (1u << cv.j) == k)) return fail("two-cover", name, e.a, e.b, cv.j, k);
    tp::path_update(anc.data(), nn, levels, e.a, k, [&](int j, uint32_t v) {
      Tmin[(size_t)j * nn + v] = std::min(Tmin[(size_t)j * nn + v], e.vmin);
      Tmax[(size_t)j * nn + v] = std::max(Tmax[(size_t)j * nn + v], e.vmax);
    });
    ++cnt->entries;
  }
  for (int j = levels - 1; j >= 1; --j)
    for (size_t v = 0; v < nn; ++v) {
      tp::push_down(anc.data(), nn, j, (uint32_t)v, [&](int jj, uint32_t y) { return Tmin[(size_t)jj * nn + y]; },
                    [&](int jj, uint32_t y, uint32_t val) { Tmin[(size_t)jj * nn + y] = std::min(Tmin[(size_t)jj * nn + y], val); });
      tp::push_down(anc.data(), nn, j, (uint32_t)v, [&](int jj, uint32_t y) { return Tmax[(size_t)jj * nn + y]; },
                    [&](int jj, uint32_t y, uint32_t val) { Tmax[(size_t)jj * nn + y] = std::max(Tmax[(size_t)jj * nn + y], val); });
    }
  for (size_t v = 0; v < nn; ++v) {
    if (Tmin[v] != want_min[v]) return fail("path minimum of a node", name, (long)v, -1, Tmin[v], want_min[v]);
    if (Tmax[v] != want_max[v]) return fail("path maximum of a node", name, (long)v, -1, Tmax[v], want_max[v]);
  }
  cnt->nodes += (long)nn;
  ++cnt->trees;
  return true;
}

static Entry make_entry(uint32_t a, uint32_t b) {
  Entry e{a, b, (rnd() % 3) != 0, 0, 0};
  e.vmin = 1 + (uint32_t)(rnd() % 1000); e.vmax = e.vmin + (uint32_t)(rnd() % 1000);     // (0 and 0xFFFFFFFF are the tables' "none")
  return e;
}
static std::vector<Entry> all_pairs(uint32_t R) {
  std::vector<Entry> v;
  for (uint32_t a = 0; a < R; ++a) for (uint32_t b = 0; b < R; ++b) if (a != b) v.push_back(make_entry(a, b));
  return v;
}
static void caterpillar(uint32_t first_leaf, uint32_t n_leaves, uint32_t R, std::vector<uint32_t>* forced) {
  uint32_t top = first_leaf;
  for (uint32_t i = 1; i < n_leaves; ++i) { forced->push_back(top); forced->push_back(first_leaf + i); top = R + (uint32_t)(forced->size() / 2) - 1; }
}
static void rounds(std::vector<uint32_t> roots, uint32_t R, std::vector<uint32_t>* forced) {
  while (roots.size() > 1) {
    std::vector<uint32_t> next;
    for (size_t i = 0; i + 1 < roots.size(); i += 2) { forced->push_back(roots[i]); forced->push_back(roots[i + 1]); next.push_back(R + (uint32_t)(forced->size() / 2) - 1); }
    if (roots.size() & 1) next.push_back(roots.back());
    roots.swap(next);
  }
}

int main(int argc, char** argv) {
  const long n_random = argc > 1 ? atol(argv[1]) : 2000;
  s_state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 0x9E3779B97F4A7C15ull;
  Counts cnt;
  {
    std::vector<uint32_t> f;
    caterpillar(0, 201, 201, &f);                        // depth 200
    if (!check_tree("caterpillar of depth 200", 201, f, all_pairs(201), &cnt)) return 1;
    std::vector<uint32_t> g;                              // the same grown from the other end: the deep leaf comes first
    g.push_back(200); g.push_back(199);
    for (uint32_t i = 2; i < 201; ++i) { g.push_back(200 - i); g.push_back(201 + i - 2); }
    if (!check_tree("caterpillar from the top", 201, g, all_pairs(201), &cnt)) return 1;
  }
  {
    std::vector<uint32_t> f, leaves(256);
    for (uint32_t i = 0; i < 256; ++i) leaves[i] = i;
    rounds(leaves, 256, &f);
    if (!check_tree("complete binary tree of 256 leaves", 256, f, all_pairs(256), &cnt)) return 1;
  }
  {
    const uint32_t R = 40;                               // leaves 30 .. 39 are never merged
    std::vector<uint32_t> f, r2, r3;
    caterpillar(0, 10, R, &f);
    for (uint32_t i = 10; i < 18; ++i) r2.push_back(i);
    rounds(r2, R, &f);
    for (uint32_t i = 18; i < 30; ++i) r3.push_back(i);
    while (r3.size() > 1) {
      const size_t i = rnd() % r3.size(); size_t j = rnd() % (r3.size() - 1); if (j >= i) ++j;
      f.push_back(r3[i]); f.push_back(r3[j]);
      r3[i] = R + (uint32_t)(f.size() / 2) - 1; r3.erase(r3.begin() + (long)j);
    }
    if (!check_tree("forest of three trees and single leaves", R, f, all_pairs(R), &cnt)) return 1;
  }
  for (long t = 0; t < n_random; ++t) {
    const uint32_t R = 2 + (uint32_t)(rnd() % 63);
    std::vector<uint32_t> f, roots(R);
    for (uint32_t i = 0; i < R; ++i) roots[i] = i;
    const uint32_t M = (rnd() % 4) ? R - 1 : (uint32_t)(rnd() % R);
    for (uint32_t m = 0; m < M; ++m) {
      // skewed picks make deep trees as often as bushy ones
      const bool deep = (t & 1) != 0;
      const size_t i = deep && m ? roots.size() - 1 : rnd() % roots.size(); size_t j = rnd() % (roots.size() - 1); if (j >= i) ++j;
      f.push_back(roots[i]); f.push_back(roots[j]);
      const uint32_t created = R + m;
      roots.erase(roots.begin() + (long)std::max(i, j)); roots.erase(roots.begin() + (long)std::min(i, j));
      roots.push_back(created);
    }
    std::vector<Entry> es;
    const size_t ne = rnd() % 200;
    for (size_t q = 0; q < ne; ++q) { const uint32_t a = (uint32_t)(rnd() % R); uint32_t b = (uint32_t)(rnd() % (R - 1)); if (b >= a) ++b; es.push_back(make_entry(a, b)); }
    if (!check_tree("random tree", R, f, es, &cnt)) { fprintf(stderr, "  (random tree %ld)\n", t); return 1; }
  }
  // the path lengths the two-cover must get right
  for (int j = 0; j <= 7; ++j)
    for (int d = -1; d <= 1; ++d) {
      const int k = (1 << j) + d;
      if (k >= 1 && k <= 200 && !cnt.len_seen[k]) { fprintf(stderr, "tree_paths_check: no path of %d nodes was exercised\n", k); return 1; }
    }
  if (!cnt.never_joined || !cnt.to_root) { fprintf(stderr, "tree_paths_check: no never-joined entry or no path that holds a root\n"); return 1; }
  printf("tree_paths_check: %ld trees, %ld nodes, %ld entries agree with parent-pointer walks (%ld never joined, %ld paths hold a root)\n", cnt.trees, cnt.nodes,
         cnt.entries, cnt.never_joined, cnt.to_root);
  return 0;
}
