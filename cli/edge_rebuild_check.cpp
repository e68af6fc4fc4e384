// cli/edge_rebuild_check.cpp -- host-only check of the rule that rebuilds an edge record of the window queue from a list entry
// (glia_amd/csrc/edge_record.hpp, rebuild_edge_record).  A hand-made graph of five regions is laid out the way adj_fill_fat lays out
// the initial lists (offsets = exclusive scan of the degrees, entries in edge order); every edge (u, v), u < v, is then taken for the
// edge (rs = u, r2 = v) that merge k = v - R0 created, and the record rebuilt from the entry in v's list is compared, byte for byte,
// with the sixteen words store_new_edge writes for such an edge.
//   edge_rebuild_check        exit 0 and one summary line when every record agrees
#include <cstdio>
#include <cstring>
#include <vector>
#include "../glia_amd/csrc/edge_record.hpp"

using namespace glia;

int main() {
  const uint32_t R = 5, R0 = 1;
  struct E { uint32_t u, v, n; double mean; uint32_t r0; bool h0; };
  // (r0, h0): the smaller region of the contracted pair and whether the (r0, rs) edge existed -- they decide the cat bits of the seq
  const std::vector<E> edges = {{0, 1, 7, 0.125, 1, true},  {0, 2, 3, 0.5, 0, true},       {1, 2, 11, 0.33203125, 0, false}, {1, 3, 1, 0.0, 2, true},
                                {2, 3, 40, 0.99609375, 1, false}, {0, 4, 5, 0.25, 3, true}, {2, 4, 9, 0.7421875, 2, true},    {3, 4, 2, 0.00390625, 1, true}};
  std::vector<uint32_t> deg(R, 0), off(R, 0), cur(R, 0);
  for (const E& e : edges) { ++deg[e.u]; ++deg[e.v]; }
  for (uint32_t r = 1; r < R; ++r) off[r] = off[r - 1] + deg[r - 1];
  std::vector<FatEntry> pool(2 * edges.size());
  std::vector<uint32_t> posu(edges.size()), posv(edges.size());
  for (size_t e = 0; e < edges.size(); ++e) {                        // adj_fill_fat, one edge after the other
    const E& g = edges[e];
    const uint32_t pu = cur[g.u]++, pv = cur[g.v]++;
    FatEntry a; a.eid = (uint32_t)e; a.rs = g.v; a.n = g.n; a.pos = pv; a.off = off[g.v]; a.len = deg[g.v]; a.mean = g.mean;
    FatEntry b = a; b.rs = g.u; b.pos = pu; b.off = off[g.u]; b.len = deg[g.u];
    pool[off[g.u] + pu] = a; pool[off[g.v] + pv] = b;
    posu[e] = pu; posv[e] = pv;
  }
  int checked = 0, cats[3] = {0, 0, 0};
  for (uint32_t v = 0; v < R; ++v) {
    for (uint32_t i = 0; i < deg[v]; ++i) {
      const FatEntry& fe = pool[off[v] + i];
      if (fe.eid == kRecNone || !(fe.rs < v)) continue;              // every edge once, from the list of its larger region
      const E& g = edges[fe.eid];
      // store_new_edge(newE, rs, r2, posRs, idx, first, second, sal = -first, seq, offRs, lenRs, r2off, lenR2)
      const uint32_t rs = g.u, r2 = g.v, k = r2 - R0;
      const uint32_t cat = rs < g.r0 ? 0u : (g.h0 ? 1u : 2u);        // update_seq
      const unsigned long long seq = ((unsigned long long)(k + 1u) << 32) | ((unsigned long long)cat << 30) | rs;
      const double first = g.mean, sal = -first;
      unsigned long long mb, sb;
      memcpy(&mb, &first, 8); memcpy(&sb, &sal, 8);
      const uint32_t want[16] = {rs, r2, posu[fe.eid], posv[fe.eid], (uint32_t)mb, (uint32_t)(mb >> 32), g.n, kRecNone,
                                 off[rs], deg[rs], off[r2], deg[r2], (uint32_t)sb, (uint32_t)(sb >> 32), (uint32_t)seq, (uint32_t)(seq >> 32)};
      const EdgeRec got = rebuild_edge_record(fe, i, v, off[v], deg[v], (uint32_t)((seq >> 30) & 3u), R0);
      if (memcmp(&got, want, 64) != 0) {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(&got);
        printf("edge_rebuild_check: edge %u (%u, %u) differs:", fe.eid, rs, r2);
        for (int j = 0; j < 16; ++j) printf(" %08x/%08x", w[j], want[j]);
        printf("\n");
        return 1;
      }
      ++checked; ++cats[cat];
    }
  }
  if (checked != (int)edges.size() || !cats[0] || !cats[1] || !cats[2]) { printf("edge_rebuild_check: %d of %zu edges visited\n", checked, edges.size()); return 1; }
  printf("edge_rebuild_check: %d records rebuilt from list entries agree with the stored form (cat 0/1/2: %d/%d/%d)\n", checked, cats[0], cats[1], cats[2]);
  return 0;
}
