// glia_amd/csrc/edge_record.hpp -- the two records of the window-queue kernels (list entry, edge record) and the rule that rebuilds an
// edge record from the entry the edge leaves in the list of its LARGER region.
//
// INVARIANT (batch kernel): a record exists iff the edge was created at or above the horizon, or has been through a baseline.  An edge
// created below the horizon (WinState::wch) is neither queued nor counted, nobody can reach it before the next baseline, and nearly all
// such edges die before one: its 64-byte record is not written.  Its two list entries are, and they hold every field of the record but
// the two `cat` bits of its seq (greedy_tree.hpp, update_seq), which go to a byte array indexed by edge slot (WinState::ecat).  The
// baseline's collection pass rebuilds the records of the survivors (greedy_baseline.hpp, win_collect_lists_kernel).
// Plain C++ as well as HIP: cli/edge_rebuild_check.cpp runs the rule on the host.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GLIA_REC_HD __host__ __device__
#else
#define GLIA_REC_HD
#endif

namespace glia {

#if defined(__HIPCC__)
typedef uint2 RecPair;
#else
struct RecPair { uint32_t x, y; };
#endif
constexpr uint32_t kRecNone = 0xFFFFFFFFu;      // == kNone (greedy_common.hpp)

// An incident-edge list entry of the window kernel: everything a contraction needs from the edge and from the
// neighbour, so that one 32-byte load replaces the second dependent round trip (edge record, neighbour's list offset).
// All of it is immutable for the lifetime of the edge / region.
struct __attribute__((aligned(16))) FatEntry {
  uint32_t eid;      // edge slot, kNone = tombstone
  uint32_t rs;       // the neighbour this entry leads to
  uint32_t n;        // boundary voxels of the edge
  uint32_t pos;      // position of the edge's other entry, in rs's list
  uint32_t off;      // adj_off[rs]
  uint32_t len;      // adj_len[rs]
  double mean;       // boundary mean of the edge
};
static_assert(sizeof(FatEntry) == 32, "FatEntry layout");

struct __attribute__((aligned(16))) EdgeRec {
  uint32_t u, v, posu, posv;                // regions (u < v) and the positions of the edge's entries in their lists
  double mean; int n; uint32_t next;        // linkage data; link of the cell list
  RecPair hu, hv;                           // (offset, length) of u's and v's incident-edge lists
  double sal; unsigned long long seq;       // queue key; seq == 0: not in the queue
};
static_assert(sizeof(EdgeRec) == 64, "EdgeRec layout");

// The record of the created edge (fe.rs, v), v = R0 + k the region merge k made, from entry number `idx` of v's list, v's list header
// (adj_off[v], adj_len[v]) and the edge's cat bits: field for field what store_new_edge writes for an edge at or above the horizon.
GLIA_REC_HD inline EdgeRec rebuild_edge_record(const FatEntry& fe, uint32_t idx, uint32_t v, uint32_t voff, uint32_t vlen, uint32_t cat, uint32_t R0) {
  EdgeRec r;
  r.u = fe.rs; r.v = v; r.posu = fe.pos; r.posv = idx;
  r.mean = fe.mean; r.n = (int)fe.n; r.next = kRecNone;
  r.hu.x = fe.off; r.hu.y = fe.len; r.hv.x = voff; r.hv.y = vlen;
  r.sal = -fe.mean;
  r.seq = ((unsigned long long)(v - R0 + 1u) << 32) | ((unsigned long long)(cat & 3u) << 30) | fe.rs;
  return r;
}

}  // namespace glia
