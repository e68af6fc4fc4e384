// glia_amd/csrc/baseline_plan.hpp -- what the pb-mean window queue decides on the host, from a handful of integers, when it is set up
// and at every baseline (greedy_baseline.hpp, WinBaseline): the number of saliency cells, the bits the sort by seq looks at, the
// lanes per list and the slots of the collection pass, and the interval and horizon of the next launch.
// Plain C++, no HIP: cli/baseline_plan_check.cpp runs the rules on the host against values worked out by hand.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>

namespace glia {

// saliency cells for E0 initial edges: ~4 initial edges per cell on average -- 256, doubled while below E0 / 4 (the exact quotient:
// 1025 edges get 512 cells) and below 2^22
inline uint32_t plan_cells(uint32_t E0) {
  uint32_t B = 256;
  while (4ull * B < E0 && B < (1u << 22)) B <<= 1;
  return B;
}

// a seq is (merge + 1) << 32 | cat << 30 | region, merge < R: 32 + bits of R + 1, the sort by seq looks at no bit above
inline int plan_seq_bits(uint32_t R) {
  int bits = 33;
  while (bits < 63 && ((unsigned long long)R >> (bits - 32)) != 0) ++bits;
  return bits + 1;
}

// Lanes per region of the collection pass's list walk: 16 while the lists are short, from numbers the host holds -- the live edges
// of the last collection (at the start: the initial edges), each in two lists, over the regions that are left (n_regions - R0 merges
// so far).  A forced 16 or 64 wins (tests).
inline uint32_t plan_collect_lanes(uint32_t R0, uint32_t n_regions, uint32_t n_last, uint32_t forced) {
  const unsigned long long live_regions = 2ull * R0 > n_regions ? 2ull * R0 - n_regions : 1ull;
  return forced == 16u || forced == 64u ? forced : 2ull * n_last <= 24ull * live_regions ? 16u : 64u;
}

// blocks of 256 threads of the collection pass over n_regions regions, and its slots for a run of R initial regions: slots_per_block
// per block, at most one wave for each of the 2 R regions there can be
inline unsigned long long plan_collect_blocks(unsigned long long n_regions, uint32_t lanes) { return (n_regions * lanes + 255ull) / 256ull; }
inline size_t plan_collect_slots(uint32_t R, uint32_t slots_per_block) { return (size_t)plan_collect_blocks(2ull * R, 64u) * slots_per_block; }

// ---- the interval (created edges until the next baseline) and the horizon (WinState::wch) of the launch behind a baseline ----
struct BaselinePolicy {                      // fixed for a run
  uint32_t wB = 0, E0 = 0;                   // saliency cells, initial edges
  double horizon_factor = 0.0;               // 0 = no horizon (set for the batch kernel)
  bool rebase_set = false;                   // GLIA_HMT_REBASE: created edges between baselines (tuning)
  unsigned long long rebase = 0;
  // GLIA_HMT_REBASE_END: an interval without a horizon in a run that has placed horizons is this many times shorter (1 = as long as
  // any).  Swept at 1024^3: 1 / 2 / 4 / 8 / 16 / 32 = 727.1 / 716.2 / 714.2 / 713.2 / 714.8 / 719.1 ms of merge loop
  unsigned long long rebase_end = 8;
};
struct BaselineTrack { long long prev_top_cell = -1; unsigned long long prev_ne = 0; };      // the last baseline of more than 4096 items
struct BaselinePlan { unsigned long long rebase_after; uint32_t wch; };

// a baseline of n items over the first n_edges edges whose largest key lies in top_cell
inline BaselinePlan plan_baseline(const BaselinePolicy& p, BaselineTrack& t, uint32_t n, uint32_t n_edges, long long top_cell) {
  BaselinePlan out;
  out.rebase_after = p.rebase_set ? p.rebase : std::max<unsigned long long>(800000ull, (unsigned long long)n / 2ull);
  // the horizon: the top of the queue sank by d cells while the last interval's edges were created; the next interval is given
  // horizon_factor times that (scaled to its planned length; at least 1/512 of the cells) before a reload would run into the horizon
  out.wch = 0;
  if (p.horizon_factor > 0.0 && n > 4096) {
    if (t.prev_top_cell >= 0 && n_edges > t.prev_ne) {
      const double d = (double)std::max<long long>(0, t.prev_top_cell - top_cell);
      const double delta = std::max(p.horizon_factor * d * (double)out.rebase_after / (double)(n_edges - t.prev_ne), (double)p.wB / 512.0);
      out.wch = (double)top_cell > delta ? (uint32_t)((double)top_cell - delta) : 0u;
    }
    t.prev_top_cell = top_cell; t.prev_ne = n_edges;
  }
  // a run that placed horizons and is left without one -- no room (the top has come within delta of cell 0) or, what ends a
  // 1024^3 run, too few items (n <= 4096): every created edge now gets its record, its list push and its count, nearly all die
  // at the next contraction of the same hub, and the cell lists keep them until a baseline drops them.  The interval, tuned for
  // 90 % of the created edges staying out of the lists, is cut by rebase_end
  if (p.horizon_factor > 0.0 && t.prev_top_cell >= 0 && n_edges > p.E0 && out.wch == 0) out.rebase_after = std::max<unsigned long long>(1ull, out.rebase_after / p.rebase_end);
  return out;
}

}  // namespace glia
