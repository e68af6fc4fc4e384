// cli/baseline_plan_check.cpp -- host-only check of what the pb-mean window queue decides on the host at its set-up and at every
// baseline (glia_amd/csrc/baseline_plan.hpp): saliency cells, the bits of the sort by seq, lanes and slots of the collection pass, and
// the interval and horizon of the next launch.  Every expected value below is a literal worked out by hand from the rules; none
// comes from the functions under test.
//   baseline_plan_check       exit 0 and one summary line when every case agrees
#include <cstdio>
#include "../glia_amd/csrc/baseline_plan.hpp"

using namespace glia;

static int failures = 0;
static void expect(bool ok, const char* what, int i, unsigned long long got, unsigned long long want) {
  if (!ok) { printf("baseline_plan_check: %s case %d: got %llu, expected %llu\n", what, i, got, want); ++failures; }
}

struct Baseline { uint32_t n, n_edges; long long top_cell; uint32_t wch; unsigned long long interval; };

// runs the baselines in order from the state `t`; returns how many were checked
static int run(const char* what, const BaselinePolicy& p, BaselineTrack& t, const Baseline* b, int count) {
  for (int i = 0; i < count; ++i) {
    const BaselinePlan got = plan_baseline(p, t, b[i].n, b[i].n_edges, b[i].top_cell);
    expect(got.wch == b[i].wch, what, i, got.wch, b[i].wch);
    expect(got.rebase_after == b[i].interval, what, i, got.rebase_after, b[i].interval);
  }
  return count;
}
static void expect_track(const char* what, const BaselineTrack& t, long long top, unsigned long long ne) {
  if (t.prev_top_cell != top || t.prev_ne != ne) { printf("baseline_plan_check: %s: state (%lld, %llu), expected (%lld, %llu)\n", what, t.prev_top_cell, t.prev_ne, top, ne); ++failures; }
}

int main() {
  int plans = 0, cells = 0, bits = 0, lanes = 0, slots = 0;

  // ---- interval and horizon: wB = 1024, factor 0.5, GLIA_HMT_REBASE = 300, rebase_end = 8, E0 = 6000 ----
  BaselinePolicy p;
  p.wB = 1024; p.E0 = 6000; p.horizon_factor = 0.5; p.rebase_set = true; p.rebase = 300; p.rebase_end = 8;
  {
    const Baseline seq[4] = {{6000, 6000, 1000, 0, 300},      // the first baseline: nothing to measure a descent against
                             {5800, 6300, 990, 985, 300},     // d = 10, delta = max(0.5 * 10 * 300 / 300, 1024 / 512) = 5
                             {5000, 6600, 990, 988, 300},     // d = 0: the floor of 2 cells
                             {4096, 6900, 980, 0, 37}};       // not more than 4096 items: no horizon, 300 / 8; the state stays
    BaselineTrack t;
    plans += run("run", p, t, seq, 3);
    expect_track("run, after #3", t, 990, 6600);
    plans += run("run #4", p, t, seq + 3, 1);
    expect_track("run, after #4", t, 990, 6600);
    const Baseline near0 = {5000, 6900, 1, 0, 37};            // d = 989, delta = 494.5 > 1: no room for a horizon, 300 / 8
    BaselineTrack u; u.prev_top_cell = 990; u.prev_ne = 6600;
    plans += run("top near cell 0", p, u, &near0, 1);
    expect_track("top near cell 0", u, 1, 6900);
  }
  const Baseline five[5] = {{6000, 6000, 1000, 0, 300}, {5800, 6300, 990, 985, 300}, {5000, 6600, 990, 988, 300}, {4096, 6900, 980, 0, 300}, {5000, 6900, 1, 0, 300}};
  {
    BaselinePolicy q = p; q.rebase_end = 1;                   // the same five baselines: the horizons stay, every interval is 300
    BaselineTrack t;
    plans += run("rebase_end 1", q, t, five, 4);
    BaselineTrack u; u.prev_top_cell = 990; u.prev_ne = 6600;
    plans += run("rebase_end 1, top near cell 0", q, u, five + 4, 1);
  }
  {
    BaselinePolicy q = p; q.horizon_factor = 0.0;             // the one-at-a-time kernel: no horizon, interval 300, the state is never touched
    Baseline flat[5];
    for (int i = 0; i < 5; ++i) { flat[i] = five[i]; flat[i].wch = 0; }
    BaselineTrack t;
    plans += run("factor 0", q, t, flat, 5);
    expect_track("factor 0", t, -1, 0);
  }
  {
    BaselinePolicy q = p; q.rebase_set = false;               // GLIA_HMT_REBASE unset: max(800000, n / 2)
    q.E0 = 3000000;
    const Baseline a = {1000000, 3000000, 1000, 0, 800000}, b = {2000000, 3000000, 1000, 0, 1000000};
    BaselineTrack t, u;
    plans += run("unset, n = 1 000 000", q, t, &a, 1);
    plans += run("unset, n = 2 000 000", q, u, &b, 1);
  }

  // ---- cells ----
  {
    const uint32_t c[5][2] = {{1000, 256}, {1024, 256}, {1025, 512}, {6000, 2048}, {1u << 26, 1u << 22}};
    for (int i = 0; i < 5; ++i, ++cells) expect(plan_cells(c[i][0]) == c[i][1], "cells", i, plan_cells(c[i][0]), c[i][1]);
  }
  // ---- seq bits ----
  {
    const uint32_t c[4][2] = {{1, 34}, {5, 36}, {1u << 20, 54}, {1u << 31, 64}};
    for (int i = 0; i < 4; ++i, ++bits) expect(plan_seq_bits(c[i][0]) == (int)c[i][1], "seq bits", i, (unsigned long long)plan_seq_bits(c[i][0]), c[i][1]);
  }
  // ---- lanes: R0, n_regions, n_last, forced -> lanes ----
  {
    const uint32_t c[9][5] = {{1000, 1000, 6000, 0, 16}, {1000, 1000, 12000, 0, 16},      // 2 x 12000 = 24 x 1000: equality
                              {1000, 1000, 12001, 0, 64}, {1000, 1900, 1300, 0, 64},      // 100 live regions: 2600 > 2400
                              {1000, 2000, 12, 0, 16}, {1000, 2000, 13, 0, 64},           // live_regions clamps to 1
                              {1000, 1000, 12001, 16, 16}, {1000, 1000, 6000, 64, 64},    // forced wins
                              {1000, 1000, 12001, 7, 64}};                                // a forced 7 is ignored
    for (int i = 0; i < 9; ++i, ++lanes) {
      const uint32_t got = plan_collect_lanes(c[i][0], c[i][1], c[i][2], c[i][3]);
      expect(got == c[i][4], "lanes", i, got, c[i][4]);
    }
  }
  // ---- slots: 5 per block of 256 threads, one wave for each of 2 R regions: R = 1 and 2 fill one block, R = 3 needs two ----
  {
    const unsigned long long c[4][2] = {{1, 5}, {2, 5}, {3, 10}, {1000, 2500}};
    for (int i = 0; i < 4; ++i, ++slots) expect(plan_collect_slots((uint32_t)c[i][0], 5) == c[i][1], "slots", i, plan_collect_slots((uint32_t)c[i][0], 5), c[i][1]);
    // no collection of a run outgrows them: at most 2 R regions, 16 or 64 lanes each
    for (uint32_t R = 1; R <= 300; ++R)
      for (uint32_t nr = R; nr <= 2 * R; ++nr)
        for (uint32_t g = 16; g <= 64; g += 48)
          if (plan_collect_blocks(nr, g) * 5 > plan_collect_slots(R, 5)) { printf("baseline_plan_check: R %u, %u regions, %u lanes: more blocks than slots\n", R, nr, g); ++failures; }
  }

  if (failures) return 1;
  printf("baseline_plan_check: %d plans, %d cell counts, %d seq-bit counts, %d lane choices and %d slot counts agree with the values worked out by hand\n",
         plans, cells, bits, lanes, slots);
  return 0;
}
