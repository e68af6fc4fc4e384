// glia_amd/csrc/greedy_window.hpp -- the window queue of the pb-mean loop and its one-at-a-time kernel (greedy_window_kernel<COND>:
// pre_merge and the GLIA_HMT_PB_BATCH=0 parity gate).  Part of greedy.hip's translation unit.
//
// What the code below relies on (the long comment in front of EdgeRec describes the queue itself):
//   * seq == 0 means "not in the queue", in an edge record (EdgeRec::seq) and in a window slot (WinShared::seq: a hole).  A record's
//     seq is cleared when the edge is popped, replaced or rejected; a dead baseline entry's seq survives only in isort_seq.
//   * w.n (slots in use) is raised by atomicAdd of any thread in a build / commit phase and rewritten by thread 0 in win_compact,
//     win_flush, win_evict and win_reload.  A decision that guards a barrier is taken on a copy read in FRONT of the barrier that
//     precedes those atomics (wn_now, wn_round, win_compact's return value), never on a second read.
//   * Cell counts (wcnt) are upper bounds of the live items of a cell below tau: a reload walks a list whenever its count is not
//     zero and resets a count that turns out too high; the batch paths never discount a tie with tau (win_retire_edge).
//   * Global stores of a contraction are fire-and-forget; whoever reads them from another wave does so behind a full_barrier().
//   * A record exists iff the edge was created at or above the horizon, or has been through a baseline (edge_record.hpp): the batch
//     kernel writes none for an edge below the horizon (store_new_edge<true>), and nothing reads one before the next baseline -- the
//     kovf look-up and win_take only see window or list items, which lie at or above the horizon; win_take_initial only sees baseline
//     members.  Record slots of such edges that die are never touched.
//   * A launch behind a baseline starts with tau at the END of the cell of the baseline's largest key (CTRL_CTHR = that cell, tsal = +inf,
//     tseq = ~0: WinBaseline::rebaseline, greedy_baseline.hpp), not of the last cell.  It is the same state: nothing alive lies above it -- the baseline
//     holds every live item, all in cells <= cthr, none above (cthr, +inf, ~0) -- and the window is empty either way.  An item CREATED
//     above it is a window item under both thresholds' rule (win_above: cell > cthr; win_queue_edge<BATCH> spills to the list and raises
//     tau if the window is full); with the last cell as threshold it went to its cell's list, and the first reload brought it back.
//     The readers of w.cthr only compare cells with it: win_above, win_retire_edge (a baseline member dies below or in tau's cell with
//     dsal < +inf: discounted from its cell, as before), win_queue_edge, win_reload (c_hi = cthr + 1: the first block of cells starts at
//     the top occupied one instead of 512 cells per step below wB), win_flush / win_evict (raise tau to the cells they push to).  The
//     horizon relation holds: wch <= the top cell whenever a horizon is placed, so tau's cell is at least wch - 1.  No live item: wB - 1.
//   * k / ne / pool_used are private copies in every thread (see greedy_tree.hpp); s.newcount is read by all behind a barrier and
//     cleared by thread 0 only behind the next one.  Audit table: DESIGN 3.3; tags [B:..] barrier, [R:..] read, [W:..] rewrite.
#pragma once
#include "greedy_tree.hpp"
#include "edge_record.hpp"       // FatEntry (list entry), EdgeRec (edge record) and the rule that rebuilds the one from the other

namespace glia {
namespace {

// =====================================================================================================================
// The window queue: the priority queue of the pb-mean loop without a tree.
//
// The tournament tree above costs a contraction ~13 k of its ~24 k cycles: every new or dying edge dirties a 256-ary
// node somewhere in the slot space, each dirty node is a 4 KB gather, and three levels are three dependent round trips
// (plus two for the pop).  The queue only ever has to answer "largest (saliency, seq)", and popped saliencies fall
// (almost) monotonically, so the live items are kept in two places instead:
//   * GLOBAL, below a threshold key tau:
//       - the INITIAL edges in one array sorted by descending key (rocPRIM, once): consumed front to back by a pointer,
//         whatever the ties (a 1024^3 Q8 volume has tie groups of thousands of equal means);
//       - edges CREATED by contractions in singly linked lists, one per saliency CELL (a monotone quantisation of the
//         saliency, ~E0/4 cells).  Insert = atomicExch on the cell head + one store, nobody waits for it.
//       A per-cell counter holds the live items of both kinds; a dying edge only decrements it (dead array entries and
//       list nodes are skipped when their cell is loaded).
//   * LDS WINDOW, above tau: unordered, <= kWinCap entries carrying (saliency, seq, edge, both regions and their list
//     headers).  Its maximum is the maximum of the queue; it is found by one scan of the window per contraction, which
//     also applies the (rare) deaths of window items.  New edges above tau go straight into the window.  When the window
//     runs empty, tau moves down: whole cells while they fit, then a prefix of the next cell's sorted initial entries
//     (tau = key of the first entry left behind) plus that cell's list nodes above tau.
// Exactness: the order is (saliency, seq) with the very seq numbers of the tree kernel, so the result is bit-identical
// (gate: SHA-1 of the whole 1024^3 order, tools/pb_bench.py); no assumption about the linkage is made (a new edge may
// well beat the current maximum: it lands in the window).  A cell whose LIST part alone exceeds the window (massive
// exact ties among created edges) stops the kernel with ST_NEED_TREE and the host continues with the tree kernel from
// the same state (edge records are unpacked into its arrays).
// With the fat list entries (FatEntry) and the list headers carried in the window a contraction is ONE dependent global
// round trip -- the two incident-edge lists -- plus LDS work; its stores are fire-and-forget: the next contraction only
// waits for them when it touches a region whose list they rewrite (a bitmap of the touched regions decides).
// Edge state is one 64-byte record (EdgeRec, edge_record.hpp) instead of twelve arrays: four wide stores per new edge, one base
// pointer -- and none at all for an edge the batch kernel creates below its horizon (see WinState::wch).
// =====================================================================================================================
static_assert(kRecNone == kNone, "edge_record.hpp");
struct WinState {
  EdgeRec* er; FatEntry* fpool;
  uint32_t* whead;                          // [wB] newest created edge of the cell's list (kNone = empty); atomics only
  uint32_t* wcnt;                           // [wB] live queue items of the cell below the threshold (sorted array + list); atomics only
  // the BASELINE: every queue item that was alive when it was taken (at the start: the initial edges; later: see
  // win_rebaseline), sorted by descending (saliency, seq), with its seq (a dead item's record no longer has it)
  const uint32_t* isort; const unsigned long long* isort_seq;
  const uint32_t* ige;                      // [wB + 1] baseline items whose cell is >= c
  const double* wrange;                     // [0] smallest initial saliency, [1] cells per unit of saliency
  uint32_t* order; double* sal_out; unsigned long long* ctrl;
  unsigned long long* rsz; double* rsum; uint32_t *mark0, *mark1, *adj_off, *adj_len;
  unsigned long long pool_cap, max_iters, cond_t0, cond_t1;
  double cond_rpb;
  uint32_t R0, Ecap, wB, nsort;             // nsort: items of the baseline
  unsigned long long ne_base, rebase_after; // edges that existed at the baseline; a new one is due after this many more
  uint32_t wcap, wbudget;                   // window slots in use (<= kWinCap) and the items a reload brings at most (tests shrink them: GLIA_HMT_WINCAP)
  int cond_n;
  // HORIZON (batch kernel): cells below wch are out of the queue's reach until the next baseline.  An edge created there is
  // neither linked into its cell's list nor counted, an edge dying there is not counted either: its two list entries and the
  // two cat bits of its seq (ecat) are all that is written -- no record; the baseline walks the lists of the live regions and
  // rebuilds the records of the edges that are still alive.  A reload that would have to go below the horizon ends the launch
  // with ST_REBASE instead.  0 = no horizon.
  uint32_t wch;
  // regions that have been merged away (batch kernel).  An edge that dies BELOW the horizon is not marked in its record (one
  // scattered store per dying edge less in the contraction's store stream): no reload can reach it before the next baseline,
  // and the baseline's collection pass recognises it by its dead region.
  uint8_t* rdead;
  // tests (GLIA_HMT_FORCE_TREE=k): hand the queue over to the tournament-tree kernel at the first empty window after k merges --
  // the path of ST_NEED_TREE, which no data set reaches by itself any more (oversized cells are split)
  unsigned long long force_tree;
  uint8_t* ecat;                            // [Ecap] cat bits of the seq of an edge created below the horizon (update_seq); grows with the records
};
constexpr uint32_t kWinCap = 1536;          // window slots (live items + holes)
constexpr uint32_t kWinBudget = 768;        // a reload stops before exceeding this many items ...
constexpr uint32_t kWinMinLoad = 192;       // ... and goes on to the next block of cells below this many
constexpr uint32_t kWinMinPartial = 96;     // a cell is split only if at least this much room is left
constexpr uint32_t kKillMax = 8;
constexpr int kNW = kGreedyThreads / 64;
constexpr int kWinPer = (int)(kWinCap / kGreedyThreads);
static_assert(kWinPer * kGreedyThreads == (int)kWinCap, "window capacity");
struct WinShared {
  double sal[kWinCap];
  unsigned long long seq[kWinCap];          // 0 = hole
  uint32_t e[kWinCap], u[kWinCap], v[kWinCap];
  uint2 hu[kWinCap], hv[kWinCap];           // (offset, length) of u's and v's incident-edge lists
  // threshold: an item is in the window iff cell(sal) > cthr, or cell(sal) == cthr and (sal, seq) > (tsal, tseq)
  int cthr; uint32_t iptr;                  // initial entries before iptr of the sorted array are consumed
  double tsal; unsigned long long tseq;
  alignas(16) uint32_t n;                   // slots in use   (n, nk, kovf, pad0: one 16-byte read in the scan)
  uint32_t nk, kovf, pad0;                  // edges that died in this contraction and sit in the window
  alignas(16) uint32_t kill[kKillMax];
  alignas(16) Key part[kNW];                // per-wave maxima of the last scan (arg = slot)
  uint32_t touched[2][64];                  // regions whose lists the previous / this contraction rewrites (bitmap over id mod 2048)
  uint32_t wsum[kNW];                       // block scan scratch
  uint32_t bcast, maxcell, err, need_tree;
  double psal; unsigned long long pseq;     // split of a cell: the list's contribution to tau
  unsigned long long spill_ord;             // image of the largest saliency that found the window full (0 = none): tau has to rise to it
};
struct WinWork {                            // the neighbour table of one contraction (small case)
  uint32_t mk[kMarkSlots], mv0[kMarkSlots], mv1[kMarkSlots];     // neighbour + 1, staged index + 1 of the (r0,rs) / (r1,rs) entry
  uint32_t items[kMarkMax], newidx[kMarkMax], nitems, newcount, bad;     // items[i]: table slot of neighbour i, then the pool position of its new entry
  FatEntry stage[kMarkMax];
};

__host__ __device__ __forceinline__ uint32_t win_cell(double sal, double smin, double scale, uint32_t B) {
  double t = (sal - smin) * scale;          // monotone in sal (saliencies are never NaN: sdivide guards the division)
  t = t > 0.0 ? t : 0.0;
  return t >= (double)(B - 1u) ? B - 1u : (uint32_t)t;
}
__device__ __forceinline__ bool win_above(int cthr, double tsal, unsigned long long tseq, int cell, double sal, unsigned long long seq) {
  return cell > cthr || (cell == cthr && (sal > tsal || (sal == tsal && seq > tseq)));
}

// inclusive block scan of one value per thread (every thread calls; two barriers)
__device__ __forceinline__ uint32_t block_scan_incl(uint32_t v, uint32_t* wsum, int tid, uint32_t* total) {
  const int lane = tid & 63, wave = tid >> 6;
  uint32_t x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)x, d); if (lane >= d) x += y; }
  full_barrier();   // [B:scan1]
  if (lane == 63) wsum[wave] = x;
  full_barrier();   // [B:scan2]
  uint32_t base = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < kNW; ++i) { const uint32_t s = wsum[i]; if (i < wave) base += s; tot += s; }
  *total = tot;
  return base + x;
}

__device__ __forceinline__ void win_put(WinShared& w, uint32_t slot, double sal, unsigned long long seq, uint32_t e, uint32_t u, uint32_t v, uint2 hu, uint2 hv) {
  w.sal[slot] = sal; w.seq[slot] = seq; w.e[slot] = e; w.u[slot] = u; w.v[slot] = v; w.hu[slot] = hu; w.hv[slot] = hv;
}
// edge e of the global storage into the window if it is alive
__device__ __forceinline__ void win_take(const WinState& st, WinShared& w, uint32_t e, const EdgeRec& r) {
  if (r.seq != 0) {
    const uint32_t slot = atomicAdd(&w.n, 1u);
    if (slot < st.wcap) win_put(w, slot, r.sal, r.seq, e, r.u, r.v, r.hu, r.hv); else w.err = 1;
  }
}

// One pass over the window: applies this contraction's deaths, completes the list header of the region just created
// (its length was not known when its edges were inserted), leaves the per-wave maxima in w.part.  Every LDS read is
// issued up front (a load inside a branch is a round trip of its own).  Ends with an LDS-only barrier.
__device__ __forceinline__ void win_scan(const WinState& st, WinShared& w, int tid, uint32_t r2, uint32_t r2len) {
  const uint4 hd = *reinterpret_cast<const uint4*>(&w.n);                 // n, nk, kovf   // [R:scan-head]
  const uint4 k0 = *reinterpret_cast<const uint4*>(&w.kill[0]), k1 = *reinterpret_cast<const uint4*>(&w.kill[4]);
  unsigned long long q[kWinPer]; uint32_t e[kWinPer], v[kWinPer]; double sl[kWinPer];
#pragma unroll
  for (int j = 0; j < kWinPer; ++j) { const uint32_t i = (uint32_t)tid + (uint32_t)j * kGreedyThreads; q[j] = w.seq[i]; e[j] = w.e[i]; v[j] = w.v[i]; sl[j] = w.sal[i]; }
  const uint32_t n = hd.x, nk = hd.y < kKillMax ? hd.y : kKillMax;
  const uint32_t kl[kKillMax] = {k0.x, k0.y, k0.z, k0.w, k1.x, k1.y, k1.z, k1.w};
  Key k;
  k.sal = -__builtin_inf(); k.seq = 0; k.arg = 0;
#pragma unroll
  for (int j = 0; j < kWinPer; ++j) {
    const uint32_t i = (uint32_t)tid + (uint32_t)j * kGreedyThreads;
    bool live = i < n && q[j] != 0;
    bool dead = false;
    if (nk) {
#pragma unroll
      for (uint32_t t = 0; t < kKillMax; ++t) dead = dead || (t < nk && kl[t] == e[j]);
    }
    if (live && hd.z) dead = dead || st.er[e[j]].seq == 0;       // more deaths than the list holds (rare): ask the edge record
    if (live && dead) { w.seq[i] = 0; live = false; }
    if (live && v[j] == r2) w.hv[i].y = r2len;
    Key c; c.sal = live ? sl[j] : -__builtin_inf(); c.seq = live ? q[j] : 0ull; c.arg = i;
    if (better(c, k)) k = c;
  }
  k = wave_max(k);
  if ((tid & 63) == 0) w.part[tid >> 6] = k;   // [W:scan-part]
  lds_barrier();   // [B:scan-end]
  if (tid == 0) { w.nk = 0; w.kovf = 0; }   // [W:scan-clear]
}
// the maximum of the per-wave maxima, in every lane: lanes 0..7 fetch one each, two quad steps leave the maxima of
// parts 0..3 / 4..7 in lanes 0 / 4, which are read out and compared as uniform values
__device__ __forceinline__ Key win_root(const WinShared& w, int lane) {
  static_assert(kNW == 8, "win_root");
  Key k = w.part[lane & (kNW - 1)];
  key_max_step<0xB1>(k); key_max_step<0x4E>(k);          // quad_perm [1,0,3,2], [2,3,0,1]: every lane holds its quad's maximum
  const Key a = lane_key(k, 0), b = lane_key(k, 4);
  return better(b, a) ? b : a;
}

// squeeze the holes out (every thread calls); returns the number of live items -- the same value in every thread, from the scan:
// a caller that decides on it must NOT read w.n again (the first wave past the barrier may already be adding to it)
__device__ __forceinline__ uint32_t win_compact(WinShared& w, int tid, uint32_t cap = kWinCap) {
  double sal[kWinPer]; unsigned long long seq[kWinPer]; uint32_t e[kWinPer], u[kWinPer], v[kWinPer]; uint2 hu[kWinPer], hv[kWinPer];
  uint32_t live = 0;
  const uint32_t n = w.n < cap ? w.n : cap;
#pragma unroll
  for (int j = 0; j < kWinPer; ++j) {
    const uint32_t i = (uint32_t)tid * kWinPer + j;
    seq[j] = i < n ? w.seq[i] : 0ull;
    sal[j] = w.sal[i]; e[j] = w.e[i]; u[j] = w.u[i]; v[j] = w.v[i]; hu[j] = w.hu[i]; hv[j] = w.hv[i];
    live += seq[j] != 0;
  }
  uint32_t total;
  uint32_t o = block_scan_incl(live, w.wsum, tid, &total) - live;      // barriers inside: every read above is done
#pragma unroll
  for (int j = 0; j < kWinPer; ++j) if (seq[j] != 0) { win_put(w, o, sal[j], seq[j], e[j], u[j], v[j], hu[j], hv[j]); ++o; }
  if (tid == 0) w.n = total;   // [W:compact-n]
  full_barrier();   // [B:compact-end]
  return total;
}

__device__ __forceinline__ void win_push_global(const WinState& st, uint32_t e, uint32_t cell) {
  const uint32_t old = atomicExch(&st.whead[cell], e);
  st.er[e].next = old;
  atomicAdd(&st.wcnt[cell], 1u);
}

// every live window item into its cell's list (initial edges too: their place in the sorted array is gone); afterwards
// the window is empty and the threshold sits above everything (every thread calls)
__device__ __forceinline__ void win_flush(const WinState& st, WinShared& w, int tid) {
  const double smin = st.wrange[0], scale = st.wrange[1];
  if (tid == 0) w.maxcell = 0;   // [W:maxcell-clear]
  full_barrier();   // [B:flush-enter]
  const uint32_t n = w.n < st.wcap ? w.n : st.wcap;
  uint32_t mc = 0;
  for (uint32_t i = tid; i < n; i += kGreedyThreads) {
    if (w.seq[i] == 0) continue;
    const uint32_t c = win_cell(w.sal[i], smin, scale, st.wB);
    win_push_global(st, w.e[i], c);
    mc = mc > c + 1u ? mc : c + 1u;
  }
  if (mc) atomicMax(&w.maxcell, mc);   // [W:maxcell]
  full_barrier();   // [B:flush-pushed]
  if (tid == 0) {   // [W:flush-tau]
    if (w.maxcell && (int)w.maxcell - 1 >= w.cthr) { w.cthr = (int)w.maxcell - 1; w.tsal = __builtin_inf(); w.tseq = ~0ull; }
    w.n = 0;
  }
  full_barrier();   // [B:flush-end]
}

// Items above tau found the window full and went to their cells' lists: tau rises to the largest of their saliencies and
// the window items at or below it follow them (every thread calls, after a scan has applied the pending deaths)
__device__ __forceinline__ void win_evict(const WinState& st, WinShared& w, int tid) {
  const double smin = st.wrange[0], scale = st.wrange[1];
  const double lim = f64_unord(w.spill_ord);   // [R:evict-head]
  const uint32_t n = w.n < st.wcap ? w.n : st.wcap;
  full_barrier();   // [B:evict-enter]
  for (uint32_t i = tid; i < n; i += kGreedyThreads) {
    if (w.seq[i] == 0 || w.sal[i] > lim) continue;
    win_push_global(st, w.e[i], win_cell(w.sal[i], smin, scale, st.wB));
    w.seq[i] = 0;
  }
  full_barrier();   // [B:evict-pushed]
  if (tid == 0) { w.n = n; w.cthr = (int)win_cell(lim, smin, scale, st.wB); w.tsal = lim; w.tseq = ~0ull; w.spill_ord = 0; }   // [W:evict-tau]
  full_barrier();   // [B:evict-end]
}

// initial entries [a, b) of the sorted array into the window (every thread calls; no barrier)
__device__ __forceinline__ void win_take_initial(const WinState& st, WinShared& w, uint32_t a, uint32_t b, int tid) {
  for (uint32_t i = a + (uint32_t)tid; i < b; i += kGreedyThreads) { const uint32_t e = st.isort[i]; const EdgeRec r = st.er[e]; win_take(st, w, e, r); }
}

// The window holds no live item: move the threshold down.  Returns 0 = loaded something (or made progress), 1 = the
// queue is empty, 2 = a cell's list does not fit the window, 3 = nothing left above the horizon (every thread calls;
// contains barriers)
constexpr uint32_t kSelMax = 384;           // list items a split cell hands over at most (bounded min-heap in LDS)
#ifdef GLIA_HMT_PROFILE
// where a reload's cycles go (cumulative, thread 0): [0] the descent over blocks of cells that load nothing, [1] whole-cell loads,
// [2] the split of a cell; [3] blocks of the descent, [4] reloads
__device__ unsigned long long g_reloadprof[5];
#define RELOAD_T(i) do { if (tid == 0) { const unsigned long long tn_ = __builtin_readcyclecounter(); g_reloadprof[i] += tn_ - rl_; rl_ = tn_; } } while (0)
#else
#define RELOAD_T(i) do {} while (0)
#endif
__device__ __forceinline__ int win_reload(const WinState& st, WinShared& w, int tid, double* sel_sal, unsigned long long* sel_seq) {
  full_barrier();                       // (vmcnt(0) inside) this workgroup's list pushes and counter updates are done   // [B:reload-enter]
  if (tid == 0) { w.n = 0; w.need_tree = 0; }   // [W:reload-n]
  full_barrier();   // [B:reload-cleared]
  uint32_t c_hi = (uint32_t)(w.cthr + 1) < st.wB ? (uint32_t)(w.cthr + 1) : st.wB, loaded = 0, iptr = w.iptr;
  int result = 1;
  const uint32_t c_floor = st.wch < st.wB ? st.wch : 0u;      // the horizon: cells below it are not loaded
#ifdef GLIA_HMT_PROFILE
  unsigned long long rl_ = __builtin_readcyclecounter();
  if (tid == 0) g_reloadprof[4] += 1;
#endif
  while (c_hi > c_floor) {
    const bool valid = (uint32_t)tid < c_hi - c_floor;
    const uint32_t c = valid ? c_hi - 1u - (uint32_t)tid : 0u;
    const uint32_t cn = valid ? ld_relaxed(&st.wcnt[c]) : 0u;
    uint32_t total;
    const uint32_t incl = block_scan_incl(cn, w.wsum, tid, &total);
    const bool ok = valid && incl <= st.wbudget - loaded;
    const uint32_t m = (uint32_t)__syncthreads_count(ok ? 1 : 0);       // ok is monotone in tid: the first m cells fit whole
    const uint32_t nvalid = c_hi - c_floor < (uint32_t)kGreedyThreads ? c_hi - c_floor : (uint32_t)kGreedyThreads;
    if (m != 0) {
      const uint32_t c_lo = c_hi - m;
      if ((uint32_t)tid == m - 1u) w.bcast = incl;   // [W:bcast-whole]
      const uint32_t i_to = st.ige[c_lo];                                // initial entries with cell >= c_lo
      win_take_initial(st, w, iptr, i_to, tid);
      iptr = i_to > iptr ? i_to : iptr;
      if ((uint32_t)tid < m) {
        uint32_t e = ld_relaxed(&st.whead[c]);
        if (e != kNone) {
          st_agent(&st.whead[c], kNone);
          if (cn != 0) while (e != kNone) { const EdgeRec r = st.er[e]; win_take(st, w, e, r); e = r.next; }
        }
        if (cn != 0) st_agent(&st.wcnt[c], 0u);
      }
      full_barrier();   // [B:whole-taken]
      loaded += w.bcast;   // [R:bcast-whole]
      c_hi = c_lo;
      if (loaded) result = 0;
#ifdef GLIA_HMT_PROFILE
      if (w.bcast == 0u) { if (tid == 0) g_reloadprof[3] += 1; RELOAD_T(0); }      // (cells with count 0 "fit whole": a block of them loads nothing)
      else RELOAD_T(1);
#endif
    } else RELOAD_T(0);
    if (m < nvalid) {
      // Cell c* = c_hi - 1 does not fit whole (a tie group of thousands of equal means, typically): the threshold moves
      // INTO the cell.  Its items are a sorted array segment (initial edges) and an unordered list (created edges); thread 0
      // finds the list's K largest keys with a bounded min-heap in LDS, the new tau is the larger of the heap's minimum and
      // the key of the array entry RA places ahead, and everything above tau moves: at most K - 1 + RA items.
      const uint32_t room = st.wbudget - loaded;
      const uint32_t cs = c_hi - 1u;
      if (room >= (kWinMinPartial < st.wbudget / 8u ? kWinMinPartial : st.wbudget / 8u) || loaded == 0) {
        const uint32_t K = (room / 2u < kSelMax ? room / 2u : kSelMax) > 1u ? (room / 2u < kSelMax ? room / 2u : kSelMax) : 2u, RA = room > K ? room - K : 1u;
        const uint32_t seg_end = st.ige[cs];
        const uint32_t before = w.n;
        if (tid == 0) {
          uint32_t hn = 0, nlive = 0;
          for (uint32_t e = ld_relaxed(&st.whead[cs]); e != kNone;) {
            const EdgeRec r = st.er[e];
            if (r.seq != 0) {
              ++nlive;
              if (hn < K) {                                                   // push, sift up (min-heap by key)
                uint32_t i = hn++;
                while (i > 0) {
                  const uint32_t p = (i - 1u) >> 1;
                  if (!(sel_sal[p] > r.sal || (sel_sal[p] == r.sal && sel_seq[p] > r.seq))) break;
                  sel_sal[i] = sel_sal[p]; sel_seq[i] = sel_seq[p]; i = p;
                }
                sel_sal[i] = r.sal; sel_seq[i] = r.seq;
              } else if (r.sal > sel_sal[0] || (r.sal == sel_sal[0] && r.seq > sel_seq[0])) {   // replace the minimum, sift down
                uint32_t i = 0;
                while (true) {
                  uint32_t c = 2u * i + 1u;
                  if (c >= hn) break;
                  if (c + 1u < hn && (sel_sal[c + 1u] < sel_sal[c] || (sel_sal[c + 1u] == sel_sal[c] && sel_seq[c + 1u] < sel_seq[c]))) ++c;
                  if (!(sel_sal[c] < r.sal || (sel_sal[c] == r.sal && sel_seq[c] < r.seq))) break;
                  sel_sal[i] = sel_sal[c]; sel_seq[i] = sel_seq[c]; i = c;
                }
                sel_sal[i] = r.sal; sel_seq[i] = r.seq;
              }
            }
            e = r.next;
          }
          // tau from the list: the heap's minimum if the list holds more than the heap
          w.psal = nlive > K ? sel_sal[0] : -__builtin_inf(); w.pseq = nlive > K ? sel_seq[0] : 0ull;   // [W:psal]
        }
        full_barrier();   // [B:heap]
        double tsal = w.psal; unsigned long long tseq = w.pseq;   // [R:psal]
        const uint32_t iA = seg_end > iptr ? (seg_end - iptr < RA ? seg_end : iptr + RA) : iptr;
        if (iA < seg_end) {                                                     // array entries stay behind: their first one bounds tau
          const uint32_t et = st.isort[iA]; const double as = st.er[et].sal; const unsigned long long aq = st.isort_seq[iA];
          if (as > tsal || (as == tsal && aq > tseq)) { tsal = as; tseq = aq; }
        }
        if (tid == 0) w.bcast = 0;   // [W:bcast-zero]
        full_barrier();   // [B:bcast-zero]
        // array entries above tau (a prefix of [iptr, iA): the array is sorted)
        uint32_t mine = 0;
        for (uint32_t i = iptr + (uint32_t)tid; i < iA; i += kGreedyThreads) {
          const uint32_t e = st.isort[i]; const EdgeRec r = st.er[e];
          const unsigned long long q = st.isort_seq[i];                         // (a dead entry's seq is gone from its record)
          if (r.sal > tsal || (r.sal == tsal && q > tseq)) { ++mine; win_take(st, w, e, r); }
        }
        if (mine) atomicAdd(&w.bcast, mine);   // [W:bcast-add]
        full_barrier();   // [B:array-taken]
        iptr += w.bcast;   // [R:bcast-array]
        if (tid == 0) {
          // list nodes above tau move, the others stay linked
          uint32_t keep_head = kNone, keep_tail = kNone;
          for (uint32_t e = ld_relaxed(&st.whead[cs]); e != kNone;) {
            const EdgeRec r = st.er[e];
            if (r.seq != 0) {
              if (r.sal > tsal || (r.sal == tsal && r.seq > tseq)) win_take(st, w, e, r);
              else { if (keep_head == kNone) keep_head = e; else st.er[keep_tail].next = e; keep_tail = e; }
            }
            e = r.next;
          }
          if (keep_tail != kNone) st.er[keep_tail].next = kNone;
          st_agent(&st.whead[cs], keep_head);
        }
        full_barrier();   // [B:list-taken]
        const uint32_t moved = w.n - before;
        if (moved == 0u && w.bcast == 0u) {   // [R:moved]
          // nothing above the new tau and no array entry passed: the cell is empty, its count was too high (counts are upper
          // bounds: the batch kernel does not discount an edge that dies with exactly tau's key) -- on to the cells below
          full_barrier();   // [B:empty-cell]
          if (tid == 0) st_agent(&st.wcnt[cs], 0u);
          c_hi = cs;
          RELOAD_T(2);
          continue;
        }
        if (tid == 0) { if (moved) atomicSub(&st.wcnt[cs], moved); w.cthr = (int)cs; w.tsal = tsal; w.tseq = tseq; w.iptr = iptr; }   // [W:split-tau]
        if (moved || w.bcast) result = 0;
        full_barrier();   // [B:split-end]
        RELOAD_T(2);
        return result;
      }
      break;
    }
    if (loaded >= (kWinMinLoad < st.wbudget / 4u ? kWinMinLoad : st.wbudget / 4u)) break;      // else: a whole block of (nearly) empty cells, go on below it
  }
  full_barrier();   // [B:reload-exit]
  if (tid == 0 && result != 2) { w.cthr = (int)c_hi - 1; w.tsal = __builtin_inf(); w.tseq = ~0ull; w.iptr = iptr; }   // [W:reload-tau]
  full_barrier();   // [B:reload-end]
  if (result == 1 && c_floor != 0u) result = 3;
  return result;
}

// ---- one contraction's edge update, piece by piece: shared by greedy_window_kernel, batch_contract_wide and the batch commit ----
// tau and the cell quantisation as a contraction sees them (registers: read from LDS / global memory once, in front of the store stream)
struct WinTau { int cthr; double tsal; unsigned long long tseq; double smin, scale; };

// Stage the two incident-edge lists of the contracted edge e (the contraction's one global round trip) and enter every live entry
// into the neighbour table: LDS (small) or the global mark arrays.  Every thread calls; the caller puts the barrier.
__device__ __forceinline__ void win_stage_lists(const WinState& st, WinWork& s, int tid, uint32_t e, uint32_t off0, uint32_t len0, uint32_t off1, uint32_t len1, bool small) {
  const uint32_t total = len0 + len1;
  for (uint32_t i = tid; i < total; i += kGreedyThreads) {
    const bool side1 = i >= len0;
    const FatEntry fe = st.fpool[side1 ? off1 + (i - len0) : off0 + i];
    if (fe.eid == e || fe.eid == kNone) continue;
    if (small) {
      s.stage[i] = fe;
      uint32_t h = (fe.rs * 2654435761u) >> 21;
      while (true) {
        const uint32_t old = atomicCAS(&s.mk[h], 0u, fe.rs + 1u);
        if (old == 0u) { s.items[atomicAdd(&s.nitems, 1u)] = h; break; }
        if (old == fe.rs + 1u) break;
        h = (h + 1u) & (kMarkSlots - 1u);
      }
      (side1 ? s.mv1 : s.mv0)[h] = i + 1u;
    } else (side1 ? st.mark1 : st.mark0)[fe.rs] = i + 1u;
  }
}
// A list entry as its two 16-byte halves (FatEntry: eid, rs, n, pos | off, len, mean), and a fence that makes the compiler hold three
// entries in registers at this point: their loads cannot sink under a later branch, and all six are issued before the one wait.
struct FatHalves { uint4 lo, hi; };
static_assert(sizeof(FatHalves) == sizeof(FatEntry), "FatEntry halves");
__device__ __forceinline__ FatHalves fat_load(const FatEntry* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  FatHalves f; f.lo = q[0]; f.hi = q[1];
  return f;
}
__device__ __forceinline__ void fat_pin(const FatHalves (&f)[3]) {      // (inputs only: a tied output would be a copy, and a copy waits)
  asm volatile("" :: "v"(f[0].lo.x), "v"(f[0].lo.y), "v"(f[0].lo.z), "v"(f[0].lo.w), "v"(f[0].hi.x), "v"(f[0].hi.y), "v"(f[0].hi.z), "v"(f[0].hi.w),
               "v"(f[1].lo.x), "v"(f[1].lo.y), "v"(f[1].lo.z), "v"(f[1].lo.w), "v"(f[1].hi.x), "v"(f[1].hi.y), "v"(f[1].hi.z), "v"(f[1].hi.w),
               "v"(f[2].lo.x), "v"(f[2].lo.y), "v"(f[2].lo.z), "v"(f[2].lo.w), "v"(f[2].hi.x), "v"(f[2].hi.y), "v"(f[2].hi.z), "v"(f[2].hi.w));
}
__device__ __forceinline__ double fat_mean(const FatHalves& f) { return __longlong_as_double((long long)(((unsigned long long)f.hi.w << 32) | f.hi.z)); }
// win_stage_lists for the batch kernel's LDS-table case (192 < total <= kMarkMax, at most kStageP entries per lane): ONE round trip.
// Every lane loads both halves of all its entries, lanes past the end from the list's last entry instead of branching round the load,
// and `eid` is tested once everything has arrived.  (win_stage_lists fetches an entry in three pieces with a wait behind each -- the
// early `continue` sinks the other fields under a branch -- and requests pass p + 1 behind pass p's table inserts.)
constexpr int kStageP = (int)((kMarkMax + kGreedyThreads - 1) / kGreedyThreads);
__device__ __forceinline__ void win_stage_lists_small(const WinState& st, WinWork& s, int tid, uint32_t e, uint32_t off0, uint32_t len0, uint32_t off1, uint32_t len1) {
  const uint32_t total = len0 + len1, last = total - 1u;      // (total >= 1: the caller's contraction is wide)
  FatHalves f[kStageP];
#pragma unroll
  for (int p = 0; p < kStageP; ++p) {
    const uint32_t i = (uint32_t)tid + (uint32_t)p * kGreedyThreads, ic = i < total ? i : last;
    f[p] = fat_load(&st.fpool[ic >= len0 ? off1 + (ic - len0) : off0 + ic]);
  }
  static_assert(kStageP == 3, "fat_pin");
  fat_pin(f);
#pragma unroll
  for (int p = 0; p < kStageP; ++p) {
    const uint32_t i = (uint32_t)tid + (uint32_t)p * kGreedyThreads;
    const uint32_t eid = f[p].lo.x, rs = f[p].lo.y;
    if (i >= total || eid == e || eid == kNone) continue;
    uint4* dst = reinterpret_cast<uint4*>(&s.stage[i]);
    dst[0] = f[p].lo; dst[1] = f[p].hi;
    uint32_t h = (rs * 2654435761u) >> 21;
    while (true) {
      const uint32_t old = atomicCAS(&s.mk[h], 0u, rs + 1u);
      if (old == 0u) { s.items[atomicAdd(&s.nitems, 1u)] = h; break; }
      if (old == rs + 1u) break;
      h = (h + 1u) & (kMarkSlots - 1u);
    }
    (i >= len0 ? s.mv1 : s.mv0)[h] = i + 1u;
  }
}
// Work item i of a contraction: neighbour rs, which of (r0,rs) / (r1,rs) exist (h0, h1) and their entries f0, f1 (a missing one
// repeats the other).  SMALL: item i of the LDS table, whose slot is cleared; else list entry i with the global marks.
// Returns false when the item is no neighbour (contracted edge, tombstone, or a common neighbour seen from the r1 side).
template <bool SMALL>
__device__ __forceinline__ bool win_match(const WinState& st, WinWork& s, uint32_t i, uint32_t e, uint32_t off0, uint32_t len0, uint32_t off1,
                                          uint32_t* rs, bool* h0, bool* h1, FatEntry* f0, FatEntry* f1) {
  if constexpr (SMALL) {
    const uint32_t h = s.items[i];
    *rs = s.mk[h] - 1u;
    const uint32_t m0 = s.mv0[h], m1 = s.mv1[h];
    s.mk[h] = 0u; s.mv0[h] = 0u; s.mv1[h] = 0u;
    *h0 = m0 != 0; *h1 = m1 != 0;
    *f0 = s.stage[*h0 ? m0 - 1u : m1 - 1u]; *f1 = s.stage[*h1 ? m1 - 1u : m0 - 1u];
  } else {
    const bool side1 = i >= len0;
    const FatEntry fe = st.fpool[side1 ? off1 + (i - len0) : off0 + i];
    if (fe.eid == e || fe.eid == kNone) return false;
    *rs = fe.rs;
    if (!side1) {
      const uint32_t m = st.mark1[fe.rs];
      *h0 = true; *h1 = m != 0; *f0 = fe;
      *f1 = *h1 ? st.fpool[off1 + (m - 1u - len0)] : fe;
    } else {
      if (st.mark0[fe.rs] != 0u) return false;         // common neighbour: handled from the r0 side
      *h0 = false; *h1 = true; *f0 = fe; *f1 = fe;
    }
  }
  return true;
}
// The new edge newE = (rs, r2): its record (four 16-byte stores), rs's reused list entry and r2's new one.  lenR2 = 0: r2's list
// length is not known yet, the caller completes the headers (win_complete_r2).  cell = win_cell(sal).
// BATCH = true and cell below the horizon: no record (nobody reads it before the next baseline, which rebuilds it from r2's entry if
// the edge is still alive then: rebuild_edge_record) -- the two entries and the cat bits of the seq, one byte, are all that is stored.
template <bool BATCH>
__device__ __forceinline__ void store_new_edge(const WinState& st, uint32_t newE, uint32_t rs, uint32_t r2, uint32_t posRs, uint32_t idx, double first, int second,
                                               double sal, unsigned long long seq, uint32_t offRs, uint32_t lenRs, uint32_t r2off, uint32_t lenR2, uint32_t cell) {
  if (BATCH && cell < st.wch) st.ecat[newE] = (uint8_t)((uint32_t)(seq >> 30) & 3u);
  else {
    uint4* pq4 = reinterpret_cast<uint4*>(&st.er[newE]);
    pq4[0] = make_uint4(rs, r2, posRs, idx);
    const unsigned long long mb = (unsigned long long)__double_as_longlong(first);
    pq4[1] = make_uint4((uint32_t)mb, (uint32_t)(mb >> 32), (uint32_t)second, kNone);
    pq4[2] = make_uint4(offRs, lenRs, r2off, lenR2);
    const unsigned long long sbits = (unsigned long long)__double_as_longlong(sal);
    pq4[3] = make_uint4((uint32_t)sbits, (uint32_t)(sbits >> 32), (uint32_t)seq, (uint32_t)(seq >> 32));
  }
  FatEntry a; a.eid = newE; a.rs = r2; a.n = (uint32_t)second; a.pos = idx; a.off = r2off; a.len = lenR2; a.mean = first;
  st.fpool[offRs + posRs] = a;
  FatEntry b; b.eid = newE; b.rs = rs; b.n = (uint32_t)second; b.pos = posRs; b.off = offRs; b.len = lenRs; b.mean = first;
  st.fpool[r2off + idx] = b;
}
// Queue the new edge: a window slot if its key is above tau, else its cell's list, whose `next` link is stored by the caller's
// NEXT push or after its loop (pend_e / pend_old: nobody waits for the atomic).
// BATCH = false (one-at-a-time kernel): the caller has made room beforehand (compaction / flush), so every slot number is valid, and
//   there is no horizon.  BATCH = true: a full window spills the item to its list and raises w.spill_ord (win_evict follows), and an
//   item below the horizon st.wch is not queued at all (it has no record either: an item above tau is never below the horizon --
//   tau's cell is at least wch - 1, and there only with tsal = +inf).  cell = win_cell(sal), shared with store_new_edge.
template <bool BATCH>
__device__ __forceinline__ void win_queue_edge(const WinState& st, WinShared& w, const WinTau& tau, uint32_t newE, double sal, unsigned long long seq, uint32_t rs, uint32_t r2,
                                               uint2 hrs, uint2 hr2, uint32_t cell, uint32_t& pend_e, uint32_t& pend_old) {
  const bool above = win_above(tau.cthr, tau.tsal, tau.tseq, (int)cell, sal, seq);
  uint32_t sl = kWinCap;
  if (above) {
    sl = atomicAdd(&w.n, 1u);   // [W:wn-add]
    if (!BATCH || sl < st.wcap) win_put(w, sl, sal, seq, newE, rs, r2, hrs, hr2);
    else atomicMax(&w.spill_ord, f64_ord(sal));          // the window is full: tau will rise above this item   // [W:spill]
  }
  if (BATCH ? (sl >= st.wcap && (above || cell >= st.wch)) : !above) {
    if (pend_e != kNone) st.er[pend_e].next = pend_old;
    pend_e = newE; pend_old = atomicExch(&st.whead[cell], newE);
    atomicAdd(&st.wcnt[cell], 1u);
  }
}
// A replaced edge de (saliency dsal) leaves the queue: a window item goes on the kill list the next scan applies (KMAX entries at
// *nkill / kill, *kovf beyond), an item below tau is discounted from its cell.
// A key equal to tau's in tau's cell: the seq decides where the edge lives, and it sits in the edge record.
// BATCH = false: that seq is loaded (and always under COND, where 0 = rejected earlier, out of the queue already).
// BATCH = true: no load in the middle of the store stream -- on this hardware it makes the wave wait for every store before it (one
//   counter for both).  A tie is treated as a window item instead: a kill that matches nothing is harmless, and its cell's count
//   stays one too high until the next baseline (counts are upper bounds: a reload walks a list whenever its count is not zero).
//   Below the horizon nothing is written: WinState::rdead speaks for the edge.
template <bool BATCH, bool COND, uint32_t KMAX>
__device__ __forceinline__ void win_retire_edge(const WinState& st, const WinTau& tau, uint32_t de, double dsal, uint32_t* nkill, uint32_t* kill, uint32_t* kovf) {
  const uint32_t dc = win_cell(dsal, tau.smin, tau.scale, st.wB);
  const bool tie = (int)dc == tau.cthr && dsal == tau.tsal;
  unsigned long long dq = BATCH ? 0ull : 1ull;
  if (BATCH && dc < st.wch) return;
  if (!BATCH && (COND || tie)) dq = st.er[de].seq;
  st.er[de].seq = 0;   // [W:retire-seq]
  if (!BATCH && dq == 0) return;
  if ((BATCH && tie) || win_above(tau.cthr, tau.tsal, tau.tseq, (int)dc, dsal, dq)) {
    const uint32_t j = atomicAdd(nkill, 1u); if (j < KMAX) kill[j] = de; else *kovf = 1;   // [W:kill]
  } else atomicSub(&st.wcnt[dc], 1u);
}
// r2's list length is known only after a contraction on the global marks: complete the headers that point at it and clear the marks
// (BATCH: an edge below the horizon has no record to complete -- store_new_edge's predicate on the entry's mean)
template <bool BATCH>
__device__ __forceinline__ void win_complete_r2(const WinState& st, int tid, uint32_t ne, uint32_t r2off, uint32_t newcount, double smin, double scale) {
  for (uint32_t j = tid; j < newcount; j += kGreedyThreads) {
    const FatEntry fb = st.fpool[r2off + j];
    st.fpool[fb.off + fb.pos].len = newcount;
    if (!BATCH || win_cell(-fb.mean, smin, scale, st.wB) >= st.wch) st.er[ne + j].hv.y = newcount;
    st.mark0[fb.rs] = 0; st.mark1[fb.rs] = 0;
  }
}
// Kernel entry and exit of the two window-queue kernels (every thread calls; no barrier inside win_enter, the caller's follows).
// ctrl layout: GreedyState::ctrl (greedy_tree.hpp).
__device__ __forceinline__ void win_enter(const WinState& st, WinShared& w, WinWork& s, int tid) {
  if (tid == 0) {
    w.n = 0; w.nk = 0; w.kovf = 0; w.err = 0; w.spill_ord = 0; s.nitems = 0; s.newcount = 0; s.bad = 0;
    w.cthr = (int)(long long)st.ctrl[CTRL_CTHR]; w.tsal = __longlong_as_double((long long)st.ctrl[CTRL_TSAL]); w.tseq = st.ctrl[CTRL_TSEQ]; w.iptr = (uint32_t)st.ctrl[CTRL_IPTR];
  }
  for (uint32_t i = tid; i < kMarkSlots; i += kGreedyThreads) { s.mk[i] = 0; s.mv0[i] = 0; s.mv1[i] = 0; }
  for (uint32_t i = tid; i < kWinCap; i += kGreedyThreads) { w.seq[i] = 0; w.e[i] = 0; w.v[i] = 0; w.sal[i] = 0.0; }
}
// leave through the global lists: the next launch (or the tree kernel) starts from them (the caller's full_barrier precedes)
__device__ __forceinline__ void win_leave(const WinState& st, WinShared& w, int tid, unsigned long long k, unsigned long long ne, unsigned long long pool_used, uint32_t status) {
  win_flush(st, w, tid);
  if (tid == 0) {
    st.ctrl[CTRL_MERGES] = k; st.ctrl[CTRL_EDGES] = ne; st.ctrl[CTRL_ENTRIES] = pool_used;
    st.ctrl[CTRL_STATUS] = w.err ? (unsigned long long)ST_INTERNAL : status; st.ctrl[CTRL_WERR] = w.err; st.ctrl[CTRL_WFILL] = w.n;
    st.ctrl[CTRL_CTHR] = (unsigned long long)(long long)w.cthr; st.ctrl[CTRL_TSAL] = (unsigned long long)__double_as_longlong(w.tsal); st.ctrl[CTRL_TSEQ] = w.tseq; st.ctrl[CTRL_IPTR] = w.iptr;
  }
}

template <bool COND>
__global__ __launch_bounds__(kGreedyThreads) void greedy_window_kernel(WinState st) {
  __shared__ WinShared w;
  __shared__ WinWork s;
  const int tid = threadIdx.x, lane = tid & 63;
  unsigned long long k = st.ctrl[CTRL_MERGES], ne = st.ctrl[CTRL_EDGES], pool_used = st.ctrl[CTRL_ENTRIES];
  uint32_t status = ST_RUN;
  win_enter(st, w, s, tid);
  if (tid < 128) w.touched[tid >> 6][tid & 63] = 0;
  if (tid < kNW) { w.part[tid].sal = -__builtin_inf(); w.part[tid].seq = 0; w.part[tid].arg = 0; }
  full_barrier();   // [B:enter]
  const double smin = st.wrange[0], scale = st.wrange[1];
  uint32_t r2prev = kNone;
#ifdef GLIA_HMT_PROFILE
  unsigned long long wph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, wlast = __builtin_readcyclecounter(), wtiter = wlast;
  unsigned long long wtb[5] = {0, 0, 0, 0, 0}, wnb[5] = {0, 0, 0, 0, 0}, wdb[5] = {0, 0, 0, 0, 0}, wreloads = 0, wcompacts = 0, wloaded = 0, winwin = 0, wdeps = 0;
#define WPH(i) do { if (tid == 0) { unsigned long long tn = __builtin_readcyclecounter(); wph[i] += tn - wlast; wlast = tn; } } while (0)
#else
#define WPH(i) do {} while (0)
#endif

  for (unsigned long long it = 0; it < st.max_iters; ++it) {
    const Key root = win_root(w, lane);   // [R:root]
    if (root.seq == 0) {
      WPH(5);
      if (st.force_tree && k >= st.force_tree) { status = ST_NEED_TREE; break; }
      const int r = win_reload(st, w, tid, reinterpret_cast<double*>(&s.stage[0]), reinterpret_cast<unsigned long long*>(&s.stage[0]) + kSelMax);
#ifdef GLIA_HMT_PROFILE
      wreloads += 1; wloaded += w.n;
#endif
      WPH(6);
      if (r == 1) { status = ST_DONE; break; }
      if (r == 2) { status = ST_NEED_TREE; break; }
      if (r == 3) { status = ST_REBASE; break; }
      win_scan(st, w, tid, kNone, 0);
      r2prev = kNone;                      // (the reload's barriers waited for every store)
      continue;
    }
    const uint32_t slot = root.arg;
    const uint32_t e = w.e[slot], r0 = w.u[slot], r1 = w.v[slot];
    const uint2 h0r = w.hu[slot], h1r = w.hv[slot];
    const uint32_t wn_now = w.n;   // [R:wn-now]
    const int cthr = w.cthr; const double tsal = w.tsal; const unsigned long long tseq = w.tseq;   // [R:tau]
    const uint32_t off0 = h0r.x, len0 = h0r.y, off1 = h1r.x, len1 = h1r.y;
    const uint32_t total = len0 + len1;
    if (k >= (unsigned long long)st.R0) { status = ST_INTERNAL; break; }      // more merges than regions: the state is corrupt, stop before writing past the outputs
    const uint32_t r2 = st.R0 + (uint32_t)k;
    const uint32_t r2off = (uint32_t)pool_used;
    const int par = (int)(k & 1ull);
    // does this contraction read a list the previous one is still writing?  (r2prev's list and its neighbours' lists)
    const uint32_t tb0 = w.touched[par ^ 1][(r0 >> 5) & 63u], tb1 = w.touched[par ^ 1][(r1 >> 5) & 63u];   // [R:touched]
    const bool dep = r2prev != kNone && (r1 == r2prev || r0 == r2prev || ((tb0 >> (r0 & 31u)) & 1u) || ((tb1 >> (r1 & 31u)) & 1u));
    if (dep) {
      full_barrier();                    // (vmcnt(0) inside) the previous contraction's stores are done   // [B:dep]
#ifdef GLIA_HMT_PROFILE
      wdeps += 1;
#endif
    }
    WPH(0);
    if (COND) {
      // pre_merge condition (gadget/main_pre_merge.cxx:27-76), see the tree kernel: a rejected item leaves the queue for good
      unsigned long long sz0 = st.rsz[r0], sz1 = st.rsz[r1]; double su0 = st.rsum[r0], su1 = st.rsum[r1];
      const unsigned long long z2 = sz0 + sz1; const double w2 = su0 + su1;
      if (sz0 > sz1) { const unsigned long long t = sz0; sz0 = sz1; sz1 = t; const double d = su0; su0 = su1; su1 = d; }
      bool ok = sz0 < st.cond_t0;
      if (!ok && st.cond_n > 1) {
        if (sz0 < st.cond_t1 && sdivide(su0, (double)sz0, 0.0) > st.cond_rpb) ok = true;
        if (!ok && sz1 < st.cond_t1 && sdivide(su1, (double)sz1, 0.0) > st.cond_rpb) ok = true;
      }
      if (!ok) {
        full_barrier();                 // every thread has read the slot   // [B:reject-read]
        if (tid == 0) { w.seq[slot] = 0; st.er[e].seq = 0; }
        full_barrier();   // [B:reject-done]
        win_scan(st, w, tid, kNone, 0);
        continue;
      }
      if (tid == 0) { st.rsz[r2] = z2; st.rsum[r2] = w2; }               // TRegionMap::merge (updateRegion)
    }
    if (ne + total > st.Ecap) { status = ST_NEED_EDGES; break; }
    if (pool_used + total > st.pool_cap) { status = ST_NEED_POOL; break; }
    if (tid == 0) {
      w.seq[slot] = 0;                                                   // popped (the other threads read the rest of the slot only)
      st.order[3 * k + 0] = r0; st.order[3 * k + 1] = r1; st.order[3 * k + 2] = r2;
      st.sal_out[k] = root.sal;
      st.er[e].seq = 0;
    }
    if (tid >= 64 && tid < 128) w.touched[par][tid & 63] = 0;            // this contraction's bitmap (last read at the pop of the previous one)   // [W:touched-clear]
    const bool small = total <= kMarkMax;

    // ---- the one round trip: the two lists; one table entry per distinct neighbour ----
    win_stage_lists(st, s, tid, e, off0, len0, off1, len1, small);
    full_barrier();     // full: a wave that loaded has waited for its loads anyway, so its older stores are done for free   // [B:lists]
    WPH(1);
    // room for every new edge that may land in the window (total bounds their number)
    if (wn_now + total > st.wcap) {   // [R:room-test]
#ifdef GLIA_HMT_PROFILE
      wcompacts += 1;
#endif
      // (round 4, found by the wave-skew build: this test used to read w.n again behind win_compact's barrier -- a wave that came out of
      // it early had already started to append this contraction's edges, a late one then saw a fuller window, flushed ALONE, and the
      // workgroup hung at mismatched barriers.  The window kernel of pre_merge is this code.)
      const uint32_t wn_live = win_compact(w, tid, st.wcap);
      if (wn_live + total > st.wcap) {   // [R:wn-live]
        win_flush(st, w, tid);
        if (total > st.wcap) {             // a contraction wider than the window: nothing of it goes there
          if (tid == 0) { w.cthr = (int)st.wB; w.tsal = __builtin_inf(); w.tseq = ~0ull; }   // [W:tau-wide]
          full_barrier();   // [B:tau-wide]
        }
      }
    }
    const bool moved = wn_now + total > st.wcap;                         // (tau as the pop read it, unless the window was compacted or flushed)
    const WinTau tau = {moved ? w.cthr : cthr, moved ? w.tsal : tsal, moved ? w.tseq : tseq, smin, scale};   // [R:tau2]
    const uint32_t nwork = small ? s.nitems : total;   // [R:nitems]
    WPH(2);

    // ---- one new edge (rs, r2) per distinct neighbour (TBoundaryTable::update) ----
    bool bad = false;
    uint32_t pend_e = kNone, pend_old = kNone;          // a list push whose link is stored later (nobody waits for the atomic)
    for (uint32_t base = 0; base < nwork; base += kGreedyThreads) {
      const uint32_t i = base + tid;
      if (i >= nwork) break;
      FatEntry f0, f1;
      bool h0, h1;
      uint32_t rs;
      if (!(small ? win_match<true>(st, s, i, e, off0, len0, off1, &rs, &h0, &h1, &f0, &f1) : win_match<false>(st, s, i, e, off0, len0, off1, &rs, &h0, &h1, &f0, &f1))) continue;
      const uint32_t idx = atomicAdd(&s.newcount, 1u);
      const uint32_t newE = (uint32_t)ne + idx;
      atomicOr(&w.touched[par][(rs >> 5) & 63u], 1u << (rs & 31u));   // [W:touched-or]
      double first;
      int second;
      if (mean_link(h0, f0.mean, (int)f0.n, h1, f1.mean, (int)f1.n, &first, &second)) bad = true;
      const uint32_t offRs = f0.off, posRs = f0.pos, lenRs = f0.len;      // rs's entry of the (r0,rs) edge -- or of (r1,rs) alone -- is reused
      if (h0 && h1) st.fpool[offRs + f1.pos].eid = kNone; // rs held two entries: the other becomes a tombstone
      const unsigned long long seq = update_seq(k, rs, r0, h0);
      const double sal = -first;
      const uint32_t cell = win_cell(sal, tau.smin, tau.scale, st.wB);
      store_new_edge<false>(st, newE, rs, r2, posRs, idx, first, second, sal, seq, offRs, lenRs, r2off, 0u, cell);
      if (small) { s.items[i] = offRs + posRs; s.newidx[i] = idx; }      // (this thread comes back to them below)
      win_queue_edge<false>(st, w, tau, newE, sal, seq, rs, r2, make_uint2(offRs, lenRs), make_uint2(r2off, 0u), cell, pend_e, pend_old);
      // the replaced edges leave the queue
      if (h0) win_retire_edge<false, COND, kKillMax>(st, tau, f0.eid, -f0.mean, &w.nk, w.kill, &w.kovf);
      if (h1) win_retire_edge<false, COND, kKillMax>(st, tau, f1.eid, -f1.mean, &w.nk, w.kill, &w.kovf);
    }
    if (bad) s.bad = 1;
    if (small) lds_barrier(); else full_barrier();         // the stores of this phase stay in flight   // [B:build]
    if (s.bad) { if (pend_e != kNone) st.er[pend_e].next = pend_old; status = ST_BAD_SALIENCY; break; }   // [R:bad]
    WPH(3);
    const uint32_t newcount = s.newcount;   // [R:newcount]
    // r2's list length is known now: complete the headers that point at it
    if (small) {
      for (uint32_t i = tid; i < nwork; i += kGreedyThreads) { st.fpool[s.items[i]].len = newcount; st.er[(uint32_t)ne + s.newidx[i]].hv.y = newcount; }
    } else {
      win_complete_r2<false>(st, tid, (uint32_t)ne, r2off, newcount, smin, scale);
    }
    // Every wave has to have READ s.newcount (above) before thread 0 clears it for the next contraction.  Rounds 2-3 cleared it here
    // without a barrier in between: a wave that came out of the last barrier a few hundred cycles late read 0, completed its headers
    // with length 0 and -- worse -- went on with its private copy of `ne` short by this contraction's edges, so the edges it created
    // later overwrote records of live ones (the rare pre_merge failure of round 3; the wide path of the batch kernel
    // always had this barrier).  kovf: the scan will ask the edge records which window items died, those stores must be done as well.
    if (w.kovf) full_barrier(); else lds_barrier();   // [B:newcount-read]
    if (tid == 0) { st.adj_off[r2] = r2off; st.adj_len[r2] = newcount; s.nitems = 0; s.newcount = 0; }   // [W:newcount-clear]
    win_scan(st, w, tid, r2, newcount);
    if (pend_e != kNone) st.er[pend_e].next = pend_old;     // (the atomic has long returned; only a reload reads the link, behind a full barrier)
    r2prev = r2;
    WPH(4);
#ifdef GLIA_HMT_PROFILE
    if (tid == 0) {
      const unsigned long long tn = __builtin_readcyclecounter();
      const int b = total <= 64 ? 0 : total <= 512 ? 1 : total <= kMarkMax ? 2 : total <= 8192 ? 3 : 4;
      wtb[b] += tn - wtiter; wnb[b] += 1; wdb[b] += total; wtiter = tn; winwin += w.n;
    }
#endif
    k += 1; ne += newcount; pool_used += total;
  }
#ifdef GLIA_HMT_PROFILE
  if (tid == 0) printf("[window profile] merges %llu: pop %llu  lists+table %llu  room %llu  build %llu  finish+scan %llu  loop-top %llu  reload %llu (cycles); reloads %llu (items %llu) compactions %llu dependent %llu; mean window fill %llu\n",
                       k, wph[0], wph[1], wph[2], wph[3], wph[4], wph[5], wph[6], wreloads, wloaded, wcompacts, wdeps, k ? winwin / k : 0ull);
  if (tid == 0) printf("[window profile] by width (<=64, <=512, <=1408, <=8192, more): merges %llu %llu %llu %llu %llu  cycles %llu %llu %llu %llu %llu  entries %llu %llu %llu %llu %llu\n",
                       wnb[0], wnb[1], wnb[2], wnb[3], wnb[4], wtb[0], wtb[1], wtb[2], wtb[3], wtb[4], wdb[0], wdb[1], wdb[2], wdb[3], wdb[4]);
#endif
  full_barrier();
  win_leave(st, w, tid, k, ne, pool_used, status);
}

}  // namespace
}  // namespace glia
