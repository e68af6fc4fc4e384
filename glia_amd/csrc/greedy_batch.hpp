// glia_amd/csrc/greedy_batch.hpp -- batched contractions on the window queue (greedy_batch_kernel, the headline pb-mean path).
// Part of greedy.hip's translation unit.
//
// What the code below relies on, beyond greedy_window.hpp's list:
//   * Between the barrier in front of a scan and the one that ends it nobody writes w.n: the scan's choice of pass is uniform.
//   * A member that fails validation has only READ global memory; the commit's stores are waited for at the END of the next scan.
//   * b.kill[] / b.nkill are filled by committing waves in front of the commit barrier and consumed (then cleared by thread 0)
//     behind the scan's closing barrier; a kill that matches no window item is harmless.
//   * b.truehit is written (atomic OR, lane 0 of the earlier member's wave) between [B:compute] and [B:exact], read behind [B:exact]
//     and in front of [B:commit], and cleared by thread 0 where b.nkill is; [B:exact] sits in a branch every wave takes or none does.
//   * Below the horizon (WinState::wch) an edge is neither queued nor counted nor marked dead: WinState::rdead speaks for it.
//     It has no record either (store_new_edge<true>): a record exists iff the edge was created at or above the horizon, or has
//     been through a baseline.  Both callers of store_new_edge here go through BATCH = true: the commit and batch_contract_wide.
#pragma once
#include "greedy_window.hpp"

namespace glia {
namespace {

// =====================================================================================================================
// Batched contractions on the window queue (pb-mean linkage without a condition).
//
// One contraction of two small regions keeps a single wave busy (a few dozen list entries) and costs ~13 k cycles of
// pure sequence: pop, one global round trip, neighbour matching, a division, a dozen stores, one scan of the window.
// The other seven waves wait.  The queue's top items, however, are mostly far apart in the volume, and the greedy
// order of FAR-APART top items is known before any of them is contracted:
//   let c0 > c1 > ... be the top items of the queue (exact keys).  After contracting c0 the next pop is c1 provided
//   (a) no edge created by c0 has a saliency >= c1's (a created edge is newer, so it wins a tie), and
//   (b) c1's two regions are neither c0's regions nor neighbours of them (then c1's lists are untouched by c0);
//   by induction over the batch, member j is merge number k + j, creates region R0 + k + j and its new edges carry
//   seq = (k + j + 1) << 32 | ... exactly as in the one-by-one loop.
// A round: every wave finds the best and the second-best item of its share of the window; the items that beat every
// second-best are the exact top of the queue, in order.  Wave j COMPUTES member j on its own (lists into registers,
// neighbour matching in a private LDS table, new means), publishes what it creates (count, largest new saliency, a
// bitmap of the regions it touches); every wave then evaluates (a) and (b) for the whole batch and the valid prefix
// COMMITS (stores, queue inserts, deaths) in parallel.  Nothing is speculated on memory: a member that fails the check
// has only read.  Contractions with more than kMemMax list entries take the whole workgroup, one at a time.
// (b) is tested as stated.  The bitmap (ids mod 2048) is a filter: it holds c0's regions and live neighbours, so a pair it does
// not flag is independent, but two ids of one residue flag a pair that shares nothing -- at 1024^3 nearly every flag is of that kind.
// A flagged pair is therefore decided by c0's wave, which compares c1's two ids with the ids it entered into its bitmap (they are in
// its registers) and reports a real conflict in BatchShared::truehit.  The set so decided is a subset of what the bitmap flags and
// is exactly (b), so the induction above is untouched; rounds without a flagged pair run as they did.
// The result is bit-identical to the sequential kernels (same gate: SHA-1 of the whole 1024^3 order).
// =====================================================================================================================
constexpr uint32_t kBatchKill = 32;
constexpr int kMemP = 3;                   // list entries per lane of a batch member ...
constexpr uint32_t kMemMax = 192;          // ... and their limit (the wave's 256-slot neighbour table stays under 3/4 full)
struct BatchShared {
  alignas(16) Key part1[kNW];               // per-wave best / second-best of the last scan
  alignas(16) Key part2[kNW];
  uint32_t nkill, kovf; alignas(16) uint32_t kill[kBatchKill];
  uint32_t byrank[kNW];                     // candidate (wave) index of the batch member of rank r
  uint32_t bitmap[kNW][64];                 // regions a member touches (id mod 2048): its own two and every neighbour
  uint32_t m_newcount[kNW], m_total[kNW], m_ok[kNW];
  double m_maxsal[kNW];
  uint32_t bad;
  uint32_t truehit;                         // bit j: member j of this round shares a region or a neighbour with an earlier member (exact)
};

// The largest and the second-largest of the 64 lanes' (a1, a2) pairs of unsigned keys -- saliency images or seqs -- (a1 >= a2
// in every lane; as a multiset: two equal values count twice) in lane 63: a butterfly that merges two pairs per step.  The rows a row_bcast step does not write receive an
// empty pair (0, 0) -- merging a pair with itself, harmless for a plain maximum, would count its best twice.
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ void top2_ord_step(unsigned long long& a1, unsigned long long& a2) {
  const unsigned long long b1 = dpp64<CTRL, ROW_MASK, ROW_MASK != 0xf>(a1), b2 = dpp64<CTRL, ROW_MASK, ROW_MASK != 0xf>(a2);
  const bool g = b1 > a1;
  const unsigned long long hi = g ? b1 : a1, lo = g ? a1 : b1, m2 = b2 > a2 ? b2 : a2;
  a1 = hi; a2 = lo > m2 ? lo : m2;
}
__device__ __forceinline__ void wave_top2_ord(unsigned long long& a1, unsigned long long& a2) {
  top2_ord_step<0xB1>(a1, a2);          // quad_perm [1,0,3,2]
  top2_ord_step<0x4E>(a1, a2);          // quad_perm [2,3,0,1]
  top2_ord_step<0x124>(a1, a2);         // row_ror 4
  top2_ord_step<0x128>(a1, a2);         // row_ror 8: every lane holds its row's pair
  top2_ord_step<0x142, 0xa>(a1, a2);    // row_bcast 15 into rows 1 and 3
  top2_ord_step<0x143, 0xc>(a1, a2);    // row_bcast 31 into rows 2 and 3: lane 63 holds the wave's pair
  a1 = lane_u64(a1, 63); a2 = lane_u64(a2, 63);
}

// one pass over the window: applies the deaths of the last round, leaves every wave's best and second-best item
#ifdef GLIA_HMT_PROFILE
__device__ unsigned long long g_scanprof[8];
__device__ unsigned long long g_scanfill[3][3];           // scans by what came before (reload or eviction / narrow round / wide contraction) x fill n (<= 512, <= 1024, more)
__device__ unsigned long long g_kovf;                     // scans that found the kill list overflowed (cumulative)
#define SCAN_T(i) do { if (tid == 0) { const unsigned long long tn_ = __builtin_readcyclecounter(); g_scanprof[i] += tn_ - st_; st_ = tn_; } } while (0)
#else
#define SCAN_T(i) do {} while (0)
#endif
enum { kScanOther = 0, kScanNarrow = 1, kScanWide = 2 };   // (profiling build: what the scan follows)
__device__ __forceinline__ void batch_scan(const WinState& st, WinShared& w, BatchShared& b, int tid, [[maybe_unused]] int from) {
#ifdef GLIA_HMT_PROFILE
  unsigned long long st_ = __builtin_readcyclecounter();
  if (tid == 0) g_scanprof[7] += 1;
#endif
  const uint32_t n = w.n < st.wcap ? w.n : st.wcap, nk = b.nkill < kBatchKill ? b.nkill : kBatchKill, kovf = b.kovf;   // [R:scan-head]
#ifdef GLIA_HMT_PROFILE
  if (tid == 0) g_scanfill[from][n <= 512u ? 0 : n <= 1024u ? 1 : 2] += 1;
  if (tid == 0 && kovf) g_kovf += 1;
#endif
  // Slot ownership is STRIPED over the waves (lane l of wave v scans the l-th slot of chunk (v + l) mod 8 in every block
  // of 512): a reload fills consecutive slots with consecutive keys, and the exact top of the queue is only as long as
  // the run of best items that sit with different waves.  (Bank pattern of a wave's reads: that of consecutive slots.)
  const uint32_t own = 64u * (uint32_t)(((tid >> 6) + (tid & 63)) & 7) + (uint32_t)(tid & 63);
  Key k1, k2;
  k1.sal = -__builtin_inf(); k1.seq = 0; k1.arg = 0; k2 = k1;
  // Only the blocks of 512 slots below the fill are read: slots at or above n hold nothing, and n is the same in every thread
  // (no thread writes it between the barrier before the scan and the one that ends it), so the choice is a uniform branch
  // and a skipped block costs neither LDS reads nor VALU work.  One instance of the pass per number of blocks.
  auto pass = [&](auto nb_tag) {
    constexpr int NB = decltype(nb_tag)::value;
    unsigned long long q[NB]; uint32_t e[NB]; double sl[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) { const uint32_t i = own + (uint32_t)j * kGreedyThreads; q[j] = w.seq[i]; e[j] = w.e[i]; sl[j] = w.sal[i]; }
    const uint4 ka = *reinterpret_cast<const uint4*>(&b.kill[0]), kb = *reinterpret_cast<const uint4*>(&b.kill[4]);   // [R:kill]
    const uint32_t kl[8] = {ka.x, ka.y, ka.z, ka.w, kb.x, kb.y, kb.z, kb.w};
    SCAN_T(0);
    // deaths: branch-free for the first eight (a short-circuit || / && chain compiles to one branch per term), a uniform
    // loop over the rest of the list, and -- only when the list overflowed -- a look at the edge records
    uint32_t deadm[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      uint32_t d = 0;
#pragma unroll
      for (uint32_t t = 0; t < 8; ++t) d |= (uint32_t)(t < nk) & (uint32_t)(kl[t] == e[j]);
      deadm[j] = d;
    }
    if (nk > 8u) {                                                       // (uniform)
      for (uint32_t t = 8; t < nk; ++t) {
        const uint32_t kt = b.kill[t];
#pragma unroll
        for (int j = 0; j < NB; ++j) deadm[j] |= (uint32_t)(kt == e[j]);
      }
      if (kovf) {                                                        // more deaths than the list holds (rare): ask the edge records
        full_barrier();                                                  // (the stores that mark them are performed)   // [B:kovf]
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          const uint32_t i = own + (uint32_t)j * kGreedyThreads;
          if (i < n && q[j] != 0) deadm[j] |= (uint32_t)(st.er[e[j]].seq == 0);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const uint32_t i = own + (uint32_t)j * kGreedyThreads;
      const bool was = (i < n) & (q[j] != 0);
      const bool live = was & (deadm[j] == 0u);
      if (was & !live) w.seq[i] = 0;
      Key c; c.sal = live ? sl[j] : -__builtin_inf(); c.seq = live ? q[j] : 0ull; c.arg = i;
      const bool b1 = better(c, k1), b2 = better(c, k2);
      // new best: the old best becomes second; else new second if it beats the old second (field by field: selecting whole
      // structs goes through private memory)
      k2.sal = b1 ? k1.sal : (b2 ? c.sal : k2.sal); k2.seq = b1 ? k1.seq : (b2 ? c.seq : k2.seq); k2.arg = b1 ? k1.arg : (b2 ? c.arg : k2.arg);
      k1.sal = b1 ? c.sal : k1.sal; k1.seq = b1 ? c.seq : k1.seq; k1.arg = b1 ? c.arg : k1.arg;
    }
  };
  static_assert(kWinPer == 3, "batch_scan: one pass instance per number of blocks");
  const uint32_t nu = (uint32_t)__builtin_amdgcn_readfirstlane((int)n);   // [R:fill]
  if (nu > 2u * kGreedyThreads) pass(std::integral_constant<int, 3>{});
  else if (nu > kGreedyThreads) pass(std::integral_constant<int, 2>{});
  else pass(std::integral_constant<int, 1>{});
  SCAN_T(1);
  // The wave's best and second-best in ONE reduction: a butterfly over the (best, second) pair of saliency images per lane
  // (wave_top2_ord), then a ballot for each of the two: a saliency that only one candidate holds names the winner's lane, whose
  // key (seq, arg) is fetched with v_readlane.  Candidates for the second place: every lane's best but the winner's, and the
  // winner's second.  A saliency several live candidates share (exact ties: common, the saliencies are means of 8-bit
  // values) is decided by seq in one more reduction (uniform branches).  Live items have distinct seqs; empty keys (seq 0)
  // are all (-inf, 0, 0): any of them is the answer.
  const int lane = tid & 63;
  const unsigned long long o1 = f64_ord(k1.sal), o2 = f64_ord(k2.sal);
  unsigned long long M1 = o1, M2 = o2;
  wave_top2_ord(M1, M2);
  const unsigned long long t1 = __ballot(o1 == M1), t1l = __ballot((o1 == M1) & (k1.seq != 0ull));
  const int l1 = (int)__builtin_ctzll(t1);                               // (some lane holds the maximum)
  const bool win1 = lane == l1;
  Key kk; kk.sal = win1 ? k2.sal : k1.sal; kk.seq = win1 ? k2.seq : k1.seq; kk.arg = win1 ? k2.arg : k1.arg;
  const unsigned long long oc = win1 ? o2 : o1;
  const unsigned long long t2 = __ballot(oc == M2), t2l = __ballot((oc == M2) & (kk.seq != 0ull));
  Key m1, m2;
  if (__popcll(t1) == 1 || t1l == 0ull) {                                // (uniform) one lane holds the largest saliency, or no lane a live item
    m1 = lane_key(k1, l1);
    int src = (int)__builtin_ctzll(t2);
    if (__popcll(t2) != 1 && t2l != 0ull) {                              // (uniform) live candidates share the second saliency: the largest seq
#ifdef GLIA_HMT_PROFILE
      if (tid == 0) g_scanprof[5] += 1;
#endif
      const unsigned long long ms = wave_max_u64(oc == M2 ? kk.seq : 0ull);
      src = (int)__builtin_ctzll(__ballot((oc == M2) & (kk.seq == ms)));
    }
    m2 = lane_key(kk, src);
    SCAN_T(2);
  } else {
    // (uniform) several live bests share the largest saliency, so the second place has it too: the two largest seqs among the
    // items of that saliency decide both (a lane's best has the larger seq of its two when they tie: s1 >= s2 holds)
#ifdef GLIA_HMT_PROFILE
    if (tid == 0) g_scanprof[6] += 1;
#endif
    unsigned long long S1 = o1 == M1 ? k1.seq : 0ull, S2 = o2 == M1 ? k2.seq : 0ull;
    wave_top2_ord(S1, S2);
    const int w1 = (int)__builtin_ctzll(__ballot((o1 == M1) & (k1.seq == S1)));
    const bool winr = lane == w1;
    Key kc; kc.sal = winr ? k2.sal : k1.sal; kc.seq = winr ? k2.seq : k1.seq; kc.arg = winr ? k2.arg : k1.arg;
    const unsigned long long occ = winr ? o2 : o1;
    m1 = lane_key(k1, w1);
    m2 = lane_key(kc, (int)__builtin_ctzll(__ballot((occ == M1) & (kc.seq == S2))));
    SCAN_T(3);
  }
  if ((tid & 63) == 0) { b.part1[tid >> 6] = m1; b.part2[tid >> 6] = m2; }   // [W:part12]
  full_barrier();                  // ... and are performed here, before the next round loads the lists they rewrote   // [B:scan-end]
  SCAN_T(4);
  if (tid == 0) { b.nkill = 0; b.kovf = 0; b.truehit = 0; }   // [W:kill-clear]   // [W:truehit-clear]
}

#ifdef GLIA_HMT_PROFILE
__device__ unsigned long long g_wideprof[8];
__device__ unsigned long long g_edgeprof[3][2];           // created edges (narrow commit / wide on the LDS table / wide on the global marks) x (at or above the horizon / below it), cumulative
#define WIDE_T(i) do { if (tid == 0) { const unsigned long long tn_ = __builtin_readcyclecounter(); g_wideprof[i] += tn_ - wt_; wt_ = tn_; } } while (0)
#else
#define WIDE_T(i) do {} while (0)
#endif
// The whole workgroup contracts ONE edge (more than kMemMax list entries): greedy_window_kernel's contraction, built from the same
// pieces (win_stage_lists .. win_retire_edge) with the batch policies -- spill instead of flush, horizon, no load in the store stream.
// LDS-table case (at most kMarkMax entries): the lists arrive in one round trip (win_stage_lists_small).
__device__ __forceinline__ uint32_t batch_contract_wide(const WinState& st, WinShared& w, WinWork& s, BatchShared& b, int tid, uint32_t slot, double rootsal,
                                                      unsigned long long k, unsigned long long ne, unsigned long long pool_used, double smin, double scale, uint32_t* newcount_out) {
  const uint32_t e = w.e[slot], r0 = w.u[slot], r1 = w.v[slot];
  const uint2 h0r = w.hu[slot], h1r = w.hv[slot];
  const uint32_t wn_now = w.n;
  const uint32_t off0 = h0r.x, len0 = h0r.y, off1 = h1r.x, len1 = h1r.y;
  const uint32_t total = len0 + len1;
  const uint32_t r2 = st.R0 + (uint32_t)k;
  const uint32_t r2off = (uint32_t)pool_used;
#ifdef GLIA_HMT_PROFILE
  unsigned long long wt_ = __builtin_readcyclecounter();
#endif
  lds_barrier();                                                        // every thread has read the slot   // [B:wide-enter]
  WIDE_T(0);
  if (tid == 0) {
    w.seq[slot] = 0;
    st.order[3 * k + 0] = r0; st.order[3 * k + 1] = r1; st.order[3 * k + 2] = r2;
    st.sal_out[k] = rootsal;
    st.er[e].seq = 0;
    st.rdead[r0] = 1; st.rdead[r1] = 1;
  }
  const bool small = total <= kMarkMax;
  if (small) win_stage_lists_small(st, s, tid, e, off0, len0, off1, len1); else win_stage_lists(st, s, tid, e, off0, len0, off1, len1, false);
  if (small) lds_barrier(); else full_barrier();      // (the global mark arrays are read by other threads below)   // [B:wide-lists]
  WIDE_T(1);
  if (wn_now + total > st.wcap && wn_now > st.wcap / 2u) win_compact(w, tid, st.wcap);      // (holes out; a full window spills, see win_evict)
  WIDE_T(2);
  const WinTau tau = {w.cthr, w.tsal, w.tseq, smin, scale};   // [R:tau]
  const uint32_t nwork = small ? s.nitems : total;   // [R:nitems]
  const uint32_t lenR2 = small ? nwork : 0u;        // small case: every table item becomes exactly one new edge, so r2's list length is known here
  bool bad = false;
  uint32_t pend_e = kNone, pend_old = kNone;
#ifdef GLIA_HMT_PROFILE
  uint32_t ep_above = 0, ep_below = 0;
#endif
  // Two instances of the loop: the LDS-table case must not share code with the one that loads from global memory -- where
  // the two meet the compiler waits for "every memory operation", and that counter includes the stores of earlier rounds.
  auto rounds = [&](auto small_tag) {
    constexpr bool SMALL = decltype(small_tag)::value;
    for (uint32_t base = 0; base < nwork; base += kGreedyThreads) {
      const uint32_t i = base + tid;
      if (i >= nwork) break;
      FatEntry f0, f1;
      bool h0, h1;
      uint32_t rs;
      if (!win_match<SMALL>(st, s, i, e, off0, len0, off1, &rs, &h0, &h1, &f0, &f1)) continue;
      const uint32_t idx = atomicAdd(&s.newcount, 1u);
      const uint32_t newE = (uint32_t)ne + idx;
      double first;
      int second;
      if (mean_link(h0, f0.mean, (int)f0.n, h1, f1.mean, (int)f1.n, &first, &second)) bad = true;
      const uint32_t offRs = f0.off, posRs = f0.pos, lenRs = f0.len;
      if (h0 && h1) st.fpool[offRs + f1.pos].eid = kNone;
      const unsigned long long seq = update_seq(k, rs, r0, h0);
      const double sal = -first;
      const uint32_t cell = win_cell(sal, tau.smin, tau.scale, st.wB);
#ifdef GLIA_HMT_PROFILE
      if (cell < st.wch) ++ep_below; else ++ep_above;
#endif
      store_new_edge<true>(st, newE, rs, r2, posRs, idx, first, second, sal, seq, offRs, lenRs, r2off, lenR2, cell);      // (wide case: r2's length is stored below)
      win_queue_edge<true>(st, w, tau, newE, sal, seq, rs, r2, make_uint2(offRs, lenRs), make_uint2(r2off, lenR2), cell, pend_e, pend_old);
      if (h0) win_retire_edge<true, false, kBatchKill>(st, tau, f0.eid, -f0.mean, &b.nkill, b.kill, &b.kovf);
      if (h1) win_retire_edge<true, false, kBatchKill>(st, tau, f1.eid, -f1.mean, &b.nkill, b.kill, &b.kovf);
    }
  };
  if (small) rounds(std::true_type{}); else rounds(std::false_type{});
  if (bad) b.bad = 1;
  WIDE_T(3);
  if (small) lds_barrier(); else full_barrier();      // (wide case: r2's new list entries are read back below, by other threads than wrote them)   // [B:wide-build]
  WIDE_T(4);
  const uint32_t newcount = s.newcount;   // [R:newcount]
  if (!small) win_complete_r2<true>(st, tid, (uint32_t)ne, r2off, newcount, smin, scale);
  if (!small) for (uint32_t i = tid; i < (w.n < st.wcap ? w.n : st.wcap); i += kGreedyThreads) if (w.v[i] == r2) w.hv[i].y = newcount;      // window items of r2: its list length
  if (pend_e != kNone) st.er[pend_e].next = pend_old;
  if (tid == 0) { st.adj_off[r2] = r2off; st.adj_len[r2] = newcount; }
  lds_barrier();                   // (the scan that follows ends with the full barrier)   // [B:wide-end]
  WIDE_T(5);
#ifdef GLIA_HMT_PROFILE
  if (ep_above) atomicAdd(&g_edgeprof[small ? 1 : 2][0], (unsigned long long)ep_above);
  if (ep_below) atomicAdd(&g_edgeprof[small ? 1 : 2][1], (unsigned long long)ep_below);
#endif
  if (tid == 0) { s.nitems = 0; s.newcount = 0; }   // [W:wide-clear]
  *newcount_out = newcount;
  return total;
}

__global__ __launch_bounds__(kGreedyThreads) void greedy_batch_kernel(WinState st) {
  __shared__ WinShared w;
  __shared__ WinWork s;
  __shared__ BatchShared b;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned long long k = st.ctrl[CTRL_MERGES], ne = st.ctrl[CTRL_EDGES], pool_used = st.ctrl[CTRL_ENTRIES];
  uint32_t status = ST_RUN;
  win_enter(st, w, s, tid);
  if (tid == 0) { b.nkill = 0; b.kovf = 0; b.bad = 0; b.truehit = 0; }
  b.bitmap[wave][lane] = 0;
  if (tid < kNW) { Key z; z.sal = -__builtin_inf(); z.seq = 0; z.arg = 0; b.part1[tid] = z; b.part2[tid] = z; }
  full_barrier();   // [B:enter]
  const double smin = st.wrange[0], scale = st.wrange[1];
  uint32_t pend_e = kNone, pend_old = kNone;          // (per lane) a list push whose link is stored a round later
  constexpr uint32_t kTab = kMarkSlots / kNW;         // private neighbour table of a wave
  uint32_t* const tk = &s.mk[wave * kTab]; uint32_t* const t0 = &s.mv0[wave * kTab]; uint32_t* const t1 = &s.mv1[wave * kTab];
  // ... and what a slot's (r1, rs) entry carries for the lane that owns the (r0, rs) entry; lives in the staging area of
  // the whole-workgroup path (never active at the same time)
  static_assert(sizeof(s.stage) >= (size_t)kNW * kTab * 20, "per-wave staging");
  uint32_t* const sg_eid = reinterpret_cast<uint32_t*>(&s.stage[0]) + wave * kTab;
  uint32_t* const sg_n = reinterpret_cast<uint32_t*>(&s.stage[0]) + (kNW + wave) * kTab;
  uint32_t* const sg_pos = reinterpret_cast<uint32_t*>(&s.stage[0]) + (2 * kNW + wave) * kTab;
  double* const sg_mean = reinterpret_cast<double*>(reinterpret_cast<uint32_t*>(&s.stage[0]) + 3 * kNW * kTab) + wave * kTab;
#ifdef GLIA_HMT_PROFILE
  unsigned long long bph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, blast = __builtin_readcyclecounter(), brounds = 0, bmembers = 0, bvalid = 0, bwide = 0, bcut_sal = 0;
  // rounds whose committed prefix ends at a wide member / at a true conflict / at a bitmap hit that is none; rounds with a flagged pair;
  // rounds in which the bitmap alone ends the prefix early; members the committed prefix is shorter by than the exact one
  unsigned long long bcut_wide = 0, bcut_true = 0, bcut_false = 0, bflag = 0, bcut_falsebm = 0, blost = 0;
  unsigned long long bw_n[4] = {0, 0, 0, 0}, bw_cyc[4] = {0, 0, 0, 0}, bw_ent[4] = {0, 0, 0, 0}, bw_new[4] = {0, 0, 0, 0};
  uint32_t bep_above = 0, bep_below = 0;                        // (per thread) edges this thread's commits created at or above / below the horizon
  unsigned long long bsel[2] = {0, 0}, bsel_n[2] = {0, 0};      // loop-top cycles (the select bucket, BPH(0)) of narrow rounds / wide pops, and their number
#define BPH0(wide) do { if (tid == 0) { unsigned long long tn = __builtin_readcyclecounter(); bph[0] += tn - blast; bsel[wide] += tn - blast; bsel_n[wide] += 1; blast = tn; } } while (0)
#define BPH(i) do { if (tid == 0) { unsigned long long tn = __builtin_readcyclecounter(); bph[i] += tn - blast; blast = tn; } } while (0)
#else
#define BPH(i) do {} while (0)
#define BPH0(wide) do {} while (0)
#endif

  for (unsigned long long it = 0; it < st.max_iters; ++it) {
    // lists grow garbage (dead nodes are only dropped when their cell is loaded): time for a new baseline?
    if (ne - st.ne_base > st.rebase_after) { status = ST_REBASE; break; }
    // ---- the exact top of the queue, in order: per-wave bests that beat every per-wave second-best ----
    const int gi = lane >> 3, gj = lane & 7;                             // an 8 x 8 grid of (i, j) comparisons per wave
    const Key A = b.part1[gi], B = b.part1[gj], C = b.part2[gi];   // [R:parts]
    const unsigned long long beats = __ballot(better(A, B)), under = __ballot(better(C, B));
    const unsigned long long col = 0x0101010101010101ull << gj;
    const uint32_t rank = (uint32_t)__popcll(beats & col);               // position of candidate gj in the order
    const bool cand_ok = B.seq != 0 && (under & col) == 0;               // it beats every second-best: part of the exact top
    if (gi == 0 && cand_ok) b.byrank[rank] = (uint32_t)gj;               // (every wave writes the same values)   // [W:byrank]
    const unsigned long long okmask = __ballot(gi == 0 && cand_ok);      // (bit j = candidate j)
    const uint32_t M = (uint32_t)__popcll(okmask);
    if (M == 0) {
      // no live item in the window
      BPH(5);
      if (pend_e != kNone) { st.er[pend_e].next = pend_old; pend_e = kNone; }
      if (st.force_tree && k >= st.force_tree) { status = ST_NEED_TREE; break; }
      const int r = win_reload(st, w, tid, reinterpret_cast<double*>(&s.stage[0]), reinterpret_cast<unsigned long long*>(&s.stage[0]) + kSelMax);
      BPH(6);
      if (r == 1) { status = ST_DONE; break; }
      if (r == 2) { status = ST_NEED_TREE; break; }
      if (r == 3) { status = ST_REBASE; break; }                          // the queue continues below the horizon: new baseline
      batch_scan(st, w, b, tid, kScanOther);
      continue;
    }
    // the candidate this wave is responsible for: the one of rank `wave`
    const unsigned long long minemask = __ballot(gi == 0 && cand_ok && rank == (uint32_t)wave);
    const bool member = minemask != 0;                                   // (uniform per wave)
    const int cj = member ? (int)__builtin_ctzll(minemask) : 0;
    const Key me = b.part1[cj];   // [R:me]
    const uint32_t slot = me.arg;
    // member data (every wave reads its own; waves without a member read a harmless slot)
    const uint32_t e = w.e[slot], r0 = w.u[slot], r1 = w.v[slot];
    const uint2 h0r = w.hu[slot], h1r = w.hv[slot];
    const uint32_t off0 = h0r.x, len0 = h0r.y, off1 = h1r.x, len1 = h1r.y;
    const uint32_t total = len0 + len1;
    if (k >= (unsigned long long)st.R0) { status = ST_INTERNAL; break; }      // more merges than regions: the state is corrupt
    // the best candidate decides: wide -> the whole workgroup takes it alone
    const unsigned long long firstmask = __ballot(gi == 0 && cand_ok && rank == 0u);
    const Key top = b.part1[__builtin_ctzll(firstmask)];
    const uint2 th0 = w.hu[top.arg], th1 = w.hv[top.arg];
    const uint32_t top_total = th0.y + th1.y;
    BPH0(top_total > kMemMax ? 1 : 0);
    if (top_total > kMemMax) {
      if (ne + top_total > st.Ecap) { status = ST_NEED_EDGES; break; }
      if (pool_used + top_total > st.pool_cap) { status = ST_NEED_POOL; break; }
      uint32_t newcount = 0;
#ifdef GLIA_HMT_PROFILE
      const unsigned long long tw0 = __builtin_readcyclecounter();
#endif
      const uint32_t tt = batch_contract_wide(st, w, s, b, tid, top.arg, top.sal, k, ne, pool_used, smin, scale, &newcount);
      if (b.bad) { status = ST_BAD_SALIENCY; break; }   // [R:wide-bad]
      k += 1; ne += newcount; pool_used += tt;
#ifdef GLIA_HMT_PROFILE
      bwide += 1;
      { const int cls = tt <= 512u ? 0 : tt <= kMarkMax ? 1 : tt <= 8192u ? 2 : 3; bw_n[cls] += 1; bw_cyc[cls] += __builtin_readcyclecounter() - tw0; bw_ent[cls] += tt; bw_new[cls] += newcount; }
#endif
      batch_scan(st, w, b, tid, kScanWide);
      if (w.spill_ord) { if (pend_e != kNone) { st.er[pend_e].next = pend_old; pend_e = kNone; } win_evict(st, w, tid); batch_scan(st, w, b, tid, kScanOther); }   // [R:spill-wide]
      BPH(4);
      continue;
    }
    // ---- compute: wave j works out member j (rank order) on its own, up to kMemP list entries per lane; wider members end the batch ----
    const bool narrow = member && total <= kMemMax;
    b.bitmap[wave][lane] = 0;   // [W:bitmap-clear]
    // The member's list in one round trip: every lane loads kMemP entries back to back -- a lane past the end (and a wave without a narrow
    // member, whose slot may hold anything) loads the pool's first entry instead of branching round the load -- and "not in the list" is
    // a select once the data is there.  (A load inside `if (inlist)` ended in a wait of its own: two or three dependent round trips for
    // a member of more than 64 entries.)
    FatEntry fe[kMemP];
    FatHalves fh[kMemP];
    bool act[kMemP], side1[kMemP];
    uint32_t h[kMemP];
#pragma unroll
    for (int p = 0; p < kMemP; ++p) {
      const uint32_t i = (uint32_t)lane + 64u * (uint32_t)p;
      act[p] = narrow && i < total;
      side1[p] = i >= len0;
      fh[p] = fat_load(&st.fpool[act[p] ? (side1[p] ? off1 + (i - len0) : off0 + i) : 0u]);
    }
    static_assert(kMemP == 3, "fat_pin");
    fat_pin(fh);
#pragma unroll
    for (int p = 0; p < kMemP; ++p) {
      const bool in = act[p];
      fe[p].eid = in ? fh[p].lo.x : kNone; fe[p].rs = in ? fh[p].lo.y : 0u; fe[p].n = in ? fh[p].lo.z : 0u; fe[p].pos = in ? fh[p].lo.w : 0u;
      fe[p].off = in ? fh[p].hi.x : 0u; fe[p].len = in ? fh[p].hi.y : 0u; fe[p].mean = in ? fat_mean(fh[p]) : 0.0;
    }
    if (pend_e != kNone) { st.er[pend_e].next = pend_old; pend_e = kNone; }      // (last round's atomic has returned with these loads)
#pragma unroll
    for (int p = 0; p < kMemP; ++p) {
      act[p] = act[p] && fe[p].eid != e && fe[p].eid != kNone;
      h[p] = (fe[p].rs * 2654435761u) >> 24;
      if (act[p]) {
        while (true) {
          const uint32_t old = atomicCAS(&tk[h[p]], 0u, fe[p].rs + 1u);
          if (old == 0u || old == fe[p].rs + 1u) break;
          h[p] = (h[p] + 1u) & (kTab - 1u);
        }
        if (side1[p]) {                                  // the (r1, rs) entry: its data waits in the table for the (r0, rs) entry's lane
          t1[h[p]] = 1u;
          sg_eid[h[p]] = fe[p].eid; sg_n[h[p]] = fe[p].n; sg_pos[h[p]] = fe[p].pos; sg_mean[h[p]] = fe[p].mean;
        } else t0[h[p]] = 1u;
        atomicOr(&b.bitmap[wave][(fe[p].rs >> 5) & 63u], 1u << (fe[p].rs & 31u));
      }
    }
    if (narrow && lane == 0) { atomicOr(&b.bitmap[wave][(r0 >> 5) & 63u], 1u << (r0 & 31u)); atomicOr(&b.bitmap[wave][(r1 >> 5) & 63u], 1u << (r1 & 31u)); }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                   // (a wave's LDS operations execute in order)
    bool owner[kMemP], both[kMemP];
    uint32_t p_eid[kMemP], p_n[kMemP], p_pos[kMemP];
    double p_mean[kMemP];
#pragma unroll
    for (int p = 0; p < kMemP; ++p) {
      const uint32_t m0 = act[p] ? t0[h[p]] : 0u, m1 = act[p] ? t1[h[p]] : 0u;
      owner[p] = act[p] && (!side1[p] || m0 == 0u);
      both[p] = owner[p] && !side1[p] && m1 != 0u;
      p_eid[p] = sg_eid[h[p]]; p_n[p] = sg_n[h[p]]; p_pos[p] = sg_pos[h[p]]; p_mean[p] = sg_mean[h[p]];
    }
#pragma unroll
    for (int p = 0; p < kMemP; ++p) if (act[p]) { tk[h[p]] = 0u; t0[h[p]] = 0u; t1[h[p]] = 0u; }      // the table is clean again
    double first[kMemP]; int second[kMemP]; uint32_t idx[kMemP];
    bool bad = false;
    uint32_t newcount = 0;
    double mx = -__builtin_inf();
#pragma unroll
    for (int p = 0; p < kMemP; ++p) {
      const bool h0 = owner[p] && !side1[p], h1 = owner[p] && (side1[p] || both[p]);
      // (a lane that owns nothing has h0 = h1 = false: its mean is sdivide's default 0, never the DUMMY)
      bad = mean_link(h0, fe[p].mean, (int)fe[p].n, h1, both[p] ? p_mean[p] : fe[p].mean, both[p] ? (int)p_n[p] : (int)fe[p].n, &first[p], &second[p]) || bad;
      const double f = first[p];
      const unsigned long long ownmask = __ballot(owner[p]);
      idx[p] = newcount + (uint32_t)__popcll(ownmask & ((1ull << lane) - 1ull));
      newcount += (uint32_t)__popcll(ownmask);
      mx = (owner[p] && -f > mx) ? -f : mx;              // the largest saliency this member creates
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const double o = __shfl_xor(mx, d); mx = o > mx ? o : mx; }
    if (lane == 0) { b.m_newcount[wave] = narrow ? newcount : 0u; b.m_total[wave] = narrow ? total : 0xFFFFFFFFu; b.m_maxsal[wave] = mx; }   // [W:member]
    if (bad) b.bad = 1;
    // the window's fill, read by every wave BEFORE the barrier: behind it the committing waves raise w.n, and the "compact first?" test below
    // has to come out the same in every wave (it guards barriers) -- on its own late read of w.n a slow wave could take the branch alone
    const uint32_t wn_round = w.n;   // [R:wn-round]
    lds_barrier();                 // (LDS data only; the round's global stores are waited for at the END of the scan that follows the commit)   // [B:compute]
    BPH(1);
    if (b.bad) { status = ST_BAD_SALIENCY; break; }   // [R:bad]
    // ---- validate: the longest prefix of the batch whose order is certain (lane j checks member j) ----
    uint32_t V, ne_off, pool_off, my_ne, my_pool;
    {
      const uint32_t j = (uint32_t)lane & 7u;
      const Key kj = b.part1[b.byrank[j]];   // [R:byrank]
      const uint32_t u = w.u[kj.arg], v = w.v[kj.arg];
      const uint32_t tj = b.m_total[j], nj = b.m_newcount[j];   // [R:members]
      double pm = -__builtin_inf();
      uint32_t hitm = 0, pre_n = 0, pre_t = 0;                             // hitm, bit i: u or v is in the bitmap of member i (< j)
#pragma unroll
      for (uint32_t i = 0; i < (uint32_t)kNW; ++i) {
        const double ms = b.m_maxsal[i];
        const uint32_t bu = b.bitmap[i][(u >> 5) & 63u], bv = b.bitmap[i][(v >> 5) & 63u];   // [R:bitmap]
        const uint32_t ti = b.m_total[i], ni = b.m_newcount[i];
        if (i < j) { pm = ms > pm ? ms : pm; hitm |= (((bu >> (u & 31u)) | (bv >> (v & 31u))) & 1u) << i; pre_n += ni; pre_t += ti; }
      }
      // rule (a) and the wide-member cut alone bound the prefix: only pairs (i, j) below that bound can matter
      const bool oka = j < M && tj != 0xFFFFFFFFu && (j == 0u || kj.sal > pm);
      const uint32_t Va = (uint32_t)__builtin_ctz(~(uint32_t)(__ballot(lane < kNW && oka) & 0xFFull));
      // Rule (b): the bitmap is the cheap filter (ids mod 2048: a hit may come from another id of the same residue), the wave of the
      // earlier member decides a flagged pair exactly.  Every wave has computed the same hitm from the same LDS words -- all of them
      // written in front of [B:compute] and none rewritten before [B:commit] -- so `flagged` is the same in every wave of the
      // workgroup, and the branch below, which holds a barrier, is uniform (as the "compact first?" test is by [R:wn-round]).
      const uint32_t flagged = (uint32_t)__ballot(lane < (int)Va && hitm != 0u);      // (Va <= 8: lane = j there)
      uint32_t th = 0;
      if (flagged) {
        // Wave i holds member i (narrow: i < Va) and answers for every flagged j > i from its registers: fe[p].rs under act[p] is exactly
        // what it entered into its bitmap (live entries: not the contracted edge, no tombstones), besides its own r0 and r1.
        const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane(wave);
        uint32_t mine = 0;
        for (uint32_t jj = wv + 1u; jj < Va; ++jj) {
          if (((uint32_t)__builtin_amdgcn_readlane((int)hitm, (int)jj) >> wv & 1u) == 0u) continue;
          const uint32_t uj = (uint32_t)__builtin_amdgcn_readlane((int)u, (int)jj), vj = (uint32_t)__builtin_amdgcn_readlane((int)v, (int)jj);
          bool c = (uj == r0) | (uj == r1) | (vj == r0) | (vj == r1);
#pragma unroll
          for (int p = 0; p < kMemP; ++p) c |= act[p] & ((fe[p].rs == uj) | (fe[p].rs == vj));
          if (__ballot(c) != 0ull) mine |= 1u << jj;
        }
        if (mine != 0u && lane == 0) atomicOr(&b.truehit, mine);   // [W:truehit]
        lds_barrier();   // [B:exact]
        th = b.truehit;   // [R:truehit]
      }
      const bool okj = oka && ((th >> j) & 1u) == 0u;
      V = (uint32_t)__builtin_ctz(~(uint32_t)(__ballot(lane < kNW && okj) & 0xFFull));      // members 0 .. V-1 are certain (no pair flagged: V = Va)
#ifdef GLIA_HMT_PROFILE
      {
        // what the bitmap alone would have committed (GLIA_HMT_BITMAP_PREFIX: it still does, the exact test only counts), and why the
        // committed prefix ends where it does
        const uint32_t Vb = (uint32_t)__builtin_ctz(~(uint32_t)(__ballot(lane < kNW && oka && hitm == 0u) & 0xFFull));
        const uint32_t Vx = V;
#ifdef GLIA_HMT_BITMAP_PREFIX
        V = Vb;
#endif
        if (flagged) bflag += 1;
        if (Vb < Vx) bcut_falsebm += 1;
        blost += Vx - V;
        if (V < M) {
          const uint32_t cutsal = (uint32_t)(__ballot(lane < kNW && j == V && !(kj.sal > pm)) & 0xFFull);
          const uint32_t cutwide = (uint32_t)(__ballot(lane < kNW && j == V && tj == 0xFFFFFFFFu) & 0xFFull);
          if (cutsal) bcut_sal += 1; else if (cutwide) bcut_wide += 1; else if ((th >> V) & 1u) bcut_true += 1; else bcut_false += 1;
        }
      }
#endif
      // offsets of this wave's member, totals of the valid prefix
      my_ne = (uint32_t)__builtin_amdgcn_readlane((int)pre_n, wave); my_pool = (uint32_t)__builtin_amdgcn_readlane((int)pre_t, wave);
      const uint32_t last = V - 1u;
      ne_off = (uint32_t)__shfl((int)(pre_n + nj), (int)last); pool_off = (uint32_t)__shfl((int)(pre_t + tj), (int)last);
    }
    const uint32_t sum_tot = pool_off;
    if (ne + sum_tot > st.Ecap) { status = ST_NEED_EDGES; break; }
    if (pool_used + sum_tot > st.pool_cap) { status = ST_NEED_POOL; break; }
    // room in the window for everything the batch may insert (the popped items leave first: a flush must not see them)
    bool popped = false;
    if (wn_round + ne_off > st.wcap && wn_round > st.wcap / 2u) {          // holes out (a full window spills, see win_evict)
      if ((uint32_t)wave < V && lane == 0) w.seq[slot] = 0;
      popped = true;                                                     // (slot numbers are void after a compaction)
      lds_barrier();   // [B:popped]
      win_compact(w, tid, st.wcap);
    }
    const WinTau tau = {w.cthr, w.tsal, w.tseq, smin, scale};   // [R:tau]
    BPH(2);
    // ---- commit: the valid members, each by its own wave ----
    if ((uint32_t)wave < V) {
      const unsigned long long kk = k + (unsigned long long)wave;
      const uint32_t r2 = st.R0 + (uint32_t)kk;
      const uint32_t r2off = (uint32_t)pool_used + my_pool;
      if (lane == 0) {
        if (!popped) w.seq[slot] = 0;                                    // popped
        st.order[3 * kk + 0] = r0; st.order[3 * kk + 1] = r1; st.order[3 * kk + 2] = r2;
        st.sal_out[kk] = me.sal;
        st.er[e].seq = 0;
        st.rdead[r0] = 1; st.rdead[r1] = 1;
        st.adj_off[r2] = r2off; st.adj_len[r2] = newcount;
      }
#pragma unroll
      for (int p = 0; p < kMemP; ++p) {
        if (!owner[p]) continue;
        const bool h0 = !side1[p];
        const uint32_t rs = fe[p].rs;
        const uint32_t newE = (uint32_t)ne + my_ne + idx[p];
        const uint32_t offRs = fe[p].off, posRs = fe[p].pos, lenRs = fe[p].len;   // rs's entry of the (r0,rs) edge -- or of (r1,rs) alone -- is reused
        if (both[p]) st.fpool[offRs + p_pos[p]].eid = kNone;             // rs held two entries: the other becomes a tombstone
        const unsigned long long seq = update_seq(kk, rs, r0, h0);
        const double sal = -first[p];
        const uint32_t cell = win_cell(sal, tau.smin, tau.scale, st.wB);
#ifdef GLIA_HMT_PROFILE
        if (cell < st.wch) ++bep_below; else ++bep_above;
#endif
        store_new_edge<true>(st, newE, rs, r2, posRs, idx[p], first[p], second[p], sal, seq, offRs, lenRs, r2off, newcount, cell);
        win_queue_edge<true>(st, w, tau, newE, sal, seq, rs, r2, make_uint2(offRs, lenRs), make_uint2(r2off, newcount), cell, pend_e, pend_old);
        // the replaced edges leave the queue: this lane's entry, and the (r1,rs) entry that waited in the table for it
        win_retire_edge<true, false, kBatchKill>(st, tau, fe[p].eid, -fe[p].mean, &b.nkill, b.kill, &b.kovf);
        if (both[p]) win_retire_edge<true, false, kBatchKill>(st, tau, p_eid[p], -p_mean[p], &b.nkill, b.kill, &b.kovf);
      }
    }
    lds_barrier();                   // the commit's global stores stay in flight through the scan ...   // [B:commit]
    BPH(3);
#ifdef GLIA_HMT_PROFILE
    brounds += 1; bmembers += M; bvalid += V;
#endif
    k += V; ne += ne_off; pool_used += pool_off;
    batch_scan(st, w, b, tid, kScanNarrow);
    if (w.spill_ord) { if (pend_e != kNone) { st.er[pend_e].next = pend_old; pend_e = kNone; } win_evict(st, w, tid); batch_scan(st, w, b, tid, kScanOther); }   // [R:spill]
    BPH(4);
  }
#ifdef GLIA_HMT_PROFILE
  if (bep_above) atomicAdd(&g_edgeprof[0][0], (unsigned long long)bep_above);
  if (bep_below) atomicAdd(&g_edgeprof[0][1], (unsigned long long)bep_below);
  full_barrier();
  if (tid == 0) printf("[batch profile] created edges at or above / below the horizon (cumulative): narrow commit %llu / %llu  wide on the LDS table %llu / %llu  wide on the global marks %llu / %llu\n",
                       atomicAdd(&g_edgeprof[0][0], 0ull), atomicAdd(&g_edgeprof[0][1], 0ull), atomicAdd(&g_edgeprof[1][0], 0ull), atomicAdd(&g_edgeprof[1][1], 0ull),
                       atomicAdd(&g_edgeprof[2][0], 0ull), atomicAdd(&g_edgeprof[2][1], 0ull));
  if (tid == 0) printf("[batch profile] merges %llu: select %llu  compute %llu  validate %llu  commit %llu  scan %llu  loop-top %llu  reload %llu (cycles); rounds %llu candidates %llu committed %llu (cut by saliency %llu, by a wide member %llu, by a true conflict %llu, by a false bitmap hit %llu) wide %llu\n",
                       k, bph[0], bph[1], bph[2], bph[3], bph[4], bph[5], bph[6], brounds, bmembers, bvalid, bcut_sal, bcut_wide, bcut_true, bcut_false, bwide);
  if (tid == 0) printf("[batch profile] conflicts (this launch): rounds with a flagged pair %llu  rounds the bitmap alone would cut short %llu  members lost to false cuts %llu;  scans with an overflowed kill list (cumulative) %llu\n",
                       bflag, bcut_falsebm, blost, g_kovf);
  if (tid == 0) printf("[batch profile] reload parts (cumulative cycles, thread 0): descent over blocks that load nothing %llu  whole-cell loads %llu  cell split %llu;  empty blocks %llu  reloads %llu\n",
                       g_reloadprof[0], g_reloadprof[1], g_reloadprof[2], g_reloadprof[3], g_reloadprof[4]);
  if (tid == 0) printf("[batch profile] scan phases (cumulative cycles, wave 0): loads %llu  compare %llu  top2 %llu  top2 with a tied best %llu  barrier %llu  calls %llu  tied second %llu  tied best %llu\n",
                       g_scanprof[0], g_scanprof[1], g_scanprof[2], g_scanprof[3], g_scanprof[4], g_scanprof[7], g_scanprof[5], g_scanprof[6]);
  if (tid == 0) printf("[batch profile] scan fill (cumulative; n <= 512, <= 1024, more): after reload/evict %llu %llu %llu  after narrow round %llu %llu %llu  after wide %llu %llu %llu\n",
                       g_scanfill[0][0], g_scanfill[0][1], g_scanfill[0][2], g_scanfill[1][0], g_scanfill[1][1], g_scanfill[1][2], g_scanfill[2][0], g_scanfill[2][1], g_scanfill[2][2]);
  if (tid == 0) printf("[batch profile] loop top (this launch): narrow rounds %llu cycles %llu  wide pops %llu cycles %llu\n", bsel_n[0], bsel[0], bsel_n[1], bsel[1]);
  if (tid == 0) printf("[batch profile] wide phases (cumulative cycles): entry-barrier %llu  lists+table %llu  compact %llu  main loop (wave 0) %llu  loop barrier %llu  tail %llu\n",
                       g_wideprof[0], g_wideprof[1], g_wideprof[2], g_wideprof[3], g_wideprof[4], g_wideprof[5]);
  if (tid == 0) printf("[batch profile] wide by entries (<=512, <=1408, <=8192, more): n %llu %llu %llu %llu  cycles %llu %llu %llu %llu  entries %llu %llu %llu %llu  new edges %llu %llu %llu %llu\n",
                       bw_n[0], bw_n[1], bw_n[2], bw_n[3], bw_cyc[0], bw_cyc[1], bw_cyc[2], bw_cyc[3], bw_ent[0], bw_ent[1], bw_ent[2], bw_ent[3], bw_new[0], bw_new[1], bw_new[2], bw_new[3]);
#endif
  if (pend_e != kNone) st.er[pend_e].next = pend_old;
  full_barrier();
  win_leave(st, w, tid, k, ne, pool_used, status);
}

}  // namespace
}  // namespace glia
