// glia_amd/csrc/greedy_tree.hpp -- the tournament-tree merge loop (greedy_pb_kernel): median linkages, GLIA_HMT_PB_WINDOW=0 and the
// hand-over from the window queue (ST_NEED_TREE).  Part of greedy.hip's translation unit.
//
// What the code below relies on:
//   * A queue item is a leaf of the tree: leaf_seq[e] == 0 means "edge e is not in the queue" (dead, popped, or rejected by the
//     pre_merge condition); its saliency never changes while it lives, so (seq, arg) identify a node's key.
//   * One workgroup, k / ne / pool_used / vals_used are PRIVATE copies in every thread: they advance by values every thread reads
//     from LDS (s.newcount, jobs.off) behind a barrier, and the word is rewritten only behind the NEXT barrier every reader
//     passes (audit table; tags [B:..] = barrier, [R:..] = read, [W:..] = rewrite).
//   * Thread 0 alone pops and decides (s.stop, s.reject); the Shared neighbour table is all zero between contractions.
//   * A barrier that hands GLOBAL data from one wave to another is full_barrier() (greedy_common.hpp), never __syncthreads().
#pragma once
#include "greedy_common.hpp"

namespace glia {

struct GreedyState {
  uint32_t R0;
  uint32_t* adj_off;   // [2*R0] start of a region's incident-edge list in pool
  uint32_t* adj_len;   // [2*R0] slots in that list (live edges + tombstones)
  uint2* pool;         // incident-edge lists: (edge slot | kNone tombstone, the neighbour it leads to)
  unsigned long long pool_cap;
  uint32_t Ecap;
  uint32_t *e_u, *e_v, *e_posu, *e_posv;
  double* e_mean;                 // mean linkage: boundary mean; median linkage: the current median
  int* e_n;
  // median linkage (util/struct_merge.hxx:90-136): every edge owns a SORTED run of its boundary values in `vals`
  float* vals;
  unsigned long long vals_cap;
  unsigned long long* e_off;      // [Ecap] start of the edge's run
  unsigned long long* rbv;        // [2*R0] values held by the region's incident edges (capacity pre-check)
  int size_weight;                // ...AndMinSize linkage (util/struct_merge.hxx:141-185): saliency = -median * min(region sizes)
  PqTree pq;
  // pre_merge condition (gadget/main_pre_merge.cxx:27-76); cond_n == 0: f_true
  int cond_n; unsigned long long cond_t0, cond_t1; double cond_rpb;
  unsigned long long* rsz;        // [2*R0] region sizes (updateRegion = true)
  double* rsum;                   // [2*R0] sum of pb over the region's voxels
  uint32_t *mark0, *mark1;        // [2*R0], zero between contractions
  uint32_t* order;                // [R0][3] dense ids
  double* sal_out;
  unsigned long long* ctrl;       // [CTRL_WORDS], see below
  unsigned long long max_iters;
};
// GreedyState::ctrl / WinState::ctrl: what a launch takes over from the previous one and hands back to the host
enum { CTRL_MERGES = 0, CTRL_EDGES = 1, CTRL_ENTRIES = 2,      // merges done, edge slots used, list entries used
       CTRL_STATUS = 3, CTRL_VALUES = 4,                       // ST_*; median linkage: values used
       CTRL_CTHR = 5, CTRL_TSAL = 6, CTRL_TSEQ = 7, CTRL_IPTR = 8,      // window queue: the threshold (cell, saliency bits, seq), consumed baseline entries
       CTRL_WERR = 9, CTRL_WFILL = 10, CTRL_WORDS = 11 };      // diagnostics of ST_INTERNAL: window overflow flag, window fill at exit

namespace {

// The mean linkage of the edge that replaces (r0,rs) and (r1,rs) (util/struct_merge.hxx:62-76): d2 = sdivide(m0*n0 + m1*n1, n0+n1, 0),
// the (r0,rs) item first, no FMA.  Returns whether the result is the reference's DUMMY, "invalid boundary saliency" (:78-79).
__device__ __forceinline__ bool mean_link(bool h0, double m0, int n0, bool h1, double m1, int n1, double* first, int* second) {
  double f = 0.0;
  int sc = 0;
  if (h0) { f += m0 * n0; sc += n0; }
  if (h1) { f += m1 * n1; sc += n1; }
  f = sdivide(f, (double)sc, 0.0);
  *first = f; *second = sc;
  return f == -1.0;
}
// The queue position of the edge (rs, r2) that merge number k creates: TBoundaryTable::update visits the neighbours rs < r0, then
// those of r0 above it, then those of r1 alone, each ascending (see greedy.hip's header)
__device__ __forceinline__ unsigned long long update_seq(unsigned long long k, uint32_t rs, uint32_t r0, bool h0) {
  const uint32_t cat = rs < r0 ? 0u : (h0 ? 1u : 2u);
  return ((k + 1ull) << 32) | ((unsigned long long)cat << 30) | rs;
}

constexpr uint32_t kMarkSlots = 2048;      // LDS neighbour table of one contraction
constexpr uint32_t kMarkMax = 1408;        // contractions with more incident entries use the global mark arrays
struct Shared {
  uint32_t r0, r1, e, stop, len0, len1, off0, off1, newcount, reject;
  PqWork pq;
  // neighbours of the contracted pair: key = neighbour + 1, values = (edge to r0) + 1, (edge to r1) + 1
  uint32_t mk[kMarkSlots], mv0[kMarkSlots], mv1[kMarkSlots];
  uint32_t items[kMarkMax], nitems;
};
constexpr uint32_t kMergeTile = 1024;      // outputs merged through LDS by one wave at a time
struct MedianJobs {               // median linkage: the value runs to merge in one batch of phase B
  uint32_t n;
  uint32_t newE[kGreedyThreads], e0[kGreedyThreads], e1[kGreedyThreads];
  unsigned long long off[kGreedyThreads + 1];    // output offset of job j (elements)
  uint32_t toff[kGreedyThreads + 1];             // first tile of job j
  uint32_t tjob[kGreedyThreads], ta0[kGreedyThreads], ta1[kGreedyThreads];   // tiles of the current round
  // the two input runs of job j (lengths, offsets in the value pool) and its median, kept here so that neither the tile
  // set-up nor the tiles nor the final pass go back to global memory for them
  uint32_t na[kGreedyThreads], nb[kGreedyThreads];
  unsigned long long oa[kGreedyThreads], ob[kGreedyThreads];
  float med[kGreedyThreads];
  float buf[kGreedyThreads / 64][2 * kMergeTile + 64];      // input pieces | output (padded: index + index / 16)
};
struct NoJobs {                   // mean linkage: never touched
  uint32_t n, newE[1], e0[1], e1[1], toff[2], tjob[1], ta0[1], ta1[1], na[1], nb[1];
  unsigned long long off[2], oa[1], ob[1];
  float med[1];
  float buf[kGreedyThreads / 64][2];
};

// number of elements of the sorted run a[0..n) that are < v (strict = true) or <= v
__device__ __forceinline__ uint32_t run_rank(const float* a, uint32_t n, float v, bool strict) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    const float x = a[mid];
    if (strict ? (x < v) : (x <= v)) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// merge path: how many elements of A are among the first d outputs of the stable merge (ties: A first)
__device__ __forceinline__ uint32_t merge_split(const float* A, uint32_t na, const float* B, uint32_t nb, uint32_t d) {
  uint32_t lo = d > nb ? d - nb : 0u, hi = d < na ? d : na;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (A[mid] <= B[d - 1u - mid]) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <bool MEDIAN>
__global__ __launch_bounds__(kGreedyThreads) void greedy_pb_kernel(GreedyState st) {
  __shared__ Shared s;
  __shared__ typename std::conditional<MEDIAN, MedianJobs, NoJobs>::type jobs;
  const int tid = threadIdx.x;
  unsigned long long k = st.ctrl[CTRL_MERGES], ne = st.ctrl[CTRL_EDGES], pool_used = st.ctrl[CTRL_ENTRIES], vals_used = st.ctrl[CTRL_VALUES];
  uint32_t status = ST_RUN;
  if (tid == 0) { s.pq.wln[0] = s.pq.wln[1] = 0; s.pq.ovf = 0; s.pq.spill = 0; s.nitems = 0; }
  for (int i = tid; i < kSetSlots; i += blockDim.x) { s.pq.set[0][i] = 0; s.pq.set[1][i] = 0; }
  for (uint32_t i = tid; i < kMarkSlots; i += blockDim.x) { s.mk[i] = 0; s.mv0[i] = 0; s.mv1[i] = 0; }
  const PqTree& pq = st.pq;
  // mean linkage: the last stored level of the tree (<= 4096 nodes) stays in LDS for the whole launch -- its nodes are
  // written by one step of the propagation and read by the next, which through global memory is a store round trip plus
  // a load round trip.  (The median kernel needs the LDS for its merge tiles.)
  constexpr uint32_t kTopLds = MEDIAN ? 1u : kTopMax;
  __shared__ Key s_topk[kTopLds];
  Key* topk = (!MEDIAN && pq.nlevels >= 2 && pq.lv[pq.nlevels - 1].size <= kTopLds) ? s_topk : nullptr;
  if (topk) pq_top_load<kGreedyThreads>(pq, topk, tid);
  full_barrier();
  pq_top<kGreedyThreads>(pq, s.pq, tid, topk);      // the root lives in LDS: rebuilt at every launch

#ifdef GLIA_HMT_PROFILE
  unsigned long long tph[6] = {0, 0, 0, 0, 0, 0}, tlast = __builtin_readcyclecounter();
  unsigned long long tb[4] = {0, 0, 0, 0}, nb[4] = {0, 0, 0, 0}, db[4] = {0, 0, 0, 0}, titer = tlast;
#define PH(i) do { if (tid == 0) { unsigned long long tn = __builtin_readcyclecounter(); tph[i] += tn - tlast; tlast = tn; } } while (0)
#else
#define PH(i) do {} while (0)
#endif
  for (unsigned long long it = 0; it < st.max_iters; ++it) {
    // ---- pop (TBoundaryTable::top) ----
    PH(5);
    if (tid == 0) {
      const Key root = pq_root<kGreedyThreads>(s.pq);
      s.stop = ST_RUN;   // [W:pop]
      s.newcount = 0;   // [W:newcount-clear]
      s.reject = 0;
      if (root.seq == 0) s.stop = ST_DONE;
      else {
        uint32_t e = root.arg;
        s.e = e; s.r0 = st.e_u[e]; s.r1 = st.e_v[e];
        if (st.cond_n > 0) {
          // TBoundaryTable::top(fcond) walks the queue from the best item down and returns the first one fcond accepts.
          // fcond depends only on the two regions, which cannot change while the item lives, so an item it rejects
          // is rejected for good: take it out of the queue (it stays in the table and is folded into later updates).
          unsigned long long sz0 = st.rsz[s.r0], sz1 = st.rsz[s.r1];
          double su0 = st.rsum[s.r0], su1 = st.rsum[s.r1];
          if (sz0 > sz1) { unsigned long long t = sz0; sz0 = sz1; sz1 = t; double d = su0; su0 = su1; su1 = d; }
          bool ok = sz0 < st.cond_t0;
          if (!ok && st.cond_n > 1) {
            if (sz0 < st.cond_t1 && sdivide(su0, (double)sz0, 0.0) > st.cond_rpb) ok = true;
            if (!ok && sz1 < st.cond_t1 && sdivide(su1, (double)sz1, 0.0) > st.cond_rpb) ok = true;
          }
          if (!ok) { s.reject = 1; pq.leaf_seq[e] = 0; pq_touch(pq, s.pq, 0, 0, e); /* e is the root, hence the maximum of its level-0 node */ }
        }
        // one round trip for everything the two regions contribute (loads first: they would queue behind the stores)
        const uint32_t len0 = st.adj_len[s.r0], len1 = st.adj_len[s.r1], off0 = st.adj_off[s.r0], off1 = st.adj_off[s.r1];
        const unsigned long long z0 = st.rsz[s.r0], z1 = st.rsz[s.r1];
        const double w0 = st.rsum[s.r0], w1 = st.rsum[s.r1];
        const unsigned long long b0 = MEDIAN ? st.rbv[s.r0] : 0ull, b1 = MEDIAN ? st.rbv[s.r1] : 0ull;
        const int en = MEDIAN ? st.e_n[e] : 0;
        s.len0 = len0; s.len1 = len1; s.off0 = off0; s.off1 = off1;
        unsigned long long tot = (unsigned long long)len0 + len1;
        if (s.reject) {}      // nothing is contracted: no capacity needed
        else if (ne + tot > st.Ecap) s.stop = ST_NEED_EDGES;
        else if (pool_used + tot > st.pool_cap) s.stop = ST_NEED_POOL;
        else if (MEDIAN && vals_used + b0 + b1 > st.vals_cap) s.stop = ST_NEED_VALUES;
        else {
          if (MEDIAN) st.rbv[st.R0 + (uint32_t)k] = b0 + b1 - 2ull * (unsigned long long)en;
          st.order[3 * k + 0] = s.r0; st.order[3 * k + 1] = s.r1; st.order[3 * k + 2] = st.R0 + (uint32_t)k;
          st.sal_out[k] = root.sal;
          st.rsz[st.R0 + (uint32_t)k] = z0 + z1;       // TRegionMap::merge (updateRegion)
          st.rsum[st.R0 + (uint32_t)k] = w0 + w1;
        }
      }
    }
    full_barrier();   // [B:pop]
    PH(0);
    if (s.stop != ST_RUN) { status = s.stop; break; }   // [R:pop]
    if (s.reject) { pq_propagate<kGreedyThreads>(pq, s.pq, tid, topk); continue; }
    const uint32_t r0 = s.r0, e = s.e, len0 = s.len0, len1 = s.len1, off0 = s.off0, off1 = s.off1;
    const uint32_t r2 = st.R0 + (uint32_t)k;
    const uint32_t total = len0 + len1;
    const uint32_t r2off = (uint32_t)pool_used;
    const bool small = total <= kMarkMax;          // the usual case: neighbour matching entirely in LDS

    // ---- phase A: one table entry per distinct neighbour, holding the edge(s) that reach it ----
    for (uint32_t i = tid; i < total; i += kGreedyThreads) {
      const bool side1 = i >= len0;
      const uint2 pe = st.pool[side1 ? off1 + (i - len0) : off0 + i];
      const uint32_t eid = pe.x, rs = pe.y;
      if (eid == e || eid == kNone) continue;        // the contracted edge / the dead twin of an earlier contraction
      if (small) {
        uint32_t h = (rs * 2654435761u) >> 21;
        while (true) {
          const uint32_t old = atomicCAS(&s.mk[h], 0u, rs + 1u);
          if (old == 0u) { s.items[atomicAdd(&s.nitems, 1u)] = h; break; }
          if (old == rs + 1u) break;
          h = (h + 1u) & (kMarkSlots - 1u);
        }
        (side1 ? s.mv1 : s.mv0)[h] = eid + 1u;
      } else (side1 ? st.mark1 : st.mark0)[rs] = eid + 1u;
    }
    full_barrier();   // [B:phaseA]
    PH(1);

    // ---- phase B: one new edge (rs, r2) per distinct neighbour (TBoundaryTable::update) ----
    bool bad = false;
    const uint32_t nwork = small ? s.nitems : total;   // [R:nitems]
    for (uint32_t base = 0; base < nwork; base += kGreedyThreads) {
      if (MEDIAN) { if (tid == 0) jobs.n = 0; full_barrier(); }   // [W:jobs-n]
      const uint32_t i = base + tid;
      do {
        if (i >= nwork) break;
        uint32_t rs, e0s, e1s;
        if (small) {
          const uint32_t h = s.items[i];
          rs = s.mk[h] - 1u;
          const uint32_t m0 = s.mv0[h], m1 = s.mv1[h];
          e0s = m0 ? m0 - 1u : kNone; e1s = m1 ? m1 - 1u : kNone;
          s.mk[h] = 0u; s.mv0[h] = 0u; s.mv1[h] = 0u;          // the table is clean again when the phase ends
        } else {
          const bool side1 = i >= len0;
          const uint2 pe = st.pool[side1 ? off1 + (i - len0) : off0 + i];
          const uint32_t eid = pe.x;
          rs = pe.y;
          if (eid == e || eid == kNone) break;
          if (!side1) {
            e0s = eid;
            const uint32_t m = st.mark1[rs];
            e1s = m ? m - 1u : kNone;
          } else {
            if (st.mark0[rs] != 0u) break;             // common neighbour: handled from the r0 side
            e0s = kNone; e1s = eid;
          }
        }
        const uint32_t idx = atomicAdd(&s.newcount, 1u);
        const uint32_t newE = (uint32_t)ne + idx;
        // Everything this record reads, requested up front and UNCONDITIONALLY (a missing side re-reads the other side's
        // slot): a load inside a branch gets its own basic block and its own s_waitcnt, i.e. its own memory round trip,
        // and a wave's loads queue behind its own earlier stores (vmcnt is in order).
        const bool h0 = e0s != kNone, h1 = e1s != kNone;
        const uint32_t a0 = h0 ? e0s : e1s, a1 = h1 ? e1s : e0s;
        const uint32_t u0 = st.e_u[a0], pu0 = st.e_posu[a0], pv0 = st.e_posv[a0];
        const uint32_t u1 = st.e_u[a1], pu1 = st.e_posu[a1], pv1 = st.e_posv[a1];
        const uint32_t offRs = st.adj_off[rs];
        const unsigned long long q0 = pq.leaf_seq[a0], q1 = pq.leaf_seq[a1];
        const uint32_t t0 = pq.lv[0].arg[a0 / kFan], t1 = pq.lv[0].arg[a1 / kFan];
        const int n0 = st.e_n[a0], n1 = st.e_n[a1];
        const double m0 = st.e_mean[a0], m1 = st.e_mean[a1];
        const unsigned long long eoff = MEDIAN ? st.e_off[a0] : 0ull, eoff1 = MEDIAN ? st.e_off[a1] : 0ull;
        const uint32_t posRs = (u0 == rs) ? pu0 : pv0;
        const unsigned long long seq0 = h0 ? q0 : 0ull, seq1 = h1 ? q1 : 0ull;
        const uint32_t top0 = h0 ? t0 : kNone, top1 = h1 ? t1 : kNone;
        const uint32_t pos1 = (h0 && h1) ? ((u1 == rs) ? pu1 : pv1) : kNone;
        double first = 0.0;
        int second = 0;
        if (!MEDIAN) {
          if (mean_link(h0, m0, n0, h1, m1, n1, &first, &second)) bad = true;
        } else {
          // util/struct_merge.hxx:118-127: the value lists are spliced; one list alone is moved (its run is reused)
          if (h0) second += n0;
          if (h1) second += n1;
          if (h0 && h1) {
            const uint32_t j = atomicAdd(&jobs.n, 1u);
            jobs.newE[j] = newE; jobs.e0[j] = e0s; jobs.e1[j] = e1s;
            jobs.na[j] = (uint32_t)n0; jobs.nb[j] = (uint32_t)n1; jobs.oa[j] = eoff; jobs.ob[j] = eoff1;
          } else { first = m0; st.e_off[newE] = eoff; }
        }
        // rs held two entries (to r0 and to r1): one is reused for the new edge, the other becomes a tombstone
        if (pos1 != kNone) st.pool[offRs + pos1] = make_uint2(kNone, 0u);
        const unsigned long long seq = update_seq(k, rs, r0, h0);
        st.e_u[newE] = rs; st.e_v[newE] = r2; st.e_posu[newE] = posRs; st.e_posv[newE] = idx;
        st.e_mean[newE] = first; st.e_n[newE] = second;
        pq.leaf_sal[newE] = (MEDIAN && st.size_weight) ? -first * (double)min(st.rsz[rs], st.rsz[r2]) : -first;
        pq.leaf_seq[newE] = seq;
        st.pool[offRs + posRs] = make_uint2(newE, r2);
        st.pool[r2off + idx] = make_uint2(newE, rs);
        pq_leaf_added(pq, s.pq, newE);
        // a dying leaf only matters to the tree if it is the current maximum of its level-0 node (see pq_leaf_removed)
        if (seq0) { pq.leaf_seq[e0s] = 0; if (top0 == e0s) pq_touch(pq, s.pq, 0, 0, e0s); }
        if (seq1) { pq.leaf_seq[e1s] = 0; if (top1 == e1s) pq_touch(pq, s.pq, 0, 0, e1s); }
      } while (false);
      if (MEDIAN) {
        full_barrier();   // [B:jobs]
        const uint32_t J = jobs.n;   // [R:jobs-n]
        if (J) {
          if (tid == 0) {
            unsigned long long o = 0;
            uint32_t to = 0;
            for (uint32_t j = 0; j < J; ++j) {
              const uint32_t n = jobs.na[j] + jobs.nb[j];
              jobs.off[j] = o; jobs.toff[j] = to;
              o += n; to += (n + kMergeTile - 1) / kMergeTile;
            }
            jobs.off[J] = o; jobs.toff[J] = to;
          }
          full_barrier();   // [B:jobs-off]
          const unsigned long long tot = jobs.off[J];
          const uint32_t ntiles = jobs.toff[J];
          // stable merge of the two sorted runs (ties: the (r0,rs) run first).  Merge-path splits cut every job into
          // tiles of kMergeTile outputs; a wave stages a tile's two input pieces in LDS, places every element at
          // (own index + rank in the other piece) and streams the tile out.
          const int lane = tid & 63, wave = tid >> 6;
          for (uint32_t round0 = 0; round0 < ntiles; round0 += kGreedyThreads) {
            const uint32_t q = round0 + (uint32_t)tid;
            if (q < ntiles) {
              uint32_t lo = 0, hi = J;
              while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (jobs.toff[mid] <= q) lo = mid; else hi = mid; }
              const uint32_t na = jobs.na[lo], nb = jobs.nb[lo], n = na + nb;
              const float* A = st.vals + jobs.oa[lo];
              const float* B = st.vals + jobs.ob[lo];
              const uint32_t d0 = (q - jobs.toff[lo]) * kMergeTile, d1 = d0 + kMergeTile < n ? d0 + kMergeTile : n;
              jobs.tjob[tid] = lo;
              jobs.ta0[tid] = d0 == 0 ? 0u : merge_split(A, na, B, nb, d0);
              jobs.ta1[tid] = d1 == n ? na : merge_split(A, na, B, nb, d1);
            }
            full_barrier();   // [B:tiles]
            const uint32_t cnt = ntiles - round0 < (uint32_t)kGreedyThreads ? ntiles - round0 : (uint32_t)kGreedyThreads;
            float* in = jobs.buf[wave];
            float* ob = in + kMergeTile;
            // a tile's two input pieces travel global memory -> registers -> LDS; the registers of the NEXT tile are
            // requested before the current one is merged, so the memory round trip overlaps the merge
            constexpr int kPer = (int)(kMergeTile / 64);
            float pre[kPer];
            auto fetch = [&](uint32_t t) __attribute__((always_inline)) {
              const uint32_t j = jobs.tjob[t], a0 = jobs.ta0[t], a1 = jobs.ta1[t];
              const uint32_t n = jobs.na[j] + jobs.nb[j];
              const uint32_t d0 = (round0 + t - jobs.toff[j]) * kMergeTile, d1 = d0 + kMergeTile < n ? d0 + kMergeTile : n;
              const uint32_t b0 = d0 - a0, la = a1 - a0, lt = d1 - d0;
              const float* A = st.vals + jobs.oa[j] + a0;
              const float* B = st.vals + jobs.ob[j] + b0;
#pragma unroll
              for (int k = 0; k < kPer; ++k) {          // unconditional loads: a clamped index re-reads the last element
                const uint32_t i = (uint32_t)lane + 64u * (uint32_t)k, ic = i < lt ? i : lt - 1u;
                const float* src = ic < la ? A + ic : B + (ic - la);      // one load through a selected address
                pre[k] = *src;
              }
            };
            if ((uint32_t)wave < cnt) fetch((uint32_t)wave);
            for (uint32_t t = wave; t < cnt; t += kGreedyThreads / 64) {
              const uint32_t j = jobs.tjob[t], a0 = jobs.ta0[t], a1 = jobs.ta1[t];
              const uint32_t n = jobs.na[j] + jobs.nb[j];
              const uint32_t d0 = (round0 + t - jobs.toff[j]) * kMergeTile, d1 = d0 + kMergeTile < n ? d0 + kMergeTile : n;
              const uint32_t b0 = d0 - a0, la = a1 - a0, lb = (d1 - a1) - b0, lt = la + lb;
              float* out = st.vals + vals_used + jobs.off[j] + d0;
#pragma unroll
              for (int k = 0; k < kPer; ++k) { const uint32_t i = (uint32_t)lane + 64u * (uint32_t)k; if (i < lt) in[i] = pre[k]; }
              if (t + kGreedyThreads / 64 < cnt) fetch(t + kGreedyThreads / 64);
              wave_lds_sync();
              {
                // every lane merges 16 consecutive outputs sequentially from its merge-path split (a rank search per
                // element cost ten dependent LDS reads each); the output index is padded against bank conflicts
                const float* TA = in;
                const float* TB = in + la;
                const uint32_t o0 = (uint32_t)lane * 16u < lt ? (uint32_t)lane * 16u : lt, o1 = o0 + 16u < lt ? o0 + 16u : lt;
                uint32_t ai = o0 == 0u ? 0u : (o0 >= lt ? la : merge_split(TA, la, TB, lb, o0));
                uint32_t bi = o0 - ai;
                float a = ai < la ? TA[ai] : 0.f, b = bi < lb ? TB[bi] : 0.f;
                for (uint32_t o = o0; o < o1; ++o) {
                  const bool ta = bi >= lb || (ai < la && a <= b);      // ties: the (r0, rs) run first
                  ob[o + (o >> 4)] = ta ? a : b;
                  if (ta) { ++ai; a = ai < la ? TA[ai] : 0.f; } else { ++bi; b = bi < lb ? TB[bi] : 0.f; }
                }
              }
              wave_lds_sync();
              for (uint32_t i = lane; i < lt; i += 64) out[i] = ob[i + (i >> 4)];
              const uint32_t mi = n / 2u;                               // util/stats.hxx:83-91
              if (lane == 0 && mi >= d0 && mi < d1) jobs.med[j] = ob[(mi - d0) + ((mi - d0) >> 4)];
              wave_lds_sync();
            }
            full_barrier();   // [B:tiles-end]
          }
          full_barrier();   // [B:merged]
          if ((uint32_t)tid < J) {
            const uint32_t newE = jobs.newE[tid];
            const unsigned long long off = vals_used + jobs.off[tid];
            const double med = (double)jobs.med[tid];
            st.e_off[newE] = off; st.e_mean[newE] = med;
            pq.leaf_sal[newE] = st.size_weight ? -med * (double)min(st.rsz[st.e_u[newE]], st.rsz[r2]) : -med;
          }
          vals_used += tot;
          full_barrier();   // [B:jobs-end]
        }
      }
        }
    if (tid == 0) { pq.leaf_seq[e] = 0; pq_touch(pq, s.pq, 0, 0, e);   /* the root is the maximum of its node: no need to look */ }
    if (__syncthreads_or(bad ? 1 : 0)) { status = ST_BAD_SALIENCY; break; }   // [B:bad]
    // (round 4 audit, DESIGN 3.3: s.nitems used to be cleared in front of this barrier -- the mean linkage has no barrier inside
    // phase B, so a wave that left the barrier behind phase A late could have read its item count after thread 0 had cleared it)
    if (tid == 0) s.nitems = 0;   // [W:nitems-clear]
    PH(2);

    // ---- phase C: publish r2's list; the rare big contraction resets the global marks it used ----
    const uint32_t newcount = s.newcount;   // [R:newcount]
    if (!small) {
      for (uint32_t j = tid; j < newcount; j += kGreedyThreads) {
        const uint32_t rs = st.e_u[(uint32_t)ne + j];
        st.mark0[rs] = 0; st.mark1[rs] = 0;
      }
    }
    if (tid == 0) { st.adj_off[r2] = r2off; st.adj_len[r2] = newcount; }

    PH(3);
    // ---- priority structure: propagate dirty nodes level by level ----
    pq_propagate<kGreedyThreads>(pq, s.pq, tid, topk);
    PH(4);
#ifdef GLIA_HMT_PROFILE
    if (tid == 0) {
      const unsigned long long tn = __builtin_readcyclecounter();
      const int b = total <= 64 ? 0 : total <= 512 ? 1 : total <= kMarkMax ? 2 : 3;
      tb[b] += tn - titer; nb[b] += 1; db[b] += total; titer = tn;
    }
#endif
    k += 1; ne += newcount; pool_used += total;
  }
  full_barrier();
  if (topk) pq_top_store<kGreedyThreads>(pq, topk, tid);      // the next launch (or the host's rebuild) starts from global memory
  if (tid == 0) { st.ctrl[CTRL_MERGES] = k; st.ctrl[CTRL_EDGES] = ne; st.ctrl[CTRL_ENTRIES] = pool_used; st.ctrl[CTRL_STATUS] = status; st.ctrl[CTRL_VALUES] = vals_used; }
#ifdef GLIA_HMT_PROFILE
  if (tid == 0) printf("[greedy profile] pq propagations by dirty level-0 nodes (<=8, <=16, more): %llu %llu %llu\n", g_pqprof[28], g_pqprof[29], g_pqprof[30]);
  if (tid == 0) printf("[greedy profile] pq top: loads %llu wave_max %llu barrier %llu calls %llu\n", g_pqprof[24], g_pqprof[25], g_pqprof[26], g_pqprof[27]);
  if (tid == 0) printf("[greedy profile] pq levels (wave 0): recompute %llu %llu %llu %llu  barrier-wait %llu %llu %llu %llu  active %llu %llu %llu %llu\n", g_pqprof[0], g_pqprof[1], g_pqprof[2],
                       g_pqprof[3], g_pqprof[8], g_pqprof[9], g_pqprof[10], g_pqprof[11], g_pqprof[16], g_pqprof[17], g_pqprof[18], g_pqprof[19]);
  if (tid == 0) printf("[greedy profile] by degree (<=64, <=512, <=1408, more): merges %llu %llu %llu %llu  cycles %llu %llu %llu %llu  entries %llu %llu %llu %llu\n",
                       nb[0], nb[1], nb[2], nb[3], tb[0], tb[1], tb[2], tb[3], db[0], db[1], db[2], db[3]);
  if (tid == 0) printf("[greedy profile] merges %llu: pop %llu  mark %llu  build %llu  reset %llu  pq %llu  loop-top %llu (cycles)\n", k, tph[0], tph[1], tph[2], tph[3], tph[4], tph[5]);
#endif
}

}  // namespace
}  // namespace glia
