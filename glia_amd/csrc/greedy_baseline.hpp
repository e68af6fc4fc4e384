// glia_amd/csrc/greedy_baseline.hpp -- the window queue's baseline chain: the whole-GPU work between two launches of a window-queue
// merge kernel and its host side, WinBaseline (what it decides from host integers: baseline_plan.hpp).  Part of greedy.hip's translation unit.
#pragma once
#include <limits>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_radix_sort.hpp>

#include "greedy_batch.hpp"
#include "baseline_plan.hpp"

namespace glia {
namespace {

__global__ void win_range_kernel(const double* sal, uint32_t E0, unsigned long long* mm) {
  unsigned long long lo = ~0ull, hi = 0ull;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < E0; i += gridDim.x * blockDim.x) {
    const unsigned long long b = f64_ord(sal[i]);
    lo = b < lo ? b : lo; hi = b > hi ? b : hi;
  }
  atomicMin(&mm[0], lo); atomicMax(&mm[1], hi);
}
__global__ void win_params_kernel(const unsigned long long* mm, uint32_t B, double* range) {
  const double smin = f64_unord(mm[0]), smax = f64_unord(mm[1]);
  range[0] = smin;
  range[1] = smax > smin ? (double)B / (smax - smin) : 0.0;
}
// ---- baseline: every live queue item, sorted by descending (saliency, seq) (whole-GPU kernels between launches) ----
__global__ void win_collect_kernel(const EdgeRec* er, uint32_t n_edges, const uint8_t* rdead, unsigned long long* kseq, uint32_t* vals, uint32_t* counter) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_edges) return;
  const unsigned long long q = er[e].seq;
  if (q == 0) return;
  const uint2 uv = *reinterpret_cast<const uint2*>(&er[e].u);
  if (rdead[uv.x] | rdead[uv.y]) return;         // died below the horizon: its record was not touched (WinState::rdead)
  const uint32_t i = atomicAdd(counter, 1u);
  kseq[i] = q; vals[i] = e;
}
// The same for the batch kernel, from the LISTS of the live regions: one wave per region r < n_regions that has not been merged away
// walks its incident-edge list and takes every entry with a live edge, a smaller neighbour (entry.rs < r picks every live edge
// exactly once, from the list of its larger region: u < v for an initial edge, and r2 is the newest region when its edges are made)
// and a live partner.  The records of 30 M created edges are not read -- the live edges sit in at most 2 x E0 entries -- and need
// not all exist: an edge created below the horizon of the interval that just ended (slot >= ne_base, cell < wch: store_new_edge's
// predicate, with the interval's values still in st) gets its record here, rebuilt from the entry (edge_record.hpp); every other
// edge has one.  counter[0] = items (cap = room in kseq / ksal / vals), counter[1] = records rebuilt.
// The item's saliency key comes from the entry: the saliency is -entry.mean (edge_fill: leaf_sal = -mean; store_new_edge's callers and
// rebuild_edge_record: sal = -mean), so no later kernel of the chain asks a record for it.  The seq of a rebuilt record is computed
// here, every other one is read from the record (the cat bits of a created edge are nowhere else).  Taking the seq of an initial
// edge as eid + 1 instead (edge_fill) was measured twice and bought nothing, not even in the first baseline, where every edge is
// initial: neither the old pass nor the two-pass one below waits for that one line.
// No record is asked whether the edge is queued: in the batch kernel an entry with an edge, in the list of a live region and leading
// to a live region, IS a queued edge.  The kernel rejects nothing (cond_n <= 0); a popped edge leaves two dead regions; of the edges
// a contraction replaces, (r0, rs) and (r1, rs), both have a dead end, rs's entry of the one is overwritten in place by the new
// edge and rs's entry of the other becomes a tombstone (eid = kNone).  A launch only ends between contractions.
// The order of the items is free: the two stable sorts behind the pass order by (saliency, seq), and the seqs of live items are
// distinct.  So where an item goes is decided without a shared counter, in TWO passes over the same lists: the first counts -- per
// block the items of its short lists, per wave those of the long lists it walks -- an inclusive scan over these kCollectSlots numbers
// per block turns them into ranges, and the second pass writes.  Measured on the way here (DESIGN 3.3 "Launch boundaries" 5): the
// pass was bound by its returning atomics on one address, ~20 to 45 ns each however few there were -- one per block for the short
// lists and one per trip of a walk was no faster than one per group of 16 lanes.
// A slot is items | rebuilt records << 32 (the items of a run stay far below 2^32: nothing carries over); counter[0] and counter[1]
// are written from the last slot of the scan.  counter[3] = the number of low key bits in which the collected saliency keys
// differ at all (from the key of wrange[0], any fixed value would do): every key agrees with it in the bits above, so the sort
// by key needs no pass over them.
constexpr uint32_t kCollectSlots = 5;                                    // per block: its short lists, then the walks of each of its four waves
struct CollectOut { unsigned long long *kseq, *ksal; uint32_t *vals, *idx, *counter; uint32_t cap; unsigned long long *slots, *ranges; };
struct CollectItem { unsigned long long q, sk; uint32_t e; bool live, rebuild; };
__device__ __forceinline__ uint32_t collect_key_bits(const CollectItem& it, unsigned long long kref) {
  const unsigned long long x = it.sk ^ kref;
  return it.live && x ? 64u - (uint32_t)__builtin_clzll(x) : 0u;
}
__device__ __forceinline__ void collect_store(const CollectOut& out, const CollectItem& it, uint32_t o) {
  if (it.live && o < out.cap) { out.kseq[o] = it.q; out.ksal[o] = it.sk; out.vals[o] = it.e; out.idx[o] = o; }      // (more than cap items: the host stops on the count)
}
// K entries per lane of region r's list: entry i[k] where in[k] says that it exists and is this lane's.  Two round trips: the
// entries; then the partner's rdead and, in the writing pass, the record's seq or the cat bits of a record to rebuild side by side
// (the seq of an edge whose partner turns out dead is dropped: there are next to none, see above).  Only the rebuild of a record
// sits under a branch, and it loads nothing: late in a run nearly every live edge was created below the last horizon and is
// rebuilt here.  The counting pass reads neither records nor cat bits and writes nothing.
template <int K, bool WRITE>
__device__ __forceinline__ void win_collect_entries(const WinState& st, uint32_t r, uint32_t off, uint32_t len, const uint32_t (&i)[K], const bool (&in)[K],
                                                    CollectItem (&it)[K]) {
  const double smin = st.wrange[0], scale = st.wrange[1];
  FatHalves f[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    f[k].lo = make_uint4(kNone, 0u, 0u, 0u); f[k].hi = make_uint4(0u, 0u, 0u, 0u);
    if (in[k]) f[k] = fat_load(&st.fpool[off + i[k]]);
  }
#pragma unroll
  for (int k = 0; k < K; ++k)      // (whole entries, here: else the fields only a rebuild needs are loaded again under its branch)
    asm volatile("" :: "v"(f[k].lo.x), "v"(f[k].lo.y), "v"(f[k].lo.z), "v"(f[k].lo.w), "v"(f[k].hi.x), "v"(f[k].hi.y), "v"(f[k].hi.z), "v"(f[k].hi.w));
  bool cand[K];
  uint8_t pdead[K], cat[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const uint32_t e = f[k].lo.x, rs = f[k].lo.y;
    cand[k] = in[k] && e != kNone && rs < r;
    const bool below = win_cell(-fat_mean(f[k]), smin, scale, st.wB) < st.wch;      // (computed for every entry: a branch round it reloads the mean)
    it[k].rebuild = cand[k] & ((unsigned long long)e >= st.ne_base) & below;
    pdead[k] = 0; it[k].q = 0; cat[k] = 0;
    if (cand[k]) pdead[k] = st.rdead[rs];
    if constexpr (WRITE) {
      if (cand[k] && !it[k].rebuild) it[k].q = st.er[e].seq;
      if (it[k].rebuild) cat[k] = st.ecat[e];
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    it[k].live = cand[k] && !pdead[k];
    it[k].rebuild = it[k].rebuild && it[k].live;
    it[k].e = f[k].lo.x;
    it[k].sk = f64_ord(-fat_mean(f[k]));
    if constexpr (WRITE) {
      if (it[k].rebuild) {
        FatEntry fe;
        fe.eid = f[k].lo.x; fe.rs = f[k].lo.y; fe.n = f[k].lo.z; fe.pos = f[k].lo.w; fe.off = f[k].hi.x; fe.len = f[k].hi.y; fe.mean = fat_mean(f[k]);
        const EdgeRec rec = rebuild_edge_record(fe, i[k], r, off, len, cat[k], st.R0);
        st.er[fe.eid] = rec;
        it[k].q = rec.seq;
      }
    }
  }
}
// A whole wave walks the list of region r, kWalkK entries per lane and trip; every lane of the wave is here.  Counting: returns
// items | rebuilt << 32 of the list (the same in every lane) and lifts *bits to the key bits of its items.  Writing: the items go to
// o, o + 1, ...; returns their number.
constexpr int kWalkK = 2;
template <bool WRITE>
__device__ __forceinline__ unsigned long long win_collect_walk(const WinState& st, const CollectOut& out, uint32_t r, uint32_t off, uint32_t len, uint32_t o,
                                                               unsigned long long kref, uint32_t* bits) {
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned long long n = 0;
  for (uint32_t base = 0; base < len; base += 64u * kWalkK) {
    uint32_t i[kWalkK];
    bool in[kWalkK];
#pragma unroll
    for (int k = 0; k < kWalkK; ++k) { i[k] = base + 64u * (uint32_t)k + lane; in[k] = i[k] < len; }
    CollectItem it[kWalkK];
    win_collect_entries<kWalkK, WRITE>(st, r, off, len, i, in, it);
#pragma unroll
    for (int k = 0; k < kWalkK; ++k) {
      const unsigned long long m = __ballot(it[k].live);
      if constexpr (WRITE) collect_store(out, it[k], o + (uint32_t)n + (uint32_t)__popcll(m & below));
      else *bits = max(*bits, collect_key_bits(it[k], kref));
      n += (unsigned long long)__popcll(m) | ((unsigned long long)__popcll(__ballot(it[k].rebuild)) << 32);
    }
  }
  return n;
}
// G = 64: one wave per region.  G = 16: four regions per wave, sixteen per block -- lists of ~14 entries leave 50 of 64 lanes idle.
// A list of at most kCollectShort entries is taken by its group of 16 lanes, both entries of a lane in one round trip; a ballot per
// wave and the four sums in LDS give the block's count (slot 0 of the block) and, in the writing pass, where each wave starts in
// the block's range.  EVERY thread of the block reaches the barrier: a dead region, one past n_regions and a long list contribute
// nothing there (no return, no branch round it).  The long lists among a wave's four (the hubs: thousands of entries late in a
// run) are walked by the whole wave BEHIND the barrier, one after the other, into the wave's own slot.
// The header of a region -- rdead, adj_len, adj_off -- is three independent loads for every region (one past the end reads the
// last one's), followed by selects.
constexpr uint32_t kCollectShort = 32;
template <uint32_t G, bool WRITE>
__global__ void __launch_bounds__(256) win_collect_lists_kernel(WinState st, uint32_t n_regions, CollectOut out) {
  static_assert(G == 16u || G == 64u, "lanes per list");
  // (blocks start in the order of their numbers: the newest regions first -- the hubs, whose walks are the longest jobs of the pass)
  const uint32_t blk = gridDim.x - 1u - blockIdx.x, t = blk * blockDim.x + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t r = t / G, rc = r < n_regions ? r : n_regions - 1u;
  const uint32_t dead = st.rdead[rc], len = st.adj_len[rc], off = st.adj_off[rc];
  const bool alive = r < n_regions && !dead && len != 0u;
  const unsigned long long kref = f64_ord(st.wrange[0]);
  const uint32_t slot0 = blk * kCollectSlots, wslot = slot0 + 1u + wave;
  // the scan is inclusive: a slot's range starts where the slot in front of it ends
  const uint32_t wbase = WRITE ? (uint32_t)out.ranges[wslot - 1u] : 0u;
  unsigned long long walked = 0;                                         // items | rebuilt << 32 of this wave's walks (uniform per wave)
  uint32_t bits = 0;
  if constexpr (G == 64u) {
    if (alive) walked = win_collect_walk<WRITE>(st, out, r, off, len, wbase, kref, &bits);      // (uniform per wave)
    if (!WRITE && threadIdx.x == 0) out.slots[slot0] = 0;
  } else {
    __shared__ uint32_t s_items[4], s_rebuilt[4];
    const uint32_t gl = lane & (G - 1u);
    const bool shortl = alive && len <= kCollectShort;
    const uint32_t i[2] = {gl, gl + G};
    const bool in[2] = {shortl && i[0] < len, shortl && i[1] < len};
    CollectItem it[2];
    win_collect_entries<2, WRITE>(st, rc, off, len, i, in, it);
    const unsigned long long m0 = __ballot(it[0].live), m1 = __ballot(it[1].live);
    const uint32_t c0 = (uint32_t)__popcll(m0), c1 = (uint32_t)__popcll(m1);
    if (lane == 0) { s_items[wave] = c0 + c1; s_rebuilt[wave] = (uint32_t)__popcll(__ballot(it[0].rebuild)) + (uint32_t)__popcll(__ballot(it[1].rebuild)); }
    if (!WRITE) bits = max(collect_key_bits(it[0], kref), collect_key_bits(it[1], kref));
    __syncthreads();
    if constexpr (WRITE) {
      uint32_t o = slot0 ? (uint32_t)out.ranges[slot0 - 1u] : 0u;
      for (uint32_t w = 0; w < wave; ++w) o += s_items[w];
      const unsigned long long below = (1ull << lane) - 1ull;
      collect_store(out, it[0], o + (uint32_t)__popcll(m0 & below));
      collect_store(out, it[1], o + c0 + (uint32_t)__popcll(m1 & below));
    } else if (threadIdx.x == 0)
      out.slots[slot0] = (unsigned long long)(s_items[0] + s_items[1] + s_items[2] + s_items[3]) |
                         ((unsigned long long)(s_rebuilt[0] + s_rebuilt[1] + s_rebuilt[2] + s_rebuilt[3]) << 32);
    for (uint32_t j = 0; j < 64u / G; ++j) {                             // the header of the wave's region j sits in the lanes of its group
      const uint32_t lenj = (uint32_t)__shfl((int)len, (int)(j * G)), offj = (uint32_t)__shfl((int)off, (int)(j * G));
      const bool longj = __shfl((int)alive, (int)(j * G)) != 0 && lenj > kCollectShort;
      if (longj) walked += win_collect_walk<WRITE>(st, out, (t >> 6) * (64u / G) + j, offj, lenj, wbase + (uint32_t)walked, kref, &bits);      // (uniform per wave)
    }
  }
  if constexpr (WRITE) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {                           // the scan's last slot: everything
      const unsigned long long all = out.ranges[gridDim.x * kCollectSlots - 1u];
      out.counter[0] = (uint32_t)all; out.counter[1] = (uint32_t)(all >> 32);
    }
  } else {
    if (lane == 0) out.slots[wslot] = walked;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) bits = max(bits, (uint32_t)__shfl_xor((int)bits, d));
    // (few waves know of more bits than the counter holds by the time they ask)
    if (lane == 0 && bits != 0u && bits > __hip_atomic_load(&out.counter[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&out.counter[3], bits);
  }
}
// the record scan's items (win_collect_kernel) get their saliency keys from the records
__global__ void win_salkey_kernel(const EdgeRec* er, const uint32_t* vals, uint32_t n, unsigned long long* ksal, uint32_t* idx) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { ksal[i] = f64_ord(er[vals[i]].sal); idx[i] = i; }
}
// between the two sorts: the saliency keys in the order of the first (idx = item numbers sorted by descending seq)
__global__ void win_gather_key_kernel(const unsigned long long* ksal, const uint32_t* idx, uint32_t n, unsigned long long* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = ksal[idx[i]];
}
// behind the sorts: item i of the baseline is item idx[i] of the collection; its cell comes from its sorted key
__global__ void win_baseline_fill_kernel(WinState st, uint32_t n, const unsigned long long* ksal_sorted, const uint32_t* idx, const unsigned long long* kseq, const uint32_t* vals,
                                         uint32_t* isort_w, unsigned long long* isort_seq) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t j = idx[i];
  isort_w[i] = vals[j]; isort_seq[i] = kseq[j];
  atomicAdd(&st.wcnt[win_cell(f64_unord(ksal_sorted[i]), st.wrange[0], st.wrange[1], st.wB)], 1u);
}
// ige[c] = number of baseline items whose cell is >= c (c = 0..B): cell c's segment of the sorted array is [ige[c+1], ige[c])
__global__ void win_segments_kernel(WinState st, const unsigned long long* ksal_sorted, uint32_t n, uint32_t* ige) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c > st.wB) return;
  uint32_t lo = 0, hi = n;                    // first index whose cell is < c
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (win_cell(f64_unord(ksal_sorted[mid]), st.wrange[0], st.wrange[1], st.wB) >= c) lo = mid + 1; else hi = mid;
  }
  ige[c] = c == 0 ? n : lo;
}
// GLIA_HMT_BASELINE_AUDIT: a finished baseline of n items against its sources; *bad counts the mismatches.
//   item j of the collection (j < n): its record's (seq, saliency key) equal the collected ones -- every collected edge has a record;
//   item i of the sorted array: (key, seq) not above its predecessor's, equal to the record of isort[i], its cell not above the starting
//     threshold cthr and its position inside its cell's segment [ige[cell + 1], ige[cell]);
//   cell c (c <= B): ige does not rise with c, ige[0] = n, and wcnt[c] is the length of the segment.
// With every item inside its cell's segment and ige falling from n, ige[c] IS the number of items whose cell is >= c: the items in
// front of ige[c] are exactly those (an item of a cell >= c sits in front of ige[its cell] <= ige[c], one of a cell below c at or
// behind ige[its cell + 1] >= ige[c]).
__global__ void win_baseline_audit_kernel(WinState st, uint32_t n, const unsigned long long* kseq, const unsigned long long* ksal, const uint32_t* vals,
                                          const unsigned long long* ksal_sorted, const uint32_t* isort, const unsigned long long* iseq, const uint32_t* ige,
                                          long long cthr, uint32_t* bad) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t wrong = 0;
  if (i < n) {
    const EdgeRec a = st.er[vals[i]];
    wrong += a.seq != kseq[i] || f64_ord(a.sal) != ksal[i] || kseq[i] == 0;
    const EdgeRec b = st.er[isort[i]];
    const unsigned long long ks = ksal_sorted[i], q = iseq[i];
    wrong += b.seq != q || f64_ord(b.sal) != ks;
    if (i > 0) wrong += ksal_sorted[i - 1] < ks || (ksal_sorted[i - 1] == ks && iseq[i - 1] <= q);
    const uint32_t c = win_cell(f64_unord(ks), st.wrange[0], st.wrange[1], st.wB);
    wrong += (long long)c > cthr;
    wrong += !(ige[c + 1] <= i && i < ige[c]);
  }
  if (i <= st.wB) {
    wrong += i == 0 ? ige[0] != n : ige[i] > ige[i - 1];
    if (i < st.wB) wrong += ige[i] < ige[i + 1] || st.wcnt[i] != ige[i] - ige[i + 1];
  }
  if (wrong) atomicAdd(bad, wrong);
}

}  // namespace

// The window queue's BASELINE on the host: all live queue items sorted by descending (saliency, seq) -- two stable radix sorts
// (by seq, then by the saliency's order-preserving image), per-cell segments and live counters; the cell lists start empty.
// The collection leaves compact arrays (seq, saliency key, edge) and the sorts move item NUMBERS: the first sorts (seq, number), one
// streaming pass gathers the saliency keys in that order, the second sorts (key, number); the fill pass writes isort / isort_seq
// through the numbers, and it and the segment search take the cells from the sorted keys.  No kernel behind the collection reads a record.
// Taken at the start (the initial edges) and whenever a launch ends before the queue is empty: the lists only shed their dead
// nodes when their cell is loaded, so after a few million created edges walking them dominates; a re-sort is ~1 ms of whole-GPU work.
struct WinBaseline {
  unsigned long long *kseq = nullptr, *kseq2 = nullptr, *ksal = nullptr, *ksalg = nullptr, *ksal2 = nullptr, *iseq = nullptr;
  uint32_t *vals = nullptr, *idx = nullptr, *idx1 = nullptr, *idx2 = nullptr, *isort = nullptr, *ige = nullptr, *counter = nullptr;
  unsigned long long *slots = nullptr, *ranges = nullptr; size_t slots_cap = 0;      // the collection pass's counts and their inclusive scan
  void* tmp = nullptr; size_t tmp_bytes = 0;
  uint32_t E0 = 0;
  double h_range[2] = {0.0, 0.0};                                        // WinState::wrange on the host
  BaselinePolicy policy; BaselineTrack track;                            // interval and horizon (baseline_plan.hpp): the caller sets the options, init the sizes
  uint32_t n_last = 0;                                                   // items of the last collection (init: the initial edges)
  bool from_lists = false;                                               // the batch kernel: collect from the lists of the live regions (win_collect_lists_kernel)
  unsigned long long rebuilt_last = 0;                                   // records the last collection rebuilt
  int seq_bits = 64;                                                     // a seq is (merge + 1) << 32 | cat << 30 | region, merge < R
  int key_bits = 64;                                                     // the collected saliency keys agree in every bit from this one up (the list walk finds it; the record scan: 64)
  uint32_t lanes_forced = 0;                                             // tests (GLIA_HMT_COLLECT_LANES): lanes per region of the collection pass
  bool audit = false;                                                    // GLIA_HMT_BASELINE_AUDIT: check every baseline (win_baseline_audit_kernel)

  // the queue's device arrays for B saliency cells, and the saliency range of the n_initial initial edges
  int init(DeviceBuffers& buf, WinState& ws, const double* leaf_sal, uint32_t n_initial, uint32_t B, uint32_t R, hipStream_t stream) {
    int rc;
    E0 = n_initial; n_last = n_initial; policy.wB = B; policy.E0 = n_initial;
    unsigned long long* mm; double* range;
    if ((rc = buf.get(&ws.rdead, 2 * (size_t)R, true, stream))) return rc;
    if ((rc = buf.get(&ws.whead, B, false, stream)) || (rc = buf.get(&ws.wcnt, B, true, stream))) return rc;
    if ((rc = buf.get(&isort, E0, false, stream)) || (rc = buf.get(&iseq, E0, false, stream)) || (rc = buf.get(&ige, (size_t)B + 1, false, stream))) return rc;
    if ((rc = buf.get(&mm, 2, false, stream)) || (rc = buf.get(&range, 2, false, stream))) return rc;
    if ((rc = buf.get(&kseq, E0, false, stream)) || (rc = buf.get(&kseq2, E0, false, stream)) || (rc = buf.get(&ksal, E0, false, stream)) ||
        (rc = buf.get(&ksalg, E0, false, stream)) || (rc = buf.get(&ksal2, E0, false, stream)) || (rc = buf.get(&vals, E0, false, stream)) ||
        (rc = buf.get(&idx, E0, false, stream)) || (rc = buf.get(&idx1, E0, false, stream)) || (rc = buf.get(&idx2, E0, false, stream)))
      return rc;
    if ((rc = buf.get(&counter, 4, true, stream))) return rc;                // items, records rebuilt, audit mismatches, key bits (CollectOut)
    GLIA_HIP_TRY(rocprim::radix_sort_pairs_desc(nullptr, tmp_bytes, kseq, kseq2, idx, idx1, (size_t)E0, 0, 64, stream));
    slots_cap = plan_collect_slots(R, kCollectSlots);
    if ((rc = buf.get(&slots, slots_cap, false, stream)) || (rc = buf.get(&ranges, slots_cap, false, stream))) return rc;
    size_t scan_bytes = 0;
    GLIA_HIP_TRY(rocprim::inclusive_scan(nullptr, scan_bytes, slots, ranges, slots_cap, rocprim::plus<unsigned long long>(), stream));
    tmp_bytes = std::max(tmp_bytes, scan_bytes);
    seq_bits = plan_seq_bits(R);
    if ((rc = buf.get((char**)&tmp, tmp_bytes ? tmp_bytes : 16, false, stream))) return rc;
    ws.wrange = range; ws.isort = isort; ws.isort_seq = iseq; ws.ige = ige;
    const unsigned long long mm0[2] = {~0ull, 0ull};
    GLIA_HIP_TRY(hipMemcpyAsync(mm, mm0, sizeof(mm0), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(win_range_kernel, dim3(256), dim3(256), 0, stream, leaf_sal, E0, mm);
    hipLaunchKernelGGL(win_params_kernel, dim3(1), dim3(1), 0, stream, mm, B, range);
    GLIA_HIP_TRY(hipGetLastError());
    GLIA_HIP_TRY(hipMemcpyAsync(h_range, range, sizeof(h_range), hipMemcpyDeviceToHost, stream));
    GLIA_HIP_TRY(hipStreamSynchronize(stream));
    return GLIA_HMT_OK;
  }
  // every live queue item (seq, saliency key, edge, its own number) into kseq / ksal / vals / idx, in any order: from the first n_edges
  // edge records, or from the lists of the live regions among the first n_regions, rebuilding the records the batch kernel did not
  // write (ws still holds the horizon and the edge count of the interval that just ended).
  int collect(const WinState& ws, uint32_t n_edges, uint32_t n_regions, hipStream_t stream, uint32_t* n_out) {
    GLIA_HIP_TRY(hipMemsetAsync(counter, 0, 4 * sizeof(uint32_t), stream));
    if (from_lists) {
      const uint32_t G = plan_collect_lanes(ws.R0, n_regions, n_last, lanes_forced);
      const dim3 grid((unsigned)plan_collect_blocks(n_regions, G));
      const CollectOut out = {kseq, ksal, vals, idx, counter, E0, slots, ranges};
      const size_t n_slots = (size_t)grid.x * kCollectSlots;
      if (n_slots > slots_cap) { set_error("greedy: the collection pass has more blocks than slots (internal error)"); return GLIA_HMT_ERR_INTERNAL; }
      // count, scan, write (the kernel's comment)
      if (G == 16u) hipLaunchKernelGGL((win_collect_lists_kernel<16u, false>), grid, dim3(256), 0, stream, ws, n_regions, out);
      else hipLaunchKernelGGL((win_collect_lists_kernel<64u, false>), grid, dim3(256), 0, stream, ws, n_regions, out);
      size_t bytes = tmp_bytes;
      GLIA_HIP_TRY(rocprim::inclusive_scan(tmp, bytes, slots, ranges, n_slots, rocprim::plus<unsigned long long>(), stream));
      if (G == 16u) hipLaunchKernelGGL((win_collect_lists_kernel<16u, true>), grid, dim3(256), 0, stream, ws, n_regions, out);
      else hipLaunchKernelGGL((win_collect_lists_kernel<64u, true>), grid, dim3(256), 0, stream, ws, n_regions, out);
    } else hipLaunchKernelGGL(win_collect_kernel, dim3((n_edges + 255) / 256), dim3(256), 0, stream, ws.er, n_edges, ws.rdead, kseq, vals, counter);
    GLIA_HIP_TRY(hipGetLastError());
    uint32_t h[4] = {0, 0, 0, 0};
    GLIA_HIP_TRY(hipMemcpyAsync(h, counter, sizeof(h), hipMemcpyDeviceToHost, stream));
    GLIA_HIP_TRY(hipStreamSynchronize(stream));
    if (h[0] > E0) { set_error("greedy: more live edges than initial edges (internal error)"); return GLIA_HMT_ERR_INTERNAL; }
    *n_out = h[0]; rebuilt_last = h[1]; n_last = h[0];
    key_bits = from_lists ? std::max(1, (int)h[3]) : 64;
    if (!from_lists && h[0]) { hipLaunchKernelGGL(win_salkey_kernel, dim3((h[0] + 255) / 256), dim3(256), 0, stream, ws.er, vals, h[0], ksal, idx); GLIA_HIP_TRY(hipGetLastError()); }
    return GLIA_HMT_OK;
  }
  // a fresh baseline of the first n_edges edges (the lists of the first R0 + merges regions); the threshold words of ctrl are reset to
  // "everything is below it": the end of the cell of the largest key
  int rebaseline(WinState& ws, uint32_t n_edges, unsigned long long* ctrl, hipStream_t stream) {
    uint32_t n = 0;
    if (int rc = collect(ws, n_edges, ws.R0 + (uint32_t)ctrl[CTRL_MERGES], stream, &n)) return rc;
    if (n) {
      size_t bytes = tmp_bytes;
      GLIA_HIP_TRY(rocprim::radix_sort_pairs_desc(tmp, bytes, kseq, kseq2, idx, idx1, (size_t)n, 0, (unsigned)seq_bits, stream));
      hipLaunchKernelGGL(win_gather_key_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, ksal, idx1, n, ksalg);
      bytes = tmp_bytes;
      GLIA_HIP_TRY(rocprim::radix_sort_pairs_desc(tmp, bytes, ksalg, ksal2, idx1, idx2, (size_t)n, 0, (unsigned)key_bits, stream));
    }
    GLIA_HIP_TRY(hipMemsetAsync(ws.whead, 0xFF, sizeof(uint32_t) * ws.wB, stream));
    GLIA_HIP_TRY(hipMemsetAsync(ws.wcnt, 0, sizeof(uint32_t) * ws.wB, stream));
    if (n) hipLaunchKernelGGL(win_baseline_fill_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, ws, n, ksal2, idx2, kseq, vals, isort, iseq);
    hipLaunchKernelGGL(win_segments_kernel, dim3((ws.wB + 1 + 255) / 256), dim3(256), 0, stream, ws, ksal2, n, ige);
    GLIA_HIP_TRY(hipGetLastError());
    ws.nsort = n;
    long long top_cell = (long long)ws.wB - 1;                             // the cell of the largest key (nothing alive: the last cell)
    if (n) {
      unsigned long long topkey = 0;
      GLIA_HIP_TRY(hipMemcpyAsync(&topkey, ksal2, sizeof(topkey), hipMemcpyDeviceToHost, stream));
      GLIA_HIP_TRY(hipStreamSynchronize(stream));
      top_cell = (long long)win_cell(f64_unord(topkey), h_range[0], h_range[1], ws.wB);
    }
    const BaselinePlan plan = plan_baseline(policy, track, n, n_edges, top_cell);      // the next launch's interval and horizon
    ws.rebase_after = plan.rebase_after; ws.wch = plan.wch;
    ws.ne_base = n_edges;
    const double inf = std::numeric_limits<double>::infinity();
    // threshold: the end of the top occupied cell -- everything alive is below it, and the first reload starts at that cell instead of
    // walking down to it from the last one, 512 empty cells per step (greedy_window.hpp, header comment)
    ctrl[CTRL_CTHR] = (unsigned long long)top_cell;
    memcpy(&ctrl[CTRL_TSAL], &inf, 8); ctrl[CTRL_TSEQ] = ~0ull; ctrl[CTRL_IPTR] = 0;
    if (audit) {
      hipLaunchKernelGGL(win_baseline_audit_kernel, dim3((std::max(n, ws.wB + 1u) + 255u) / 256u), dim3(256), 0, stream, ws, n, kseq, ksal, vals, ksal2, isort, iseq, ige,
                         top_cell, counter + 2);
      GLIA_HIP_TRY(hipGetLastError());
      uint32_t bad = 0;
      GLIA_HIP_TRY(hipMemcpyAsync(&bad, counter + 2, sizeof(bad), hipMemcpyDeviceToHost, stream));
      GLIA_HIP_TRY(hipStreamSynchronize(stream));
      if (bad) { set_error("greedy: the baseline audit found " + std::to_string(bad) + " mismatches (internal error)"); return GLIA_HMT_ERR_INTERNAL; }
    }
    return GLIA_HMT_OK;
  }
};

}  // namespace glia
