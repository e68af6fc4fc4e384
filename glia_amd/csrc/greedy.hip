// glia_amd/csrc/greedy.hip -- K4b + K5: edge table and the greedy agglomeration loop, on the device.
//
// Reference semantics reproduced (all under /root/reference/code/):
//   * TBoundaryTable::init (type/boundary_table.hxx:91-114): one edge per unordered label pair, only if BOTH
//     directed boundaries exist; queue inserts happen in lexicographic (r0,r1) order.
//   * TBoundaryTable::top (:46-52) on a std::multimap<double,...>: largest saliency, and among equal
//     saliencies the MOST RECENTLY INSERTED item.  Here every queue item carries a 64-bit sequence number
//     that is order-isomorphic to the reference's insertion order, and the queue orders by (saliency, seq).
//   * TBoundaryTable::update (:121-167): the table scan visits the neighbours rs of the merged pair
//     (r0 < r1) in this order:  rs < r0 ascending;  neighbours of r0 with rs > r0 ascending;  neighbours of
//     r1 only, ascending.  seq = (merge# + 1) << 32 | category << 30 | rs encodes exactly that, so no sort
//     is needed.  pData0s is always the (r0,rs) item, pData1s the (r1,rs) item (:139-153).
//   * genMergeOrderGreedy (util/struct_merge.hxx:13-33) and the mean linkage (:62-76):
//     d2 = sdivide(m0*n0 + m1*n1, n0+n1, 0) with the reference's operation order (no FMA contraction).
//
// MI355X mapping.  The loop is a chain of R-1 dependent contractions, so it runs as ONE persistent
// workgroup: all state (edge records, adjacency pool, priority structure) stays in HBM/L2, each
// contraction is data-parallel over the neighbours of the merged pair.  The priority queue is a
// 64-ary tournament tree over edge slots (one wave recomputes one node with a 64-lane reduction);
// insertions and deletions of one contraction are applied level by level from a dirty-node worklist.
// Dense region ids: leaves 0..R-1 ascending by label, merged regions R+k; the map id -> key is monotone,
// so every key comparison of the reference is an id comparison here.
#include <atomic>
#include <cstring>
#include <vector>
#include <limits>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "greedy_batch.hpp"      // <- greedy_window.hpp <- greedy_tree.hpp <- greedy_common.hpp: the three loops

namespace glia {

__global__ void pq_build_level_kernel(PqTree t, int l) {
  const int lane = threadIdx.x & 63;
  uint32_t j = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (j < t.lv[l].size) (void)pq_recompute_node(t, l, j, lane, true);   // fresh memory: always write
}

// (re)allocates the tree levels above t.nleaves leaves and builds them from the current leaf keys
int pq_setup(DeviceBuffers& buf, PqTree& t, hipStream_t stream) {
  t.nlevels = 0;
  uint32_t n = t.nleaves;
  while (true) {
    n = (n + kFan - 1) / kFan;
    if (t.nlevels >= kMaxLevels) { set_error("greedy: edge table too large"); return GLIA_HMT_ERR_ARG; }
    PqLevel& L = t.lv[t.nlevels++];
    L.size = n;
    int rc;
    if ((rc = buf.get(&L.sal, n, false, stream))) return rc;
    if ((rc = buf.get(&L.seq, n, false, stream))) return rc;
    if ((rc = buf.get(&L.arg, n, false, stream))) return rc;
    if ((rc = buf.get(&L.dirty, n, true, stream))) return rc;
    if (n <= kTopMax) break;
  }
  {
    int rc;
    if ((rc = buf.get(&t.glist[0], t.lv[0].size, false, stream))) return rc;
    if ((rc = buf.get(&t.glist[1], t.lv[0].size, false, stream))) return rc;
    if ((rc = buf.get(&t.gcount, 2, true, stream))) return rc;
  }
  for (int l = 0; l < t.nlevels; ++l) {
    unsigned long long threads = (unsigned long long)t.lv[l].size * 64ull;
    hipLaunchKernelGGL(pq_build_level_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, t, l);
  }
  GLIA_HIP_TRY(hipGetLastError());
  return GLIA_HMT_OK;
}

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
__global__ void adj_fill_fat(GreedyState g, WinState st, uint32_t E0, uint32_t* cursor) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E0) return;
  const uint32_t u = g.e_u[e], v = g.e_v[e];
  const uint32_t pu = atomicAdd(&cursor[u], 1u), pv = atomicAdd(&cursor[v], 1u);
  const uint32_t ou = g.adj_off[u], ov = g.adj_off[v], lu = g.adj_len[u], lv = g.adj_len[v];
  FatEntry a; a.eid = e; a.rs = v; a.n = (uint32_t)g.e_n[e]; a.pos = pv; a.off = ov; a.len = lv; a.mean = g.e_mean[e];
  FatEntry b = a; b.rs = u; b.pos = pu; b.off = ou; b.len = lu;
  st.fpool[ou + pu] = a; g.e_posu[e] = pu;
  st.fpool[ov + pv] = b; g.e_posv[e] = pv;
  EdgeRec r; r.u = u; r.v = v; r.posu = pu; r.posv = pv; r.mean = g.e_mean[e]; r.n = g.e_n[e]; r.next = kNone;
  r.hu = make_uint2(ou, lu); r.hv = make_uint2(ov, lv); r.sal = g.pq.leaf_sal[e]; r.seq = g.pq.leaf_seq[e];
  st.er[e] = r;
}
// ST_NEED_TREE: the tree kernel continues on its own arrays -- thin list entries and one array per edge field
__global__ void fat_to_thin(const FatEntry* f, uint2* out, unsigned long long n) {
  const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { const FatEntry fe = f[i]; out[i] = make_uint2(fe.eid, fe.eid == kNone ? 0u : fe.rs); }
}
__global__ void edge_unpack(GreedyState g, const EdgeRec* er, const uint8_t* rdead, uint32_t n) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const EdgeRec r = er[e];
  g.e_u[e] = r.u; g.e_v[e] = r.v; g.e_posu[e] = r.posu; g.e_posv[e] = r.posv; g.e_mean[e] = r.mean; g.e_n[e] = r.n;
  g.pq.leaf_sal[e] = r.sal; g.pq.leaf_seq[e] = (rdead[r.u] | rdead[r.v]) ? 0ull : r.seq;
}

// ... after a batch launch: only the n live edges the collection pass listed (vals) have records for certain, and only they are ever
// looked at again (a live region's list holds live edges and tombstones); every other leaf has been marked dead beforehand
__global__ void edge_unpack_live(GreedyState g, const EdgeRec* er, const uint32_t* vals, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t e = vals[i];
  const EdgeRec r = er[e];
  g.e_u[e] = r.u; g.e_v[e] = r.v; g.e_posu[e] = r.posu; g.e_posv[e] = r.posv; g.e_mean[e] = r.mean; g.e_n[e] = r.n;
  g.pq.leaf_sal[e] = r.sal; g.pq.leaf_seq[e] = r.seq;
}

// ---- edge table construction --------------------------------------------------------------------------
__global__ void edge_flags(const uint32_t* pa, const uint32_t* pb, long long P, uint32_t* flag, long long* partner) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  uint32_t a = pa[i], b = pb[i];
  long long j = (a < b) ? find_pair(pa, pb, P, b, a) : -1;   // "boundaries have to be mutual" (boundary_table.hxx:99-102)
  flag[i] = j >= 0 ? 1u : 0u;
  partner[i] = j;
}

__global__ void edge_fill(const uint32_t* pa, const uint32_t* pb, const uint32_t* prec, long long P,
                          const uint32_t* flag, const uint32_t* eidx, const long long* partner,
                          const uint32_t* rlabel, uint32_t R, GreedyState st, uint32_t* deg) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P || !flag[i]) return;
  const uint32_t e = eidx[i];
  const long long j = partner[i];
  const uint32_t u = find_label(rlabel, R, pa[i]), v = find_label(rlabel, R, pb[i]);
  const uint32_t* wi = &prec[(size_t)i * kPairWords];
  const uint32_t* wj = &prec[(size_t)j * kPairWords];
  double si, sj;
  memcpy(&si, &wi[P_SUM], 8);
  memcpy(&sj, &wj[P_SUM], 8);
  // util/struct_merge.hxx:45-56: sum of pb over both directed boundaries / their voxel count
  const int n = (int)(wi[P_CNT] + wj[P_CNT]);
  const double mean = sdivide(si + sj, (double)n, 0.0);
  st.e_u[e] = u; st.e_v[e] = v; st.e_mean[e] = mean; st.e_n[e] = n;
  st.pq.leaf_sal[e] = -mean; st.pq.leaf_seq[e] = (unsigned long long)e + 1ull;
  atomicAdd(&deg[u], 1u);
  atomicAdd(&deg[v], 1u);
}

__global__ void adj_fill(GreedyState st, uint32_t E0, uint32_t* cursor) {
  uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E0) return;
  const uint32_t u = st.e_u[e], v = st.e_v[e];
  const uint32_t pu = atomicAdd(&cursor[u], 1u), pv = atomicAdd(&cursor[v], 1u);
  st.pool[st.adj_off[u] + pu] = make_uint2(e, v); st.e_posu[e] = pu;
  st.pool[st.adj_off[v] + pv] = make_uint2(e, u); st.e_posv[e] = pv;
}

__global__ void region_sizes(const uint32_t* rrec, uint32_t R, unsigned long long* rsz, double* rsum) {
  uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const uint32_t* w = &rrec[(size_t)r * kRegionWords];
  rsz[r] = w[R_CNT];
  double d; memcpy(&d, &w[R_SUM], 8); rsum[r] = d;
}

// median linkage, initFb (util/struct_merge.hxx:97-103): the pb value of every voxel on either directed boundary of a
// table edge.  The voxel's pair is re-derived with the neighbour rule of getContourTraits (type/neighbor.hxx:109-126).
__global__ void median_collect(VolumeRef vol, const uint32_t* pa, const uint32_t* pb, long long P, const uint32_t* flag,
                               const uint32_t* eidx, const unsigned long long* e_off, uint32_t* cursor, float* out) {
  const long long N = vol.nx * vol.ny * vol.nz;
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= N) return;
  const long long x = p % vol.nx, y = (p / vol.nx) % vol.ny, z = p / (vol.nx * vol.ny);
  const uint32_t t = vol.lab[p];
  if (t == kMaskedLabel) return;                          // masked-out centre (point-map mode)
  uint32_t nb = t;
  const long long sy = vol.nx, sz = vol.nx * vol.ny;
  const uint32_t* L = vol.lab_nb;                         // masked-out neighbours hold kMaskedLabel: invalid
  do {
    uint32_t q;
    if (x > 0 && (q = L[p - 1]) != t && q != kMaskedLabel) { nb = q; break; }
    if (x + 1 < vol.nx && (q = L[p + 1]) != t && q != kMaskedLabel) { nb = q; break; }
    if (y > 0 && (q = L[p - sy]) != t && q != kMaskedLabel) { nb = q; break; }
    if (y + 1 < vol.ny && (q = L[p + sy]) != t && q != kMaskedLabel) { nb = q; break; }
    if (vol.dim == 3) {
      if (z > 0 && (q = L[p - sz]) != t && q != kMaskedLabel) { nb = q; break; }
      if (z + 1 < vol.nz && (q = L[p + sz]) != t && q != kMaskedLabel) { nb = q; break; }
    }
  } while (false);
  if (nb == t) return;
  const long long i = find_pair(pa, pb, P, t < nb ? t : nb, t < nb ? nb : t);
  if (i < 0 || !flag[i]) return;                         // not a mutual boundary: no table edge
  const uint32_t e = eidx[i];
  out[e_off[e] + atomicAdd(&cursor[e], 1u)] = vol.pb[p];
}

// the same from a map that carries its boundary values per directed pair (slab route, RagArrays::d_pv): the run of a table edge
// = the runs of its two directions, one thread per value
__global__ void median_from_runs(const unsigned long long* pv_off, const float* pv, unsigned long long nV, const uint32_t* pa, const uint32_t* pb, long long P,
                                 const uint32_t* flag, const uint32_t* eidx, const unsigned long long* e_off, float* out) {
  const unsigned long long v = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nV) return;
  long long lo = 0, hi = P;                     // the pair whose run holds value v
  while (lo < hi) { const long long mid = (lo + hi) >> 1; if (pv_off[mid + 1] <= v) lo = mid + 1; else hi = mid; }
  const long long i = lo;
  const uint32_t a = pa[i], b = pb[i];
  // the (a < b) direction owns the edge slot when the boundary is mutual (edge_flags); its values come first
  const long long owner = a < b ? i : find_pair(pa, pb, P, b, a);
  if (owner < 0 || !flag[owner]) return;       // not a mutual boundary: no table edge
  const unsigned long long first = owner == i ? 0ull : pv_off[owner + 1] - pv_off[owner];
  out[e_off[eidx[owner]] + first + (v - pv_off[i])] = pv[v];
}

__global__ void median_init(GreedyState st, uint32_t E0) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E0) return;
  const uint32_t n = (uint32_t)st.e_n[e];
  const double med = (double)st.vals[st.e_off[e] + n / 2u];      // amedian, util/stats.hxx:83-91
  st.e_mean[e] = med;
  st.pq.leaf_sal[e] = st.size_weight ? -med * (double)min(st.rsz[st.e_u[e]], st.rsz[st.e_v[e]]) : -med;
  atomicAdd(&st.rbv[st.e_u[e]], (unsigned long long)n);
  atomicAdd(&st.rbv[st.e_v[e]], (unsigned long long)n);
}

__global__ void fill_leaves_dead(PqTree t, uint32_t from) {
  uint32_t i = from + blockIdx.x * blockDim.x + threadIdx.x;
  if (i < t.nleaves) { t.leaf_seq[i] = 0; t.leaf_sal[i] = -__builtin_inf(); }
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
  long long prev_top_cell = -1;
  unsigned long long prev_ne = 0;
  uint32_t n_last = 0;                                                   // items of the last collection (init: the initial edges)
  double horizon_factor = 0.0;                                           // 0 = no horizon (set for the batch kernel)
  bool from_lists = false;                                               // the batch kernel: collect from the lists of the live regions (win_collect_lists_kernel)
  unsigned long long rebuilt_last = 0;                                   // records the last collection rebuilt
  int seq_bits = 64;                                                     // a seq is (merge + 1) << 32 | cat << 30 | region, merge < R
  int key_bits = 64;                                                     // the collected saliency keys agree in every bit from this one up (the list walk finds it; the record scan: 64)
  uint32_t lanes_forced = 0;                                             // tests (GLIA_HMT_COLLECT_LANES): lanes per region of the collection pass
  // GLIA_HMT_REBASE_END: an interval without a horizon in a run that has placed horizons is this many times shorter (1 = as long as
  // any).  Swept at 1024^3: 1 / 2 / 4 / 8 / 16 / 32 = 727.1 / 716.2 / 714.2 / 713.2 / 714.8 / 719.1 ms of merge loop
  unsigned long long rebase_end = 8;
  bool audit = false;                                                    // GLIA_HMT_BASELINE_AUDIT: check every baseline (win_baseline_audit_kernel)

  // the queue's device arrays for B saliency cells, and the saliency range of the n_initial initial edges
  int init(DeviceBuffers& buf, WinState& ws, const double* leaf_sal, uint32_t n_initial, uint32_t B, uint32_t R, hipStream_t stream) {
    int rc;
    E0 = n_initial; n_last = n_initial;
    unsigned long long* mm; double* range;
    if ((rc = buf.get(&ws.rdead, 2 * (size_t)R, true, stream))) return rc;
    if ((rc = buf.get(&ws.whead, B, false, stream))) return rc;
    if ((rc = buf.get(&ws.wcnt, B, true, stream))) return rc;
    if ((rc = buf.get(&isort, E0, false, stream))) return rc;
    if ((rc = buf.get(&iseq, E0, false, stream))) return rc;
    if ((rc = buf.get(&ige, (size_t)B + 1, false, stream))) return rc;
    if ((rc = buf.get(&mm, 2, false, stream))) return rc;
    if ((rc = buf.get(&range, 2, false, stream))) return rc;
    if ((rc = buf.get(&kseq, E0, false, stream))) return rc;
    if ((rc = buf.get(&kseq2, E0, false, stream))) return rc;
    if ((rc = buf.get(&ksal, E0, false, stream))) return rc;
    if ((rc = buf.get(&ksalg, E0, false, stream))) return rc;
    if ((rc = buf.get(&ksal2, E0, false, stream))) return rc;
    if ((rc = buf.get(&vals, E0, false, stream))) return rc;
    if ((rc = buf.get(&idx, E0, false, stream))) return rc;
    if ((rc = buf.get(&idx1, E0, false, stream))) return rc;
    if ((rc = buf.get(&idx2, E0, false, stream))) return rc;
    if ((rc = buf.get(&counter, 4, true, stream))) return rc;                // items, records rebuilt, audit mismatches, key bits (CollectOut)
    GLIA_HIP_TRY(rocprim::radix_sort_pairs_desc(nullptr, tmp_bytes, kseq, kseq2, idx, idx1, (size_t)E0, 0, 64, stream));
    // the collection pass's slots: kCollectSlots per block of 256 threads, at most one wave for each of the 2 R regions there can be
    slots_cap = (((size_t)2 * R * 64 + 255) / 256) * kCollectSlots;
    if ((rc = buf.get(&slots, slots_cap, false, stream))) return rc;
    if ((rc = buf.get(&ranges, slots_cap, false, stream))) return rc;
    size_t scan_bytes = 0;
    GLIA_HIP_TRY(rocprim::inclusive_scan(nullptr, scan_bytes, slots, ranges, slots_cap, rocprim::plus<unsigned long long>(), stream));
    tmp_bytes = std::max(tmp_bytes, scan_bytes);
    seq_bits = 33;
    while (seq_bits < 63 && ((unsigned long long)R >> (seq_bits - 32)) != 0) ++seq_bits;
    seq_bits += 1;                                                         // 32 + bits of R + 1: the sort by seq looks at no bit above
    std::string o_txt;
    if (option("GLIA_HMT_COLLECT_LANES", &o_txt)) lanes_forced = (uint32_t)strtoul(o_txt.c_str(), nullptr, 10);
    audit = option("GLIA_HMT_BASELINE_AUDIT", &o_txt) && o_txt[0] != '0';
    if (option("GLIA_HMT_REBASE_END", &o_txt)) rebase_end = std::max(1ull, strtoull(o_txt.c_str(), nullptr, 10));
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
  // Lanes per region of the list walk: 16 while the lists are short, from numbers the host holds -- the live edges of the last
  // collection (at the start: the initial edges), each in two lists, over the regions that are left (n_regions - R0 merges so far)
  int collect(const WinState& ws, uint32_t n_edges, uint32_t n_regions, hipStream_t stream, uint32_t* n_out) {
    GLIA_HIP_TRY(hipMemsetAsync(counter, 0, 4 * sizeof(uint32_t), stream));
    if (from_lists) {
      const unsigned long long live_regions = 2ull * ws.R0 > n_regions ? 2ull * ws.R0 - n_regions : 1ull;
      const uint32_t G = lanes_forced == 16u || lanes_forced == 64u ? lanes_forced : 2ull * n_last <= 24ull * live_regions ? 16u : 64u;
      const dim3 grid((unsigned)(((unsigned long long)n_regions * G + 255ull) / 256ull));
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
    std::string renv;                                                      // created edges between baselines (tuning)
    ws.rebase_after = option("GLIA_HMT_REBASE", &renv) ? strtoull(renv.c_str(), nullptr, 10) : std::max<unsigned long long>(800000ull, (unsigned long long)n / 2ull);
    // the horizon (WinState::wch): the top of the queue sank by d cells while the last interval's edges were created; the next
    // interval is given horizon_factor times that (scaled to its planned length; at least 1/512 of the cells) before a reload
    // would run into the horizon
    ws.wch = 0;
    long long top_cell = (long long)ws.wB - 1;                             // the cell of the largest key (nothing alive: the last cell)
    if (n) {
      unsigned long long topkey = 0;
      GLIA_HIP_TRY(hipMemcpyAsync(&topkey, ksal2, sizeof(topkey), hipMemcpyDeviceToHost, stream));
      GLIA_HIP_TRY(hipStreamSynchronize(stream));
      top_cell = (long long)win_cell(f64_unord(topkey), h_range[0], h_range[1], ws.wB);
    }
    if (horizon_factor > 0.0 && n > 4096) {
      if (prev_top_cell >= 0 && n_edges > prev_ne) {
        const double d = (double)std::max<long long>(0, prev_top_cell - top_cell);
        const double delta = std::max(horizon_factor * d * (double)ws.rebase_after / (double)(n_edges - prev_ne), (double)ws.wB / 512.0);
        ws.wch = (double)top_cell > delta ? (uint32_t)((double)top_cell - delta) : 0u;
      }
      prev_top_cell = top_cell; prev_ne = n_edges;
    }
    // a run that placed horizons and is left without one -- no room (the top has come within delta of cell 0) or, what ends a
    // 1024^3 run, too few items (n <= 4096): every created edge now gets its record, its list push and its count, nearly all die
    // at the next contraction of the same hub, and the cell lists keep them until a baseline drops them.  The interval, tuned for
    // 90 % of the created edges staying out of the lists, is cut by rebase_end
    if (horizon_factor > 0.0 && prev_top_cell >= 0 && n_edges > E0 && ws.wch == 0) ws.rebase_after = std::max<unsigned long long>(1ull, ws.rebase_after / rebase_end);
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

// Runs the pb-mean, median or pre_merge greedy merge on a compact RAG; the order is in dense ids (MergeResult).
static int run_pb_loop(const RagArrays& rag, hipStream_t stream, const PbRequest& req, MergeResult* out) {
  const long long P = rag.P;
  const uint32_t R = (uint32_t)rag.R;
  if (R == 0 || P == 0) return GLIA_HMT_OK;
  const VolumeRef* median_of = req.median_of;
  CallEvents<3> ev;
  int rc;
  if ((rc = ev.create())) return rc;
  GLIA_HIP_TRY(hipEventRecord(ev.ev[0], stream));
  DeviceBuffers buf;
  uint32_t* flag; uint32_t* eidx; long long* partner;
  if ((rc = buf.get(&flag, P + 1, true, stream))) return rc;
  if ((rc = buf.get(&eidx, P + 1, false, stream))) return rc;
  if ((rc = buf.get(&partner, P, false, stream))) return rc;
  hipLaunchKernelGGL(edge_flags, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, stream, rag.d_pa, rag.d_pb, P, flag, partner);
  if ((rc = rocprim_run(buf, stream, [&](void* t, size_t& b) {
        return rocprim::exclusive_scan(t, b, flag, eidx, 0u, (size_t)(P + 1), rocprim::plus<uint32_t>(), stream); }))) return rc;
  uint32_t E0 = 0;
  GLIA_HIP_TRY(hipMemcpyAsync(&E0, eidx + P, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  GLIA_HIP_TRY(hipStreamSynchronize(stream));
  if (E0 == 0) return GLIA_HMT_OK;

  GreedyState st;
  memset(&st, 0, sizeof(st));
  st.R0 = R;
  // created edges are never reused: a 1024^3 run ends at ~16.4 x E0 edge slots and ~33 x E0 list entries (measured) --
  // sized so that the usual run never stops to grow (growth = a relaunch plus a copy of gigabytes)
  const bool mincap = initial_capacities(E0, 18, 36, &st.Ecap, &st.pool_cap);
  if ((rc = buf.get(&st.adj_off, 2 * (size_t)R, true, stream))) return rc;
  if ((rc = buf.get(&st.adj_len, 2 * (size_t)R + 1, true, stream))) return rc;
  // pb-mean linkage (with or without the pre_merge condition) runs on the window queue; GLIA_HMT_PB_WINDOW=0 keeps the
  // tournament tree (kernel experiments, parity gate: both must give byte-identical results)
  std::string o_window, o_batch, o_txt;
  const bool batch_off = option("GLIA_HMT_PB_BATCH", &o_batch) && o_batch[0] == '0';      // one contraction at a time on the window queue (same result)
  bool window = !median_of && !req.size_weight && !(option("GLIA_HMT_PB_WINDOW", &o_window) && o_window[0] == '0');
  WinState ws;
  memset(&ws, 0, sizeof(ws));
  GrowList edges, entries, values;              // the arrays indexed by edge slot, by list entry, by value
  if (window) {
    if ((rc = entries.add(buf, &ws.fpool, st.pool_cap, stream))) return rc;
    if ((rc = edges.add(buf, &ws.er, st.Ecap, stream))) return rc;
    if ((rc = edges.add(buf, &ws.ecat, st.Ecap, stream))) return rc;
  }
  else if ((rc = entries.add(buf, &st.pool, st.pool_cap, stream))) return rc;
  if ((rc = edges.add(buf, &st.e_u, st.Ecap, stream)) || (rc = edges.add(buf, &st.e_v, st.Ecap, stream)) ||
      (rc = edges.add(buf, &st.e_posu, st.Ecap, stream)) || (rc = edges.add(buf, &st.e_posv, st.Ecap, stream)) ||
      (rc = edges.add(buf, &st.e_mean, st.Ecap, stream)) || (rc = edges.add(buf, &st.e_n, st.Ecap, stream, true)) ||
      (rc = edges.add(buf, &st.pq.leaf_sal, st.Ecap, stream)) || (rc = edges.add(buf, &st.pq.leaf_seq, st.Ecap, stream)))
    return rc;
  st.pq.nleaves = st.Ecap;
  if ((rc = buf.get(&st.rsz, 2 * (size_t)R, true, stream))) return rc;
  if ((rc = buf.get(&st.rsum, 2 * (size_t)R, true, stream))) return rc;
  st.cond_n = req.cond_n; st.cond_rpb = req.cond_rpb; st.size_weight = req.size_weight ? 1 : 0;
  st.cond_t0 = req.cond_n > 0 ? (unsigned long long)req.cond_sizes[0] : 0; st.cond_t1 = req.cond_n > 1 ? (unsigned long long)req.cond_sizes[1] : 0;
  hipLaunchKernelGGL(region_sizes, dim3((R + 255) / 256), dim3(256), 0, stream, rag.d_rrec, R, st.rsz, st.rsum);
  if ((rc = buf.get(&st.mark0, 2 * (size_t)R, true, stream))) return rc;
  if ((rc = buf.get(&st.mark1, 2 * (size_t)R, true, stream))) return rc;
  // (+ kNW entries: a loop whose state is corrupt is stopped when k reaches R, at most one round of the batch kernel later)
  if ((rc = buf.get(&st.order, 3 * ((size_t)R + 16), false, stream))) return rc;
  if ((rc = buf.get(&st.sal_out, (size_t)R + 16, false, stream))) return rc;
  if ((rc = buf.get(&st.ctrl, 16, true, stream))) return rc;
  uint32_t* cursor;
  if ((rc = buf.get(&cursor, 2 * (size_t)R, true, stream))) return rc;

  hipLaunchKernelGGL(fill_leaves_dead, dim3((st.Ecap - E0 + 255) / 256), dim3(256), 0, stream, st.pq, E0);
  hipLaunchKernelGGL(edge_fill, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, stream, rag.d_pa, rag.d_pb, rag.d_prec, P,
                     flag, eidx, partner, rag.d_rlabel, R, st, st.adj_len);
  // adjacency offsets = exclusive scan of the degrees (adj_len[0..R) holds them, the rest is zero)
  if ((rc = rocprim_run(buf, stream, [&](void* t, size_t& b) {
        return rocprim::exclusive_scan(t, b, st.adj_len, st.adj_off, 0u, (size_t)R, rocprim::plus<uint32_t>(), stream); }))) return rc;
  if (window) hipLaunchKernelGGL(adj_fill_fat, dim3((E0 + 255) / 256), dim3(256), 0, stream, st, ws, E0, cursor);
  else hipLaunchKernelGGL(adj_fill, dim3((E0 + 255) / 256), dim3(256), 0, stream, st, E0, cursor);
  GLIA_HIP_TRY(hipGetLastError());
  unsigned long long n_values = 0;
  if (median_of) {
    // sorted value runs: offsets = scan of the edges' voxel counts, one scatter pass over the volume, segmented sort
    if ((rc = edges.add(buf, &st.e_off, st.Ecap, stream))) return rc;
    if ((rc = buf.get(&st.rbv, 2 * (size_t)R, true, stream))) return rc;
    if ((rc = rocprim_run(buf, stream, [&](void* t, size_t& b) {
          return rocprim::exclusive_scan(t, b, st.e_n, st.e_off, 0ull, (size_t)E0 + 1, rocprim::plus<unsigned long long>(), stream); }))) return rc;
    GLIA_HIP_TRY(hipMemcpyAsync(&n_values, st.e_off + E0, sizeof(n_values), hipMemcpyDeviceToHost, stream));
    GLIA_HIP_TRY(hipStreamSynchronize(stream));
    if (n_values >= 0xFFFFFFFFull) { set_error("merge_order_pb: more than 2^32 boundary voxels (median linkage)"); return GLIA_HMT_ERR_ARG; }
    st.vals_cap = mincap ? std::max(n_values, 1ull) : n_values * 4ull + (1ull << 20);
    float* unsorted;
    if ((rc = values.add(buf, &st.vals, (size_t)st.vals_cap, stream))) return rc;
    if ((rc = buf.get(&unsorted, (size_t)n_values, false, stream))) return rc;
    uint32_t* vcursor;
    if ((rc = buf.get(&vcursor, (size_t)E0, true, stream))) return rc;
    if (median_of->lab) {
      const long long N = median_of->nx * median_of->ny * median_of->nz;
      hipLaunchKernelGGL(median_collect, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, *median_of, rag.d_pa, rag.d_pb, P,
                         flag, eidx, st.e_off, vcursor, unsorted);
    } else {
      if (!rag.d_pv_off) { set_error("merge_order_pb: median linkage needs the volume or the map's boundary values"); return GLIA_HMT_ERR_UNSUPPORTED; }
      if (rag.nV) hipLaunchKernelGGL(median_from_runs, dim3((unsigned)((rag.nV + 255) / 256)), dim3(256), 0, stream, rag.d_pv_off, rag.d_pv, rag.nV, rag.d_pa, rag.d_pb,
                                     (long long)P, flag, eidx, st.e_off, unsorted);
    }
    GLIA_HIP_TRY(hipGetLastError());
    if ((rc = rocprim_run(buf, stream, [&](void* t, size_t& b) {
          return rocprim::segmented_radix_sort_keys(t, b, unsorted, st.vals, (unsigned)n_values, (unsigned)E0, st.e_off, st.e_off + 1, 0, 32, stream); }))) return rc;
    hipLaunchKernelGGL(median_init, dim3((E0 + 255) / 256), dim3(256), 0, stream, st, E0);
    GLIA_HIP_TRY(hipGetLastError());
  }
  unsigned long long ctrl[CTRL_WORDS] = {};
  ctrl[CTRL_EDGES] = E0; ctrl[CTRL_ENTRIES] = 2ull * E0; ctrl[CTRL_STATUS] = ST_RUN; ctrl[CTRL_VALUES] = n_values;
  WinBaseline base;
  if (window) {
    // saliency cells: ~4 initial edges per cell on average
    uint32_t B = 256;
    while (B < E0 / 4 && B < (1u << 22)) B <<= 1;
    ws.wB = B; ws.R0 = R;
    ws.wcap = kWinCap; ws.wbudget = kWinBudget;
    ws.force_tree = 0;
    if (option("GLIA_HMT_FORCE_TREE", &o_txt)) ws.force_tree = strtoull(o_txt.c_str(), nullptr, 10);
    if (option("GLIA_HMT_WINCAP", &o_txt)) {                             // tests: a tiny window makes spills, evictions and cell splits routine
      const uint32_t c = (uint32_t)strtoul(o_txt.c_str(), nullptr, 10);
      if (c >= 16 && c <= kWinCap) { ws.wcap = c; ws.wbudget = c / 2; }
    }
    ws.order = st.order; ws.sal_out = st.sal_out; ws.ctrl = st.ctrl; ws.rsz = st.rsz; ws.rsum = st.rsum;
    ws.mark0 = st.mark0; ws.mark1 = st.mark1; ws.adj_off = st.adj_off; ws.adj_len = st.adj_len;
    ws.pool_cap = st.pool_cap; ws.Ecap = st.Ecap;
    ws.cond_n = st.cond_n; ws.cond_t0 = st.cond_t0; ws.cond_t1 = st.cond_t1; ws.cond_rpb = st.cond_rpb;
    if ((rc = base.init(buf, ws, st.pq.leaf_sal, E0, B, R, stream))) return rc;
    // the horizon: 0 = off; else the factor on the measured descent (swept 0.05 .. 8 at 1024^3: flat from 0.1 to 0.5, +1 % at 2, +2 % at 4)
    if (req.cond_n <= 0 && !batch_off) base.horizon_factor = option("GLIA_HMT_HORIZON", &o_txt) ? atof(o_txt.c_str()) : 0.5;
    // the batch kernel keeps rdead and writes no record below its horizon: its baselines come from the lists of the live regions.  The
    // one-at-a-time kernel (pre_merge, GLIA_HMT_PB_BATCH=0) has neither -- a rejected edge stays in the lists with seq == 0 -- and
    // keeps the scan of the records
    base.from_lists = req.cond_n <= 0 && !batch_off;
    if ((rc = base.rebaseline(ws, E0, ctrl, stream))) return rc;
  } else if ((rc = pq_setup(buf, st.pq, stream))) return rc;
  GLIA_HIP_TRY(hipMemcpyAsync(st.ctrl, ctrl, sizeof(ctrl), hipMemcpyHostToDevice, stream));
  GLIA_HIP_TRY(hipEventRecord(ev.ev[1], stream));


  // ---- the loop, in bounded launches so a contraction budget can be re-negotiated between them ----
  st.max_iters = window ? 1ull << 22 : 1ull << 16;
  const bool trace = option("GLIA_HMT_TRACE");
  if (option("GLIA_HMT_MAXITERS", &o_txt)) st.max_iters = std::max(1ull, strtoull(o_txt.c_str(), nullptr, 10));      // tests: launches that end early
  const auto kernel = [&]() { return !window ? "tree" : req.cond_n > 0 ? "window" : "batch"; };
  const auto unhandled = [&]() {
    set_error(std::string("greedy: the ") + kernel() + " kernel stopped with status " + std::to_string(ctrl[CTRL_STATUS]) + ", which its driver does not handle (internal error)");
    return GLIA_HMT_ERR_INTERNAL;
  };
  while (true) {
    if (window) {
      ws.max_iters = st.max_iters;
      if (req.cond_n > 0) hipLaunchKernelGGL(greedy_window_kernel<true>, dim3(1), dim3(kGreedyThreads), 0, stream, ws);
      else if (batch_off) hipLaunchKernelGGL(greedy_window_kernel<false>, dim3(1), dim3(kGreedyThreads), 0, stream, ws);
      else hipLaunchKernelGGL(greedy_batch_kernel, dim3(1), dim3(kGreedyThreads), 0, stream, ws);
    } else if (median_of) hipLaunchKernelGGL(greedy_pb_kernel<true>, dim3(1), dim3(kGreedyThreads), 0, stream, st);
    else hipLaunchKernelGGL(greedy_pb_kernel<false>, dim3(1), dim3(kGreedyThreads), 0, stream, st);
    GLIA_HIP_TRY(hipGetLastError());
    GLIA_HIP_TRY(hipMemcpyAsync(ctrl, st.ctrl, sizeof(ctrl), hipMemcpyDeviceToHost, stream));
    GLIA_HIP_TRY(hipStreamSynchronize(stream));
    if (trace) fprintf(stderr, "[trace] merge loop launch ended: status %llu, merges %llu of %u regions, edges %llu, list entries %llu, records rebuilt %llu, baseline items %u, horizon %u, interval %llu\n", ctrl[CTRL_STATUS], ctrl[CTRL_MERGES], R, ctrl[CTRL_EDGES], ctrl[CTRL_ENTRIES], base.rebuilt_last, ws.nsort, ws.wch, ws.rebase_after);      // (rebuilt: by the baseline or hand-over in front of this launch)
    base.rebuilt_last = 0;
    if (ctrl[CTRL_STATUS] == ST_DONE) break;
    switch (ctrl[CTRL_STATUS]) {
      case ST_RUN:                              // max_iters reached: the tree kernel goes on from its state, the window queue re-baselines
        if (!window) continue;
        break;
      case ST_REBASE:
        if (!window) return unhandled();
        break;
      case ST_BAD_SALIENCY: set_error("Error: invalid boundary saliency..."); return GLIA_HMT_ERR_SALIENCY;
      case ST_INTERNAL: {
        char msg[256];
        snprintf(msg, sizeof(msg), "greedy: window queue overflow or more merges than regions (internal error: merges %llu of %u regions, %llu edges of %u initial, "
                 "window %llu%s, %s kernel)", ctrl[CTRL_MERGES], R, ctrl[CTRL_EDGES], E0, ctrl[CTRL_WFILL], ctrl[CTRL_WERR] ? " overflowed" : "", kernel());
        set_error(msg);
        return GLIA_HMT_ERR_INTERNAL;
      }
      case ST_NEED_TREE:
        // a saliency cell with more live items than the window holds (massive exact ties): the tournament tree takes over
        // from the same state -- leaf keys are the ground truth of both queues, the lists get their thin entries
        if (!window) return unhandled();
        entries.remove(&ws.fpool);
        edges.remove(&ws.er);
        edges.remove(&ws.ecat);
        if ((rc = entries.add(buf, &st.pool, st.pool_cap, stream))) return rc;
        hipLaunchKernelGGL(fat_to_thin, dim3((unsigned)((ctrl[CTRL_ENTRIES] + 255) / 256)), dim3(256), 0, stream, ws.fpool, st.pool, ctrl[CTRL_ENTRIES]);
        if (base.from_lists) {
          // the batch kernel's edges below the horizon have no records yet: the collection pass of a baseline rebuilds those of the
          // live ones and lists every live edge; the rest of the leaves are dead
          uint32_t n_live = 0;
          if ((rc = base.collect(ws, (uint32_t)ctrl[CTRL_EDGES], R + (uint32_t)ctrl[CTRL_MERGES], stream, &n_live))) return rc;
          hipLaunchKernelGGL(fill_leaves_dead, dim3((st.Ecap + 255) / 256), dim3(256), 0, stream, st.pq, 0u);
          if (n_live) hipLaunchKernelGGL(edge_unpack_live, dim3((n_live + 255) / 256), dim3(256), 0, stream, st, ws.er, base.vals, n_live);
        } else
        hipLaunchKernelGGL(edge_unpack, dim3((unsigned)((ctrl[CTRL_EDGES] + 255) / 256)), dim3(256), 0, stream, st, ws.er, ws.rdead, (uint32_t)ctrl[CTRL_EDGES]);
        GLIA_HIP_TRY(hipGetLastError());
        if ((rc = pq_setup(buf, st.pq, stream))) return rc;
        window = false;
        st.max_iters = 1ull << 16;
        break;
      case ST_NEED_POOL: {
        const unsigned long long ncap = st.pool_cap * 2;
        if ((rc = entries.grow(buf, (size_t)st.pool_cap, (size_t)ncap, stream))) return rc;
        st.pool_cap = ncap; ws.pool_cap = ncap;
        break;
      }
      case ST_NEED_VALUES: {
        if (!median_of) return unhandled();
        const unsigned long long ncap = st.vals_cap * 2;
        if ((rc = values.grow(buf, (size_t)ctrl[CTRL_VALUES], (size_t)ncap, stream))) return rc;
        st.vals_cap = ncap;
        break;
      }
      case ST_NEED_EDGES: {
        if (st.Ecap >= kMaxEdgeSlots) { set_error("greedy: more than 2^32 edge slots needed"); return GLIA_HMT_ERR_ARG; }
        const uint32_t ocap = st.Ecap, ncap = (uint32_t)std::min<unsigned long long>(kMaxEdgeSlots, (unsigned long long)ocap * 2ull);
        if ((rc = edges.grow(buf, ocap, ncap, stream))) return rc;
        st.Ecap = ncap; st.pq.nleaves = ncap; ws.Ecap = ncap;
        hipLaunchKernelGGL(fill_leaves_dead, dim3((ncap - ocap + 255) / 256), dim3(256), 0, stream, st.pq, ocap);
        if (!window && (rc = pq_setup(buf, st.pq, stream))) return rc;
        break;
      }
      default: return unhandled();
    }
    if (window) {
      // the launch left through the lists (everything alive sits there): a fresh baseline, an empty window
      if ((rc = base.rebaseline(ws, (uint32_t)ctrl[CTRL_EDGES], ctrl, stream))) return rc;
      GLIA_HIP_TRY(hipMemcpyAsync(st.ctrl + CTRL_CTHR, ctrl + CTRL_CTHR, 4 * sizeof(unsigned long long), hipMemcpyHostToDevice, stream));
    }
    unsigned long long zero = ST_RUN;
    GLIA_HIP_TRY(hipMemcpyAsync(st.ctrl + CTRL_STATUS, &zero, sizeof(zero), hipMemcpyHostToDevice, stream));
  }
  GLIA_HIP_TRY(hipEventRecord(ev.ev[2], stream));
  GLIA_HIP_TRY(hipEventSynchronize(ev.ev[2]));
  out->ms_table = ev.ms(0, 1); out->ms_loop = ev.ms(1, 2);
  out->n_scored = (int64_t)ctrl[CTRL_EDGES];
  return copy_merges(out, (int64_t)ctrl[CTRL_MERGES], st.order, st.sal_out);
}


// Every merge of a correct order joins two regions that still exist and creates region R + k (util/struct_merge.hxx:19-31: the loop
// appends (r0, r1, key++) and erases both regions' items).  Every merge loop replays its order against this rule on the host before
// it returns it -- an O(R) pass, ~1 ms at 262 144 regions -- and a violation is an ERROR (GLIA_HMT_ERR_INTERNAL), never a silent
// second run: round 3 re-ran such calls (a net under the window kernel's race on its edge counter), which let a
// kernel defect pass every test.  glia_hmt_internal_errors() counts the calls that ended this way.
static std::atomic<unsigned long long> g_internal_errors{0};
unsigned long long internal_errors() { return g_internal_errors.load(); }
void count_internal_error() { g_internal_errors.fetch_add(1); }
bool merge_order_is_consistent(const uint32_t* o, int64_t n, uint32_t R, int64_t* first_bad) {
  std::vector<uint8_t> gone(2 * (size_t)R + 1, 0);
  for (int64_t k = 0; k < n; ++k) {
    const uint32_t a = o[3 * k], b = o[3 * k + 1], c = o[3 * k + 2];
    if (k >= (int64_t)R || c != R + (uint32_t)k || a >= c || b >= c || a == b || gone[a] || gone[b]) { if (first_bad) *first_bad = k; return false; }
    gone[a] = gone[b] = 1;
  }
  return true;
}
int finish_merge_order(int rc, const uint32_t* o, int64_t n, uint32_t R, hipStream_t stream) {
  int64_t bad = -1;
  if (rc == GLIA_HMT_OK && !merge_order_is_consistent(o, n, R, &bad)) {
    set_error("greedy: merge " + std::to_string(bad) + " of " + std::to_string(n) + " joins a region that does not exist (any more) or creates the wrong one (internal error)");
    rc = GLIA_HMT_ERR_INTERNAL;
  }
  if (rc == GLIA_HMT_ERR_INTERNAL) { count_internal_error(); (void)hipStreamSynchronize(stream); }
  return rc;
}
int greedy_mean(const RagArrays& rag, hipStream_t stream, const PbRequest& req, MergeResult* out) {
  const int rc = run_pb_loop(rag, stream, req, out);
  return finish_merge_order(rc, out->order.data(), out->n, (uint32_t)rag.R, stream);
}

}  // namespace glia
