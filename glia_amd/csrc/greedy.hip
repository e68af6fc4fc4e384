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
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "greedy_baseline.hpp"   // <- greedy_batch.hpp <- greedy_window.hpp <- greedy_tree.hpp <- greedy_common.hpp: the three loops and the baseline chain

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

// The options of a pb loop call, read once at its top (GLIA_HMT_MINCAP: initial_capacities, shared with the classifier loop).
struct PbOptions {
  bool window_off = false, batch_off = false;      // the tournament tree; one contraction at a time on the window queue (parity gates: byte-identical results)
  uint32_t wincap = 0, collect_lanes = 0;    // tests: a tiny window makes spills, evictions and cell splits routine; lanes per region of the collection pass (0: unset)
  double horizon = 0.5;                      // 0 = off; else the factor on the measured descent (swept 0.05 .. 8 at 1024^3: flat from 0.1 to 0.5, +1 % at 2, +2 % at 4)
  unsigned long long force_tree = 0, max_iters = 0;      // max_iters: tests, launches that end early (0: unset)
  bool trace = false, audit = false, rebase_set = false;
  unsigned long long rebase = 0, rebase_end = 8;      // BaselinePolicy
  PbOptions() {
    std::string t;
    window_off = option("GLIA_HMT_PB_WINDOW", &t) && t[0] == '0';
    batch_off = option("GLIA_HMT_PB_BATCH", &t) && t[0] == '0';
    if (option("GLIA_HMT_FORCE_TREE", &t)) force_tree = strtoull(t.c_str(), nullptr, 10);
    if (option("GLIA_HMT_WINCAP", &t)) wincap = (uint32_t)strtoul(t.c_str(), nullptr, 10);
    if (option("GLIA_HMT_HORIZON", &t)) horizon = atof(t.c_str());
    if (option("GLIA_HMT_MAXITERS", &t)) max_iters = std::max(1ull, strtoull(t.c_str(), nullptr, 10));
    trace = option("GLIA_HMT_TRACE");
    if ((rebase_set = option("GLIA_HMT_REBASE", &t))) rebase = strtoull(t.c_str(), nullptr, 10);
    if (option("GLIA_HMT_REBASE_END", &t)) rebase_end = std::max(1ull, strtoull(t.c_str(), nullptr, 10));
    if (option("GLIA_HMT_COLLECT_LANES", &t)) collect_lanes = (uint32_t)strtoul(t.c_str(), nullptr, 10);
    audit = option("GLIA_HMT_BASELINE_AUDIT", &t) && t[0] != '0';
  }
};

// One pb loop call: what it holds between its steps, and the steps run_pb_loop calls in order.
struct PbRun {
  const RagArrays& rag; hipStream_t stream; const PbRequest& req; const PbOptions& opt;
  uint32_t R, E0 = 0;
  DeviceBuffers buf;
  GrowList edges, entries, values;           // the arrays indexed by edge slot, by list entry, by value
  GreedyState st = {}; WinState ws = {}; WinBaseline base;
  uint32_t *flag = nullptr, *eidx = nullptr; // per directed pair: whether it owns a table edge, and the edge's slot
  bool window = false, mincap = false;
  unsigned long long ctrl[CTRL_WORDS] = {};  // the host's copy of st.ctrl
  const char* kernel() const { return !window ? "tree" : req.cond_n > 0 ? "window" : "batch"; }
  int unhandled() const {
    set_error(std::string("greedy: the ") + kernel() + " kernel stopped with status " + std::to_string(ctrl[CTRL_STATUS]) + ", which its driver does not handle (internal error)");
    return GLIA_HMT_ERR_INTERNAL;
  }
  // Step 1, the edge table: one edge per mutual pair, the loop's arrays, the initial incident-edge lists.  E0 stays 0 without an edge.
  int edge_table() {
    const long long P = rag.P;
    int rc; long long* partner;
    if ((rc = buf.get(&flag, P + 1, true, stream))) return rc;
    if ((rc = buf.get(&eidx, P + 1, false, stream))) return rc;
    if ((rc = buf.get(&partner, P, false, stream))) return rc;
    hipLaunchKernelGGL(edge_flags, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, stream, rag.d_pa, rag.d_pb, P, flag, partner);
    if ((rc = rocprim_run(buf, stream, [&](void* t, size_t& b) {
          return rocprim::exclusive_scan(t, b, flag, eidx, 0u, (size_t)(P + 1), rocprim::plus<uint32_t>(), stream); }))) return rc;
    GLIA_HIP_TRY(hipMemcpyAsync(&E0, eidx + P, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    GLIA_HIP_TRY(hipStreamSynchronize(stream));
    if (E0 == 0) return GLIA_HMT_OK;
    st.R0 = R;
    // created edges are never reused: a 1024^3 run ends at ~16.4 x E0 edge slots and ~33 x E0 list entries (measured) --
    // sized so that the usual run never stops to grow (growth = a relaunch plus a copy of gigabytes)
    mincap = initial_capacities(E0, 18, 36, &st.Ecap, &st.pool_cap);
    if ((rc = buf.get(&st.adj_off, 2 * (size_t)R, true, stream)) || (rc = buf.get(&st.adj_len, 2 * (size_t)R + 1, true, stream))) return rc;
    // pb-mean linkage (with or without the pre_merge condition) runs on the window queue
    window = !req.median_of && !req.size_weight && !opt.window_off;
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
    if ((rc = buf.get(&st.rsz, 2 * (size_t)R, true, stream)) || (rc = buf.get(&st.rsum, 2 * (size_t)R, true, stream))) return rc;
    st.cond_n = req.cond_n; st.cond_rpb = req.cond_rpb; st.size_weight = req.size_weight ? 1 : 0;
    st.cond_t0 = req.cond_n > 0 ? (unsigned long long)req.cond_sizes[0] : 0; st.cond_t1 = req.cond_n > 1 ? (unsigned long long)req.cond_sizes[1] : 0;
    hipLaunchKernelGGL(region_sizes, dim3((R + 255) / 256), dim3(256), 0, stream, rag.d_rrec, R, st.rsz, st.rsum);
    if ((rc = buf.get(&st.mark0, 2 * (size_t)R, true, stream)) || (rc = buf.get(&st.mark1, 2 * (size_t)R, true, stream))) return rc;
    // (+ kNW entries: a loop whose state is corrupt is stopped when k reaches R, at most one round of the batch kernel later)
    if ((rc = buf.get(&st.order, 3 * ((size_t)R + 16), false, stream)) || (rc = buf.get(&st.sal_out, (size_t)R + 16, false, stream))) return rc;
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
    ctrl[CTRL_EDGES] = E0; ctrl[CTRL_ENTRIES] = 2ull * E0; ctrl[CTRL_STATUS] = ST_RUN;
    return GLIA_HMT_OK;
  }
  // Step 2, median linkage: sorted value runs -- offsets = scan of the edges' voxel counts, one scatter pass over the volume, segmented sort
  int median_setup() {
    const VolumeRef* median_of = req.median_of; const long long P = rag.P;
    int rc;
    if ((rc = edges.add(buf, &st.e_off, st.Ecap, stream))) return rc;
    if ((rc = buf.get(&st.rbv, 2 * (size_t)R, true, stream))) return rc;
    if ((rc = rocprim_run(buf, stream, [&](void* t, size_t& b) {
          return rocprim::exclusive_scan(t, b, st.e_n, st.e_off, 0ull, (size_t)E0 + 1, rocprim::plus<unsigned long long>(), stream); }))) return rc;
    unsigned long long n_values = 0;
    GLIA_HIP_TRY(hipMemcpyAsync(&n_values, st.e_off + E0, sizeof(n_values), hipMemcpyDeviceToHost, stream));
    GLIA_HIP_TRY(hipStreamSynchronize(stream));
    if (n_values >= 0xFFFFFFFFull) { set_error("merge_order_pb: more than 2^32 boundary voxels (median linkage)"); return GLIA_HMT_ERR_ARG; }
    ctrl[CTRL_VALUES] = n_values;
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
    return GLIA_HMT_OK;
  }
  // Step 3, the window queue: its cells, its view of the loop's arrays, and the first baseline (of the initial edges)
  int window_setup() {
    const uint32_t B = plan_cells(E0);
    ws.wB = B; ws.R0 = R;
    ws.wcap = kWinCap; ws.wbudget = kWinBudget;
    ws.force_tree = opt.force_tree;
    if (opt.wincap >= 16 && opt.wincap <= kWinCap) { ws.wcap = opt.wincap; ws.wbudget = opt.wincap / 2; }
    ws.order = st.order; ws.sal_out = st.sal_out; ws.ctrl = st.ctrl; ws.rsz = st.rsz; ws.rsum = st.rsum;
    ws.mark0 = st.mark0; ws.mark1 = st.mark1; ws.adj_off = st.adj_off; ws.adj_len = st.adj_len;
    ws.pool_cap = st.pool_cap; ws.Ecap = st.Ecap;
    ws.cond_n = st.cond_n; ws.cond_t0 = st.cond_t0; ws.cond_t1 = st.cond_t1; ws.cond_rpb = st.cond_rpb;
    base.lanes_forced = opt.collect_lanes; base.audit = opt.audit;
    base.policy.rebase_set = opt.rebase_set; base.policy.rebase = opt.rebase; base.policy.rebase_end = opt.rebase_end;
    if (int rc = base.init(buf, ws, st.pq.leaf_sal, E0, B, R, stream)) return rc;
    // the batch kernel keeps rdead and writes no record below its horizon: its baselines come from the lists of the live regions.  The
    // one-at-a-time kernel (pre_merge, GLIA_HMT_PB_BATCH=0) has neither -- a rejected edge stays in the lists with seq == 0 -- and
    // keeps the scan of the records, without a horizon
    base.from_lists = req.cond_n <= 0 && !opt.batch_off;
    if (base.from_lists) base.policy.horizon_factor = opt.horizon;
    return base.rebaseline(ws, E0, ctrl, stream);
  }
  // Step 4, ST_NEED_TREE: a saliency cell with more live items than the window holds (massive exact ties): the tournament tree takes
  // over from the same state -- leaf keys are the ground truth of both queues, the lists get their thin entries
  int hand_over() {
    int rc;
    entries.remove(&ws.fpool); edges.remove(&ws.er); edges.remove(&ws.ecat);
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
    return GLIA_HMT_OK;
  }
  // Step 5, the loop, in bounded launches so a contraction budget can be re-negotiated between them
  int launch_loop() {
    int rc;
    st.max_iters = opt.max_iters ? opt.max_iters : window ? 1ull << 22 : 1ull << 16;
    while (true) {
      if (window) {
        ws.max_iters = st.max_iters;
        if (req.cond_n > 0) hipLaunchKernelGGL(greedy_window_kernel<true>, dim3(1), dim3(kGreedyThreads), 0, stream, ws);
        else if (opt.batch_off) hipLaunchKernelGGL(greedy_window_kernel<false>, dim3(1), dim3(kGreedyThreads), 0, stream, ws);
        else hipLaunchKernelGGL(greedy_batch_kernel, dim3(1), dim3(kGreedyThreads), 0, stream, ws);
      } else if (req.median_of) hipLaunchKernelGGL(greedy_pb_kernel<true>, dim3(1), dim3(kGreedyThreads), 0, stream, st);
      else hipLaunchKernelGGL(greedy_pb_kernel<false>, dim3(1), dim3(kGreedyThreads), 0, stream, st);
      GLIA_HIP_TRY(hipGetLastError());
      GLIA_HIP_TRY(hipMemcpyAsync(ctrl, st.ctrl, sizeof(ctrl), hipMemcpyDeviceToHost, stream));
      GLIA_HIP_TRY(hipStreamSynchronize(stream));
      if (opt.trace) fprintf(stderr, "[trace] merge loop launch ended: status %llu, merges %llu of %u regions, edges %llu, list entries %llu, records rebuilt %llu, baseline items %u, horizon %u, interval %llu\n", ctrl[CTRL_STATUS], ctrl[CTRL_MERGES], R, ctrl[CTRL_EDGES], ctrl[CTRL_ENTRIES], base.rebuilt_last, ws.nsort, ws.wch, ws.rebase_after);      // (rebuilt: by the baseline or hand-over in front of this launch)
      base.rebuilt_last = 0;
      if (ctrl[CTRL_STATUS] == ST_DONE) return GLIA_HMT_OK;
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
          if (!window) return unhandled();
          if ((rc = hand_over())) return rc;
          break;
        case ST_NEED_POOL: {
          const unsigned long long ncap = st.pool_cap * 2;
          if ((rc = entries.grow(buf, (size_t)st.pool_cap, (size_t)ncap, stream))) return rc;
          st.pool_cap = ncap; ws.pool_cap = ncap;
          break;
        }
        case ST_NEED_VALUES: {
          if (!req.median_of) return unhandled();
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
  }
};

// Runs the pb-mean, median or pre_merge greedy merge on a compact RAG; the order is in dense ids (MergeResult).
static int run_pb_loop(const RagArrays& rag, hipStream_t stream, const PbRequest& req, MergeResult* out) {
  const PbOptions opt;
  if ((uint32_t)rag.R == 0 || rag.P == 0) return GLIA_HMT_OK;
  CallEvents<3> ev;
  int rc = ev.create();
  if (rc) return rc;
  GLIA_HIP_TRY(hipEventRecord(ev.ev[0], stream));
  PbRun p{rag, stream, req, opt, (uint32_t)rag.R};
  if ((rc = p.edge_table()) || p.E0 == 0) return rc;
  if (req.median_of && (rc = p.median_setup())) return rc;
  if ((rc = p.window ? p.window_setup() : pq_setup(p.buf, p.st.pq, stream))) return rc;
  GLIA_HIP_TRY(hipMemcpyAsync(p.st.ctrl, p.ctrl, sizeof(p.ctrl), hipMemcpyHostToDevice, stream));
  GLIA_HIP_TRY(hipEventRecord(ev.ev[1], stream));
  if ((rc = p.launch_loop())) return rc;
  GLIA_HIP_TRY(hipEventRecord(ev.ev[2], stream));
  GLIA_HIP_TRY(hipEventSynchronize(ev.ev[2]));
  out->ms_table = ev.ms(0, 1); out->ms_loop = ev.ms(1, 2);
  out->n_scored = (int64_t)p.ctrl[CTRL_EDGES];
  return copy_merges(out, (int64_t)p.ctrl[CTRL_MERGES], p.st.order, p.st.sal_out);
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
