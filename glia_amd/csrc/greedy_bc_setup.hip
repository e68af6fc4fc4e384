// glia_amd/csrc/greedy_bc_setup.hip -- the classifier loop's set-up kernels and its host driver: everything of the loop that is the
// same for every instance of its kernels (greedy_bc.hip, where the reference semantics are described), compiled once.  The driver
// builds the state from the compact RAG, then has the instance it is given score the initial edges and run the loop.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "greedy_bc_state.hpp"
#include "median_layout.hpp"
#include "rmap_order.hpp"

namespace glia {

namespace {

// ---- initialisation kernels ---------------------------------------------------------------------------
// per channel c; the structural fields are written by the channel-0 launch
__global__ void bc_leaf_entries(BcState st, int c, const uint32_t* pa, const uint32_t* pb, const uint32_t* prec,
                                const uint32_t* rlabel, long long* partner, int bins, int nthr) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= st.P) return;
  if (c == 0) {
    const uint32_t a = pa[i], b = pb[i];
    const long long j = find_pair(pa, pb, st.P, b, a);
    partner[i] = j;
    st.le_mutual[i] = j >= 0;
    const uint32_t src = find_label(rlabel, st.R0, a), dst = find_label(rlabel, st.R0, b);
    st.le_src[i] = src; st.le_dst[i] = dst; st.le_next[i] = kNone;
    if (j < 0) atomicAdd(&st.nm_out[src], 1u);
  }
  const uint32_t* w = &prec[(size_t)i * kPairWords];
  EStats s;
  estats_clear(s);
  s.n = w[P_CNT];
  for (int t = 0; t < nthr; ++t) s.thr[t] = w[P_THR + t];
  s.mn = ord_float(~w[P_MIN]); s.mx = ord_float(w[P_MAX]);
  memcpy(&s.sum, &w[P_SUM], 8); memcpy(&s.sq, &w[P_SQ], 8);
  for (int k = 0; k < bins; ++k) s.hist[k] = w[P_HIST + k];
  st.ch[c].le_stats[i] = s;
}

// first out-entry of every leaf (pairs ascend by source label): lower bound of the leaf's label in pa
__global__ void bc_leaf_starts(BcState st, const uint32_t* pa, const uint32_t* rlabel) {
  uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r > st.R0) return;
  if (r == st.R0) { st.le_start[r] = (uint32_t)st.P; return; }
  const uint32_t key = rlabel[r];
  long long lo = 0, hi = st.P;
  while (lo < hi) { long long mid = (lo + hi) >> 1; if (pa[mid] < key) lo = mid + 1; else hi = mid; }
  st.le_start[r] = (uint32_t)lo;
}

__global__ void bc_leaf_regions(BcState st, int c, const uint32_t* rrec, int bins) {
  uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= st.R0) return;
  const BcChan& ch = st.ch[c];
  const uint32_t* w = &rrec[(size_t)r * kRegionWords];
  PStats p;
  p.n = w[R_CNT]; p.border = w[R_BORDER];
  for (int d = 0; d < 3; ++d) { p.lo[d] = (int)(0x7fffffffu - w[R_LO + d]); p.hi[d] = (int)w[R_HI + d] - 1; }
  p.mn = ord_float(~w[R_MIN]); p.mx = ord_float(w[R_MAX]);
  memcpy(&p.sum, &w[R_SUM], 8); memcpy(&p.sq, &w[R_SQ], 8);
  for (int k = 0; k < GLIA_HMT_MAX_BINS; ++k) p.hist[k] = k < bins ? w[R_HIST + k] : 0;
  ch.pts[r] = p;
  EStats bn, bt;
  estats_clear(bn); estats_clear(bt);
  for (uint32_t i = st.le_start[r]; i < st.le_start[r + 1]; ++i) {
    estats_add(bt, ch.le_stats[i]);
    if (!st.le_mutual[i]) estats_add(bn, ch.le_stats[i]);
  }
  ch.Bn[r] = bn; ch.Bt[r] = bt; ch.Bmn[r] = bt.mn; ch.Bmx[r] = bt.mx;
  {
    // the same sums, in bin order from +0.0, as the scoring pass forms them (util/stats.hxx:145-152); the log2 of cfg.libm_log2,
    // chosen here at run time, is the one an instance with its libm fixed is only ever picked for (api_loops.cpp)
    double ep = 0.0, eb = 0.0;
    for (int k = 0; k < bins; ++k) { ep = ep - feat::entropy_term(p.hist[k], p.n, st.cfg.libm_log2); eb = eb - feat::entropy_term(bt.hist[k], bt.n, st.cfg.libm_log2); }
    ch.entP[r] = ep; ch.entB[r] = eb;
  }
  if (c == 0) st.parent[r] = r;
}

__global__ void bc_record_flags(BcState st, const uint32_t* pa, const uint32_t* pb, uint32_t* flag) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= st.P) return;
  // one record per unordered leaf pair: owned by the (a<b) entry when it exists, else by the lone (a>b) entry
  flag[i] = (pa[i] < pb[i] || !st.le_mutual[i]) ? 1u : 0u;
}

__global__ void bc_record_fill(BcState st, int c, const uint32_t* flag, const uint32_t* eidx, const long long* partner,
                               const uint32_t* rank, uint32_t* deg) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= st.P || !flag[i]) return;
  const BcChan& ch = st.ch[c];
  const uint32_t e = eidx[i];
  const uint32_t src = st.le_src[i], dst = st.le_dst[i];
  const uint32_t u = src < dst ? src : dst, v = src < dst ? dst : src;
  EStats A, NA;
  estats_clear(A); estats_clear(NA);
  float* d = &ch.e_dir[(size_t)e * 4];
  d[0] = d[2] = __builtin_inff(); d[1] = d[3] = -__builtin_inff();
  const long long j = partner[i];
  if (j >= 0) {            // mutual pair: i = (u -> v), j = (v -> u)
    const EStats& si = ch.le_stats[i];
    const EStats& sj = ch.le_stats[j];
    A = si; estats_add(A, sj);
    d[0] = si.mn; d[1] = si.mx; d[2] = sj.mn; d[3] = sj.mx;
  } else if (st.nm_out[dst]) NA = ch.le_stats[i];
  ch.e_A[e] = A; ch.e_NA[e] = NA;
  if (c != 0) return;
  // structure (once)
  st.e_u[e] = u; st.e_v[e] = v; st.e_alive[e] = 1;
  st.e_orient[e] = rank[u] < rank[v] ? 1 : 0;
  st.e_fhead[e] = st.e_ftail[e] = kNone;
  if (j >= 0) {
    st.e_table[e] = 1;
    st.pq.leaf_seq[e] = (unsigned long long)i + 1ull;      // lexicographic (u,v) order of the table edges
  } else {
    st.e_table[e] = 0;
    if (!st.nm_out[dst]) { st.e_fhead[e] = st.e_ftail[e] = (uint32_t)i; }
  }
  atomicAdd(&deg[u], 1u);
  atomicAdd(&deg[v], 1u);
}

__global__ void bc_adj_fill(BcState st, uint32_t E0, uint32_t* cursor) {
  uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E0) return;
  const uint32_t u = st.e_u[e], v = st.e_v[e];
  const uint32_t pu = atomicAdd(&cursor[u], 1u), pv = atomicAdd(&cursor[v], 1u);
  st.pool[st.adj_off[u] + pu] = e; st.e_posu[e] = pu;
  st.pool[st.adj_off[v] + pv] = e; st.e_posv[e] = pv;
  for (int c = 0; c < st.cfg.K; ++c) {
    const float* d = &st.ch[c].e_dir[(size_t)e * 4];
    st.ch[c].pool_dir[st.adj_off[u] + pu] = make_float2(d[0], d[1]);
    st.ch[c].pool_dir[st.adj_off[v] + pv] = make_float2(d[2], d[3]);
  }
}

// the helpers' copy of the leaves' list headers (BcState::hadj)
__global__ void bc_hadj_fill(BcState st) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < st.R0) st.hadj[r] = (unsigned long long)st.adj_off[r] | ((unsigned long long)st.adj_len[r] << 32);
}

__global__ void bc_init_dead(BcState st, uint32_t from) {
  uint32_t i = from + blockIdx.x * blockDim.x + threadIdx.x;
  if (i < st.Ecap) { st.pq.leaf_seq[i] = 0; st.pq.leaf_sal[i] = -__builtin_inf(); st.e_alive[i] = 0; st.e_table[i] = 0; }
}

// first voxel index of every leaf (the accumulation pass records its complement, R_FIRST) as a sort key
__global__ void bc_first_keys(const uint32_t* rrec, uint32_t R, unsigned long long* keys, uint32_t* leaf) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= R) return;
  const uint2 f = *reinterpret_cast<const uint2*>(&rrec[(size_t)i * kRegionWords + R_FIRST]);
  keys[i] = ~(((unsigned long long)f.y << 32) | f.x);
  leaf[i] = i;
}

}  // namespace

int greedy_bc_run(const BcInstance& inst, const RagArrays& rag, const BcCfg& cfg, const DeviceClassifier& clf, hipStream_t stream,
                  const BcRequest& req, MergeResult* out) {
  const long long P = rag.P;
  const uint32_t R = (uint32_t)rag.R;
  if (R == 0 || P == 0) return GLIA_HMT_OK;
  // the vector is assembled at FULL length (bc_full_dim) and the simple selection compacted in place afterwards: the full length
  // is what the per-thread buffers (double x[kMaxFeat]) hold, not cfg.fdim
  if (bc_full_dim(cfg) > kMaxFeat || cfg.fdim > kMaxFeat) {
    set_error("merge_order_bc: feature vector too long (" + std::to_string(bc_full_dim(cfg)) + " columns before --simpf, limit " + std::to_string(kMaxFeat) + ")");
    return GLIA_HMT_ERR_ARG;
  }
  if (req.median && cfg.fdim + median_extra_cols(cfg) > kMaxFeat) {
    set_error("score_initial_edges: feature vector too long with the median columns (" + std::to_string(cfg.fdim + median_extra_cols(cfg)) + " columns, limit " + std::to_string(kMaxFeat) + ")");
    return GLIA_HMT_ERR_ARG;
  }
  CallEvents<4> ev;
  int rc;
  if ((rc = ev.create())) return rc;
  GLIA_HIP_TRY(hipEventRecord(ev.ev[0], stream));
  DeviceBuffers buf;
  BcState st;
  memset(&st, 0, sizeof(st));
  st.R0 = R; st.P = P; st.cfg = cfg; st.clf = clf;
  if (clf.kind == 2) {
    if (!inst.has_mlp) { set_error("merge_order_bc: this instance of the loop holds no MLP scorer (internal error)"); return GLIA_HMT_ERR_INTERNAL; }
    if (!req.mlp) { set_error("merge_order_bc: an MLP classifier without its model (internal error)"); return GLIA_HMT_ERR_INTERNAL; }
  }
  st.shard = (uint32_t)req.shard; st.n_shards = (uint32_t)(req.n_shards > 0 ? req.n_shards : 1);

  // reference region-map iteration order (rmap_order.cpp): leaves sorted by first voxel on the device, the hashtable replay on the host
  std::vector<uint32_t> lab(R), by_first(R), rank;
  uint32_t* h_stage = nullptr;                // page-locked: [by_first | labels | rank]
  {
    unsigned long long* k0; unsigned long long* k1; uint32_t* v0; uint32_t* v1;
    if ((rc = buf.get(&k0, R, false, stream))) return rc;
    if ((rc = buf.get(&k1, R, false, stream))) return rc;
    if ((rc = buf.get(&v0, R, false, stream))) return rc;
    if ((rc = buf.get(&v1, R, false, stream))) return rc;
    hipLaunchKernelGGL(bc_first_keys, dim3((R + 255) / 256), dim3(256), 0, stream, rag.d_rrec, R, k0, v0);
    if ((rc = rocprim_run(buf, stream, [&](void* t, size_t& b) { return rocprim::radix_sort_pairs(t, b, k0, k1, v0, v1, (size_t)R, 0, 64, stream); }))) return rc;
    if ((rc = PinnedHost::mine().get((void**)&h_stage, sizeof(uint32_t) * 3 * (size_t)R))) return rc;
    GLIA_HIP_TRY(hipMemcpyAsync(h_stage, v1, sizeof(uint32_t) * R, hipMemcpyDeviceToHost, stream));
    GLIA_HIP_TRY(hipMemcpyAsync(h_stage + R, rag.d_rlabel, sizeof(uint32_t) * R, hipMemcpyDeviceToHost, stream));
    GLIA_HIP_TRY(hipStreamSynchronize(stream));
    std::copy(h_stage, h_stage + R, by_first.begin());
    std::copy(h_stage + R, h_stage + 2 * (size_t)R, lab.begin());
  }
  const bool trace = option("GLIA_HMT_TRACE");
  const auto tr0 = std::chrono::steady_clock::now();
  auto tr_ms = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tr0).count(); };
  rmap_ranks_ordered(lab, by_first, &rank);
  if (trace) fprintf(stderr, "[trace] greedy_bc: region-map order replay %.2f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tr0).count());
  uint32_t* d_rank;
  if ((rc = buf.get(&d_rank, R, false, stream))) return rc;
  std::copy(rank.begin(), rank.end(), h_stage + 2 * (size_t)R);
  GLIA_HIP_TRY(hipMemcpyAsync(d_rank, h_stage + 2 * (size_t)R, sizeof(uint32_t) * R, hipMemcpyHostToDevice, stream));
  if (trace) { fprintf(stderr, "[trace] greedy_bc: rank upload queued at %.2f ms\n", tr_ms()); (void)hipStreamSynchronize(stream); fprintf(stderr, "[trace] greedy_bc: rank upload done at %.2f ms\n", tr_ms()); }

  if ((rc = buf.get(&st.le_src, P, false, stream))) return rc;
  if ((rc = buf.get(&st.le_dst, P, false, stream))) return rc;
  for (int c = 0; c < cfg.K; ++c) if ((rc = buf.get(&st.ch[c].le_stats, P, false, stream))) return rc;
  if ((rc = buf.get(&st.le_next, P, false, stream))) return rc;
  if ((rc = buf.get(&st.le_mutual, P, false, stream))) return rc;
  if ((rc = buf.get(&st.le_start, (size_t)R + 1, false, stream))) return rc;
  if ((rc = buf.get(&st.nm_out, R, true, stream))) return rc;
  long long* partner; uint32_t* flag; uint32_t* eidx;
  if ((rc = buf.get(&partner, P, false, stream))) return rc;
  if ((rc = buf.get(&flag, P + 1, true, stream))) return rc;
  if ((rc = buf.get(&eidx, P + 1, false, stream))) return rc;
  if (trace) { (void)hipStreamSynchronize(stream); fprintf(stderr, "[trace] greedy_bc: leaf buffers taken (and zeroed) at %.2f ms\n", tr_ms()); }
  const unsigned gP = (unsigned)((P + 255) / 256);
  for (int c = 0; c < cfg.K; ++c)
    hipLaunchKernelGGL(bc_leaf_entries, dim3(gP), dim3(256), 0, stream, st, c, rag.d_pa, rag.d_pb, rag.c_prec[c], rag.d_rlabel, partner,
                       cfg.cbins[c], cfg.T);
  hipLaunchKernelGGL(bc_leaf_starts, dim3((R + 256) / 256), dim3(256), 0, stream, st, rag.d_pa, rag.d_rlabel);
  hipLaunchKernelGGL(bc_record_flags, dim3(gP), dim3(256), 0, stream, st, rag.d_pa, rag.d_pb, flag);
  if ((rc = rocprim_run(buf, stream, [&](void* t, size_t& b) {
        return rocprim::exclusive_scan(t, b, flag, eidx, 0u, (size_t)(P + 1), rocprim::plus<uint32_t>(), stream); }))) return rc;
  uint32_t E0 = 0;
  GLIA_HIP_TRY(hipMemcpyAsync(&E0, eidx + P, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  GLIA_HIP_TRY(hipStreamSynchronize(stream));
  if (trace) fprintf(stderr, "[trace] greedy_bc: leaf entries + record flags done at %.2f ms\n", tr_ms());
  if (E0 == 0) return GLIA_HMT_OK;

  (void)initial_capacities(E0, 6, 12, &st.Ecap, &st.pool_cap);
  const size_t R2 = 2 * (size_t)R;
  GrowList edges, entries;                      // the arrays indexed by edge slot, by list entry
  for (int c = 0; c < cfg.K; ++c) {
    BcChan& ch = st.ch[c];
    if ((rc = buf.get(&ch.pts, R2, false, stream))) return rc;
    if ((rc = buf.get(&ch.Bn, R2, false, stream))) return rc;
    if ((rc = buf.get(&ch.Bt, R2, false, stream))) return rc;
    if ((rc = buf.get(&ch.Bmn, R2, false, stream))) return rc;
    if ((rc = buf.get(&ch.Bmx, R2, false, stream))) return rc;
    if ((rc = buf.get(&ch.entP, R2, false, stream))) return rc;
    if ((rc = buf.get(&ch.entB, R2, false, stream))) return rc;
    if ((rc = edges.add(buf, &ch.e_A, st.Ecap, stream))) return rc;
    if ((rc = edges.add(buf, &ch.e_NA, st.Ecap, stream))) return rc;
    if ((rc = edges.add(buf, &ch.e_dir, st.Ecap, stream, false, 4))) return rc;
    if ((rc = entries.add(buf, &ch.pool_dir, st.pool_cap, stream))) return rc;
  }
  if ((rc = buf.get(&st.parent, R2, false, stream))) return rc;
  if ((rc = buf.get(&st.adj_off, R2, true, stream))) return rc;
  if ((rc = buf.get(&st.adj_len, R2 + 1, true, stream))) return rc;
  if ((rc = entries.add(buf, &st.pool, st.pool_cap, stream))) return rc;
  if ((rc = edges.add(buf, &st.e_u, st.Ecap, stream)) || (rc = edges.add(buf, &st.e_v, st.Ecap, stream)) ||
      (rc = edges.add(buf, &st.e_posu, st.Ecap, stream)) || (rc = edges.add(buf, &st.e_posv, st.Ecap, stream)) ||
      (rc = edges.add(buf, &st.e_alive, st.Ecap, stream)) || (rc = edges.add(buf, &st.e_table, st.Ecap, stream)) ||
      (rc = edges.add(buf, &st.e_orient, st.Ecap, stream)) || (rc = edges.add(buf, &st.e_fhead, st.Ecap, stream)) ||
      (rc = edges.add(buf, &st.e_ftail, st.Ecap, stream)) || (rc = edges.add(buf, &st.pq.leaf_sal, st.Ecap, stream)) ||
      (rc = edges.add(buf, &st.pq.leaf_seq, st.Ecap, stream)))
    return rc;
  st.pq.nleaves = st.Ecap;
  if ((rc = buf.get(&st.mark0, R2, true, stream))) return rc;
  if ((rc = buf.get(&st.mark1, R2, true, stream))) return rc;
  if ((rc = buf.get(&st.order, 3 * (size_t)R, false, stream))) return rc;
  if ((rc = buf.get(&st.sal_out, (size_t)R, false, stream))) return rc;
  if (req.rows) { if ((rc = buf.get(&st.feats_out, (size_t)R * cfg.fdim, false, stream))) return rc; }
  if ((rc = buf.get(&st.hctl, (size_t)kFlagReps * kFlagStride, true, stream))) return rc;
  if ((rc = buf.get(&st.hrec, (size_t)kJobMax * cfg.K * kRowWords, false, stream))) return rc;
  if ((rc = buf.get(&st.hadj, R2, true, stream))) return rc;
  if ((rc = buf.get(&st.hjob, (size_t)kJobBufs * kJobWords, true, stream))) return rc;
  if ((rc = buf.get(&st.hctl2, (size_t)kFlagReps * kFlagStride, true, stream))) return rc;
  if ((rc = buf.get(&st.hjob2, (size_t)kJobBufs * kJob2Words, true, stream))) return rc;
  if ((rc = buf.get(&st.hvotes, kJobMax, true, stream))) return rc;
  {
    // helper workgroups that score whole records (only a real forest in a scoring run needs them): one per compute unit
    // beside the loop's; GLIA_HMT_HELPERS overrides
    std::string env;
    int nh = option("GLIA_HMT_HELPERS", &env) ? atoi(env.c_str()) : 255;
    if (nh < 0) nh = 0;
    if (nh > 1023) nh = 1023;
    // the loop's workgroup and its helpers talk through polled flags, so they must all be resident at once: never ask for
    // more workgroups than the device can hold of this kernel (a helper that still does not answer -- the device is shared --
    // is noticed by the spin limit and reported as a failed run)
    int per_cu = 0, dev = 0;
    hipDeviceProp_t prop;
    GLIA_HIP_TRY(hipGetDevice(&dev));
    GLIA_HIP_TRY(hipGetDeviceProperties(&prop, dev));
    GLIA_HIP_TRY(inst.loop_workgroups_per_cu(&per_cu));
    const int resident = per_cu * prop.multiProcessorCount;
    if (resident < 1) { set_error("merge_order_bc: the loop kernel does not fit this device"); return GLIA_HMT_ERR_HIP; }
    if (nh > resident - 1) nh = resident - 1;
    st.n_helpers = (clf.kind == 0 && !req.forced && !req.init_only) ? (uint32_t)nh : 0u;
  }
  if ((rc = buf.get(&st.ctrl, 8, true, stream))) return rc;
  uint32_t* cursor;
  if ((rc = buf.get(&cursor, R2, true, stream))) return rc;

  if (trace) fprintf(stderr, "[trace] greedy_bc: buffers taken at %.2f ms\n", tr_ms());
  hipLaunchKernelGGL(bc_init_dead, dim3((st.Ecap + 255) / 256), dim3(256), 0, stream, st, 0u);
  for (int c = 0; c < cfg.K; ++c) {
    hipLaunchKernelGGL(bc_leaf_regions, dim3((R + 255) / 256), dim3(256), 0, stream, st, c, rag.c_rrec[c], cfg.cbins[c]);
    hipLaunchKernelGGL(bc_record_fill, dim3(gP), dim3(256), 0, stream, st, c, flag, eidx, partner, d_rank, st.adj_len);
  }
  if ((rc = rocprim_run(buf, stream, [&](void* t, size_t& b) {
        return rocprim::exclusive_scan(t, b, st.adj_len, st.adj_off, 0u, (size_t)R, rocprim::plus<uint32_t>(), stream); }))) return rc;
  hipLaunchKernelGGL(bc_adj_fill, dim3((E0 + 255) / 256), dim3(256), 0, stream, st, E0, cursor);
  hipLaunchKernelGGL(bc_hadj_fill, dim3((R + 255) / 256), dim3(256), 0, stream, st);
  GLIA_HIP_TRY(hipGetLastError());
  GLIA_HIP_TRY(hipEventRecord(ev.ev[1], stream));
  if (!req.forced && !req.median) inst.init_score(st, req, E0, stream);
  if (!req.forced && req.median) {
    // the median layout: per batch of records the medians / means / standard deviations of their sets (median_init.hip), then the
    // scores.  A batch's side table stays below 1 GiB; more than one batch sorts the images once per batch (GLIA_HMT_MEDIAN_BATCH:
    // records per batch, tests).
    const size_t per_rec = 3 * sizeof(double) * (size_t)(3 * cfg.n_region + 4 * cfg.n_boundary);
    uint32_t batch = (uint32_t)std::min<size_t>(E0, std::max<size_t>(1, ((size_t)1 << 30) / std::max<size_t>(per_rec, 1)));
    std::string env;
    if (option("GLIA_HMT_MEDIAN_BATCH", &env) && atoi(env.c_str()) > 0) batch = (uint32_t)std::min<long long>(E0, atoll(env.c_str()));
    double *d_reg, *d_bnd;
    if ((rc = buf.get(&d_reg, (size_t)batch * 3 * cfg.n_region * 3, false, stream)) || (rc = buf.get(&d_bnd, (size_t)batch * 4 * cfg.n_boundary * 3, false, stream))) return rc;
    const MedianInitRecords recs{st.e_u, st.e_v, st.e_table, st.shard, st.n_shards, st.le_start, st.le_dst};
    MedianInitTiming mt;
    for (uint32_t e0 = 0; e0 < E0; e0 += batch) {
      const uint32_t e1 = (uint32_t)std::min<unsigned long long>(E0, (unsigned long long)e0 + batch);
      if ((rc = median_init_stats(*req.median, recs, e0, e1, stream, d_reg, d_bnd, &mt))) return rc;
      inst.init_score_median(st, req, e0, e1, d_reg, d_bnd, stream);
    }
    if (trace) fprintf(stderr, "[trace] greedy_bc: median layout, %u records in batches of %u: sort stage %.2f ms, selection %.2f ms, %.1f MB of run buffers + %.1f MB side table\n",
                       E0, batch, mt.ms_sort, mt.ms_select, (double)mt.bytes / 1048576.0, (double)((size_t)batch * per_rec) / 1048576.0);
  }
  if (req.forced) {
    uint32_t* d_forced;
    if ((rc = buf.get(&d_forced, (size_t)2 * req.n_forced + 2, false, stream))) return rc;
    GLIA_HIP_TRY(hipMemcpyAsync(d_forced, req.forced, sizeof(uint32_t) * 2 * (size_t)req.n_forced, hipMemcpyHostToDevice, stream));
    st.forced = d_forced; st.forced_n = (unsigned long long)req.n_forced;
  }
  GLIA_HIP_TRY(hipGetLastError());
  if ((rc = pq_setup(buf, st.pq, stream))) return rc;
  unsigned long long ctrl[4] = {0, E0, 2ull * E0, ST_RUN};
  GLIA_HIP_TRY(hipMemcpyAsync(st.ctrl, ctrl, sizeof(ctrl), hipMemcpyHostToDevice, stream));
  GLIA_HIP_TRY(hipEventRecord(ev.ev[2], stream));

  if (trace) fprintf(stderr, "[trace] greedy_bc: kernels launched at %.2f ms\n", tr_ms());
  if (trace) { (void)hipStreamSynchronize(stream); fprintf(stderr, "[trace] greedy_bc: set-up + initial scores %.2f ms since the replay started; %zu of %zu device blocks (%.1f MB) were not in the block cache\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tr0).count(), buf.misses, buf.all.size(), (double)buf.miss_bytes / 1048576.0); }
  if (req.init_only) {     // features + scores of the initial table edges only (TBoundaryTable::init)
    GLIA_HIP_TRY(hipEventSynchronize(ev.ev[2]));
    out->ms_table = ev.ms(0, 1); out->ms_init = ev.ms(1, 2); out->ms_loop = 0;
    std::vector<uint8_t> tab(E0);
    if ((rc = copy_to_host_staged(tab.data(), st.e_table, E0))) return rc;
    int64_t nt = 0;
    for (uint8_t t : tab) nt += t;
    out->n_scored = nt;
    out->n = (int64_t)E0;            // init-only calls report the number of records here
    if (req.scores) {
      out->sal.resize(E0);
      if ((rc = copy_to_host_staged(out->sal.data(), st.pq.leaf_sal, sizeof(double) * E0))) return rc;
    }
    return GLIA_HMT_OK;
  }
  st.max_iters = 1ull << 14;
  while (true) {
    GLIA_HIP_TRY(hipMemsetAsync(st.hctl, 0, (size_t)kFlagReps * kFlagStride * sizeof(uint32_t), stream));
    GLIA_HIP_TRY(hipMemsetAsync(st.hjob, 0, (size_t)kJobBufs * kJobWords * sizeof(unsigned long long), stream));
    GLIA_HIP_TRY(hipMemsetAsync(st.hctl2, 0, (size_t)kFlagReps * kFlagStride * sizeof(uint32_t), stream));
    GLIA_HIP_TRY(hipMemsetAsync(st.hjob2, 0, (size_t)kJobBufs * kJob2Words * sizeof(unsigned long long), stream));
    GLIA_HIP_TRY(hipMemsetAsync(st.hvotes, 0, (size_t)kJobMax * sizeof(unsigned long long), stream));
    inst.loop(st, req, stream);
    GLIA_HIP_TRY(hipGetLastError());
    GLIA_HIP_TRY(hipMemcpyAsync(ctrl, st.ctrl, sizeof(ctrl), hipMemcpyDeviceToHost, stream));
    GLIA_HIP_TRY(hipStreamSynchronize(stream));
    if (ctrl[3] == ST_DONE) break;
    switch (ctrl[3]) {
      case ST_RUN: continue;                    // max_iters reached
      case ST_BAD_SALIENCY:
        // in this kernel: a helper workgroup did not answer within the spin limit, and the round's scores came from a stale
        // vote buffer -- the order is wrong, and a second run would hide that
        set_error("merge_order_bc: helper workgroups were lost (no answer within the spin limit), the order is not the reference's (internal error)");
        return GLIA_HMT_ERR_INTERNAL;
      case ST_NEED_POOL: {
        const unsigned long long ncap = st.pool_cap * 2;
        if ((rc = entries.grow(buf, (size_t)st.pool_cap, (size_t)ncap, stream))) return rc;
        st.pool_cap = ncap;
        break;
      }
      case ST_NEED_EDGES: {
        if (st.Ecap >= kMaxEdgeSlots) { set_error("greedy: more than 2^32 edge slots needed"); return GLIA_HMT_ERR_ARG; }
        const uint32_t ocap = st.Ecap, ncap = (uint32_t)std::min<unsigned long long>(kMaxEdgeSlots, (unsigned long long)ocap * 2ull);
        if ((rc = edges.grow(buf, ocap, ncap, stream))) return rc;
        st.Ecap = ncap; st.pq.nleaves = ncap;
        hipLaunchKernelGGL(bc_init_dead, dim3((ncap - ocap + 255) / 256), dim3(256), 0, stream, st, ocap);
        if ((rc = pq_setup(buf, st.pq, stream))) return rc;
        break;
      }
      default:
        set_error("greedy_bc: the loop kernel stopped with status " + std::to_string(ctrl[3]) + ", which its driver does not handle (internal error)");
        return GLIA_HMT_ERR_INTERNAL;
    }
    unsigned long long zero = ST_RUN;
    GLIA_HIP_TRY(hipMemcpyAsync(st.ctrl + 3, &zero, sizeof(zero), hipMemcpyHostToDevice, stream));
  }
  GLIA_HIP_TRY(hipEventRecord(ev.ev[3], stream));
  GLIA_HIP_TRY(hipEventSynchronize(ev.ev[3]));
  out->ms_table = ev.ms(0, 1); out->ms_init = ev.ms(1, 2); out->ms_loop = ev.ms(2, 3);
  out->n_scored = (int64_t)ctrl[1];
  return copy_merges(out, (int64_t)ctrl[0], st.order, st.sal_out, req.rows ? st.feats_out : nullptr, (size_t)cfg.fdim);
}

}  // namespace glia
