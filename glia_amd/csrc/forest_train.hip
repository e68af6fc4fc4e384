// glia_amd/csrc/forest_train.hip -- train_rf's forest (ml/rf/main_train_rf.cxx) grown on the device, level by level.
//
// The growing rule is this project's own definition (tests/_rfdef.py restates it in NumPy and the tests hold every array
// of a model to it bit for bit).  Everything random is a hash of (seed, tree, purpose, index); every number a split is chosen by is
// computed from INTEGER class counts and the fixed class weights, so no result depends on the order rows were counted in, on the
// arrival order of an atomic or on how many trees are in flight.
//
// State of a batch of T trees laid side by side (tree-major, so the nodes of a level are ordered by (tree, node number)):
//   rows / rcm / p2n [M]   the in-bag rows (each distinct row once), grouped by node: row index | multiplicity << 3 | class | node
//   NodeRec [nodes of the level]   tree, node number, first row, rows, class counts
// One level = plain launches, no workgroup waits for another:
//   k_prepare    16 lanes per node: terminal?  else the mtry variables with the smallest (hash, variable), and one segment per variable
//   k_gather     one thread per (row, variable): the order-preserving 64-bit image of the value and the row's position -> its segment
//   rocPRIM      segmented radix sort of (image, position) pairs -- all segments of all nodes of all trees in one call
//   k_eval_small one THREAD per segment of up to 16 rows (most segments of the deep levels hold a handful of rows: 64 per wave)
//   k_eval_wave  one WAVE per longer segment: per-class inclusive scans of the counts in 64-row steps, crit at every boundary between
//                distinct values, arg-max under the tie rule (lowest x_a)
//   k_winner     one thread per node: the best of its mtry segments (ties: lowest variable), the split value, the scan input
//   rocPRIM      exclusive scan of (splits, rows) over the level's nodes -> daughters' numbers (level order) and their first rows
//   k_assign     daughters' records
//   k_partition  one thread per row: the winning segment IS the node's rows in split order, so the stable partition is a copy in that
//                order; the daughters' class counts are integer atomic adds (summed per wave first where a wave is inside one daughter)
// and one 8-byte read-back: nodes and rows of the next level.
// When the call asks for the out-of-bag error or the importances, the passes of forest_oob.hip run on every batch after
// its last level, on the rows, the bootstrap counts and the trees this file still holds on the device; they change nothing here.
#include <chrono>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "forest_train.hpp"
#include "greedy_common.hpp"

namespace glia {

namespace {

constexpr int kSmallSeg = 16;    // segments up to this many rows: one thread each
constexpr int kGroup = 16;       // lanes per node in k_prepare
constexpr int kC = kTrainMaxClasses;

struct NodeRec {
  int tree, id;                  // tree within the batch, node number within the tree
  uint32_t start, len;           // its rows in the level's arrays
  uint32_t first;                // level index of the first node of this tree on this level
  int cnt[kC];                   // sum of multiplicities per class
};

struct TrainDev {
  const double* X; const uint8_t* ycls;
  long long N; int D, nclass, mtry, nodesize, max_depth, tree0, T;
  uint32_t sampsize, cap;        // cap: node slots per tree in the o_* arrays
  uint64_t s0;                   // mix(seed)
  double w[kC];
  uint32_t *cnt, *pos;           // [T * N + 1] bootstrap multiplicities, exclusive scan of "in bag"
  int* ndbig;                    // [T]
  int *o_left, *o_var, *o_class; double* o_split;   // [T][cap]: left daughter (1-based; right = left + 1), variable (1-based), class (1-based)
  int* vars; uint32_t *seg_begin, *seg_end; double* seg_crit; int* seg_idx;   // per (node, tried variable)
  uint8_t* term; uint32_t* wbeg; int* wcut;          // per node: terminal | begin of the winning segment | cut position in it (-1: no split)
  unsigned long long *sc_in, *sc_out;                // per node (+1): splits << 32 | rows, and its exclusive scan
};

__device__ __forceinline__ uint64_t key_of(double x) {   // order-preserving image; -0.0 and +0.0 share one
  uint64_t u = (uint64_t)__double_as_longlong(x);
  if ((u << 1) == 0) u = 0;
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double value_of(uint64_t k) {
  const uint64_t u = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
  return __longlong_as_double((long long)u);
}

// crit of a cut: the operations and their order are part of the definition
__device__ __forceinline__ double rf_crit(const TrainDev& d, const int* nL, const int* tot) {
  double numL = 0.0, denL = 0.0, numR = 0.0, denR = 0.0;
#pragma unroll
  for (int k = 0; k < kC; ++k)
    if (k < d.nclass) {
      const double tL = d.w[k] * (double)nL[k];
      numL += tL * tL; denL += tL;
      const double tR = d.w[k] * (double)(tot[k] - nL[k]);
      numR += tR * tR; denR += tR;
    }
  return numL / denL + numR / denR;
}

__device__ __forceinline__ void write_terminal(const TrainDev& d, const NodeRec& r) {
  int best = 0;
  double bw = d.w[0] * (double)r.cnt[0];
  for (int k = 1; k < d.nclass; ++k) {
    const double v = d.w[k] * (double)r.cnt[k];
    if (v > bw) { bw = v; best = k; }
  }
  const size_t slot = (size_t)r.tree * d.cap + (size_t)r.id;
  d.o_left[slot] = 0; d.o_var[slot] = 0; d.o_split[slot] = 0.0; d.o_class[slot] = best + 1;
}

__global__ void __launch_bounds__(256) k_bootstrap_count(TrainDev d) {
  const unsigned long long i = blockIdx.x * 256ull + threadIdx.x;
  if (i >= (unsigned long long)d.T * d.sampsize) return;
  const uint32_t t = (uint32_t)(i / d.sampsize), j = (uint32_t)(i % d.sampsize);
  const uint64_t h = rf_mix(rf_mix(rf_mix(d.s0 ^ (uint64_t)(d.tree0 + (int)t)) ^ 0ull) ^ (uint64_t)j);
  atomicAdd(&d.cnt[(size_t)t * d.N + (size_t)(h % (uint64_t)d.N)], 1u);
}

struct InBag {
  const uint32_t* cnt;
  __host__ __device__ uint32_t operator()(size_t i) const { return cnt[i] != 0u; }
};

// grid (blocks over the rows, T): the in-bag rows of tree blockIdx.y in ascending order, and the root's record
__global__ void __launch_bounds__(256) k_bootstrap_fill(TrainDev d, NodeRec* node, uint32_t* rows, uint32_t* rcm, uint32_t* p2n) {
  __shared__ int sc[kC];
  if (threadIdx.x < kC) sc[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t t = blockIdx.y;
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  const size_t base = (size_t)t * d.N;
  if (i < d.N) {
    const uint32_t c = d.cnt[base + i];
    if (c) {
      const uint32_t p = d.pos[base + i], cls = d.ycls[i];
      rows[p] = (uint32_t)i; rcm[p] = (c << 3) | cls; p2n[p] = t;
      atomicAdd(&sc[cls], (int)c);
    }
  }
  __syncthreads();
  if (threadIdx.x < kC && sc[threadIdx.x]) atomicAdd(&node[t].cnt[threadIdx.x], sc[threadIdx.x]);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    node[t].tree = (int)t; node[t].id = 0; node[t].first = t;
    node[t].start = d.pos[base]; node[t].len = d.pos[base + d.N] - d.pos[base];
  }
}

__global__ void __launch_bounds__(256) k_prepare(TrainDev d, const NodeRec* node, uint32_t nn, int depth) {
  const unsigned long long j = (blockIdx.x * 256ull + threadIdx.x) / kGroup;
  const int g = threadIdx.x & (kGroup - 1);
  const bool live = j < nn;
  NodeRec r;
  r.tree = 0; r.id = 0; r.start = 0; r.len = 0;
  bool term = true;
  if (live) {
    r = node[j];
    int nz = 0;
    for (int k = 0; k < d.nclass; ++k) nz += r.cnt[k] > 0;
    term = r.len <= (uint32_t)d.nodesize || nz <= 1 || (d.max_depth > 0 && depth >= d.max_depth);
    if (g == 0) {
      d.term[j] = term;
      if (term) write_terminal(d, r);
    }
  }
  const bool pick = live && !term;
  const uint64_t s1 = rf_mix(rf_mix(d.s0 ^ (uint64_t)(d.tree0 + r.tree)) ^ (uint64_t)(1 + r.id));
  const int Dn = pick ? d.D : 0;           // (every lane of the wave takes part in the shuffles below)
  uint64_t ph = 0;
  int pv = -1;
  for (int q = 0; q < d.mtry; ++q) {
    uint64_t bh = ~0ull;
    int bv = 0x7FFFFFFF;
    if (d.mtry == d.D) bv = q;            // every variable is tried: the order among them decides nothing
    else {
      for (int v = g; v < Dn; v += kGroup) {
        const uint64_t h = rf_mix(s1 ^ (uint64_t)v);
        const bool after = pv < 0 || h > ph || (h == ph && v > pv);
        if (after && (h < bh || (h == bh && v < bv))) { bh = h; bv = v; }
      }
      for (int o = kGroup / 2; o; o >>= 1) {
        const uint64_t oh = __shfl_xor(bh, o);
        const int ov = __shfl_xor(bv, o);
        if (oh < bh || (oh == bh && ov < bv)) { bh = oh; bv = ov; }
      }
      ph = bh; pv = bv;
    }
    if (live && g == 0) {
      const size_t s = (size_t)j * d.mtry + q;
      if (term) { d.seg_begin[s] = 0; d.seg_end[s] = 0; d.vars[s] = 0; }
      else {
        const uint32_t b = r.start * (uint32_t)d.mtry + (uint32_t)q * r.len;
        d.vars[s] = bv; d.seg_begin[s] = b; d.seg_end[s] = b + r.len;
      }
    }
  }
}

__global__ void __launch_bounds__(256) k_gather(TrainDev d, const NodeRec* node, const uint32_t* rows, const uint32_t* p2n, uint32_t mrows,
                                                unsigned long long* keys, uint32_t* vals) {
  const unsigned long long idx = blockIdx.x * 256ull + threadIdx.x;
  if (idx >= (unsigned long long)mrows * d.mtry) return;
  const uint32_t p = (uint32_t)(idx / d.mtry), q = (uint32_t)(idx % d.mtry);
  const uint32_t j = p2n[p];
  if (d.term[j]) return;
  const uint32_t start = node[j].start, len = node[j].len;
  const int v = d.vars[(size_t)j * d.mtry + q];
  const size_t dst = (size_t)start * d.mtry + (size_t)q * len + (p - start);
  keys[dst] = key_of(d.X[(size_t)rows[p] * d.D + v]);
  vals[dst] = p;
}

__global__ void __launch_bounds__(256) k_eval_small(TrainDev d, const NodeRec* node, const unsigned long long* keys, const uint32_t* vals,
                                                    const uint32_t* rcm, uint32_t nseg) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= nseg) return;
  const uint32_t b = d.seg_begin[s], len = d.seg_end[s] - b;
  if (len == 0 || len > (uint32_t)kSmallSeg) return;
  const NodeRec* r = &node[s / (uint32_t)d.mtry];
  int tot[kC], nL[kC];
#pragma unroll
  for (int k = 0; k < kC; ++k) { tot[k] = k < d.nclass ? r->cnt[k] : 0; nL[k] = 0; }
  double best = -1.0;
  int bi = -1;
  unsigned long long key = keys[b];
  for (uint32_t i = 0; i + 1 < len; ++i) {
    const uint32_t cm = rcm[vals[b + i]];
#pragma unroll
    for (int k = 0; k < kC; ++k) nL[k] += ((int)(cm & 7u) == k) ? (int)(cm >> 3) : 0;
    const unsigned long long nk = keys[b + i + 1];
    if (nk != key) {
      const double c = rf_crit(d, nL, tot);
      if (c > best) { best = c; bi = (int)i; }
    }
    key = nk;
  }
  d.seg_crit[s] = best; d.seg_idx[s] = bi;
}

__global__ void __launch_bounds__(256) k_eval_wave(TrainDev d, const NodeRec* node, const unsigned long long* keys, const uint32_t* vals,
                                                   const uint32_t* rcm, uint32_t nseg) {
  // A wave per segment of the level, short ones included: those leave here.  Measured against a list of the long segments that
  // k_prepare compacted with one atomic add per node: the list cost 2 ms of k_prepare per forest and saved nothing here.
  const unsigned long long w = (blockIdx.x * 256ull + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (w >= nseg) return;                                     // (wave-uniform)
  const uint32_t s = (uint32_t)w;
  const uint32_t b = d.seg_begin[s], len = d.seg_end[s] - b;
  if (len <= (uint32_t)kSmallSeg) return;
  const NodeRec* r = &node[s / (uint32_t)d.mtry];
  int tot[kC], run[kC];
#pragma unroll
  for (int k = 0; k < kC; ++k) { tot[k] = k < d.nclass ? r->cnt[k] : 0; run[k] = 0; }
  double best = -1.0;
  int bi = -1;
  for (uint32_t base = 0; base + 1 < len; base += 64) {       // position i is a candidate cut between rows i and i + 1
    const uint32_t i = base + lane;
    const bool valid = i + 1 < len;
    const unsigned long long key = valid ? keys[b + i] : 0ull, nk = valid ? keys[b + i + 1] : 0ull;
    const uint32_t cm = valid ? rcm[vals[b + i]] : 0u;
    int nL[kC];
#pragma unroll
    for (int k = 0; k < kC; ++k) {
      nL[k] = 0;
      if (k < d.nclass) {                                    // (wave-uniform)
        int c = ((int)(cm & 7u) == k) ? (int)(cm >> 3) : 0;
        for (int o = 1; o < 64; o <<= 1) {
          const int t = __shfl_up(c, o);
          if (lane >= o) c += t;
        }
        nL[k] = run[k] + c;
        run[k] += __shfl(c, 63);
      }
    }
    if (valid && nk != key) {
      const double c = rf_crit(d, nL, tot);
      if (c > best) { best = c; bi = (int)i; }
    }
  }
  for (int o = 32; o; o >>= 1) {
    const double ob = __shfl_xor(best, o);
    const int oi = __shfl_xor(bi, o);
    if (ob > best || (ob == best && oi >= 0 && oi < bi)) { best = ob; bi = oi; }
  }
  if (lane == 0) { d.seg_crit[s] = best; d.seg_idx[s] = bi; }
}

__global__ void __launch_bounds__(256) k_winner(TrainDev d, const NodeRec* node, uint32_t nn, const unsigned long long* keys) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j > nn) return;
  if (j == nn) { d.sc_in[nn] = 0ull; return; }
  d.sc_in[j] = 0ull; d.wcut[j] = -1;
  if (d.term[j]) return;
  const NodeRec r = node[j];
  double best = -1.0;
  int bq = -1, bv = 0;
  for (int q = 0; q < d.mtry; ++q) {
    const size_t s = (size_t)j * d.mtry + q;
    if (d.seg_idx[s] < 0) continue;
    const double c = d.seg_crit[s];
    const int v = d.vars[s];
    if (bq < 0 || c > best || (c == best && v < bv)) { best = c; bq = q; bv = v; }
  }
  if (bq < 0) { write_terminal(d, r); return; }             // no valid cut
  const size_t s = (size_t)j * d.mtry + bq;
  const uint32_t sb = d.seg_begin[s];
  const int a = d.seg_idx[s];
  const double xa = value_of(keys[sb + a]), xb = value_of(keys[sb + a + 1]);
  double split = 0.5 * xa + 0.5 * xb;
  if (!(split < xb)) split = xa;
  const size_t slot = (size_t)r.tree * d.cap + (size_t)r.id;
  d.o_var[slot] = bv + 1; d.o_split[slot] = split; d.o_class[slot] = 0;
  d.wbeg[j] = sb; d.wcut[j] = a;
  d.sc_in[j] = (1ull << 32) | r.len;
}

__global__ void __launch_bounds__(256) k_assign(TrainDev d, const NodeRec* node, NodeRec* next, uint32_t nn) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= nn) return;
  const int a = d.wcut[j];
  if (a < 0) return;
  const NodeRec r = node[j];
  const unsigned long long e = d.sc_out[j];
  const uint32_t c = (uint32_t)(e >> 32), rs = (uint32_t)e, fb = (uint32_t)(d.sc_out[r.first] >> 32);
  const int idl = d.ndbig[r.tree] + 2 * (int)(c - fb);
  d.o_left[(size_t)r.tree * d.cap + (size_t)r.id] = idl + 1;
  NodeRec L;
  L.tree = r.tree; L.id = idl; L.start = rs; L.len = (uint32_t)a + 1u; L.first = 2u * fb;
  for (int k = 0; k < kC; ++k) L.cnt[k] = 0;
  NodeRec R = L;
  R.id = idl + 1; R.start = rs + L.len; R.len = r.len - L.len;
  next[2 * (size_t)c] = L; next[2 * (size_t)c + 1] = R;
}

// one thread per row of the level; the first nn threads also close the level's node numbering (ndbig is read by k_assign only)
__global__ void __launch_bounds__(256) k_partition(TrainDev d, const NodeRec* node, NodeRec* next, uint32_t nn, uint32_t mrows,
                                                   const uint32_t* rows, const uint32_t* rcm, const uint32_t* p2n, const uint32_t* sorted,
                                                   uint32_t* rows_n, uint32_t* rcm_n, uint32_t* p2n_n) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  const int lane = threadIdx.x & 63;
  if (p < nn) {
    const int t = node[p].tree;
    if (p + 1 == nn || node[p + 1].tree != t)
      d.ndbig[t] += 2 * (int)((uint32_t)(d.sc_out[p + 1] >> 32) - (uint32_t)(d.sc_out[node[p].first] >> 32));
  }
  bool active = false;
  uint32_t c = 0, cm = 0;
  if (p < mrows) {
    const uint32_t j = p2n[p];
    const int a = d.wcut[j];
    if (a >= 0) {
      const uint32_t i = p - node[j].start;
      const uint32_t src = sorted[d.wbeg[j] + i];
      const unsigned long long e = d.sc_out[j];
      const uint32_t np = (uint32_t)e + i;
      c = 2u * (uint32_t)(e >> 32) + (i > (uint32_t)a ? 1u : 0u);
      cm = rcm[src];
      rows_n[np] = rows[src]; rcm_n[np] = cm; p2n_n[np] = c;
      active = true;
    }
  }
  // daughters' class counts: integers, so the order of the adds decides nothing
  const unsigned long long act = __ballot(active);
  if (act == 0ull) return;                                   // (wave-uniform)
  const uint32_t c0 = __shfl(c, __ffsll((long long)act) - 1);
  if (__all(!active || c == c0)) {
    for (int k = 0; k < d.nclass; ++k) {
      int v = (active && (int)(cm & 7u) == k) ? (int)(cm >> 3) : 0;
      for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
      if (lane == 0 && v) atomicAdd(&next[c0].cnt[k], v);
    }
  } else if (active) atomicAdd(&next[c].cnt[cm & 7u], (int)(cm >> 3));
}

}  // namespace

int forest_train_device(const double* h_x, int64_t N, int D, const TrainPlan& plan, const TrainOptions& opts, hipStream_t stream, ForestModel* out,
                        glia_hmt_forest_train_timing* tm, const OobOptions* oob, glia_hmt_forest_oob_timing* otm) {
  const auto wall0 = std::chrono::steady_clock::now();
  const bool trace = option("GLIA_HMT_TRACE");
  memset(tm, 0, sizeof(*tm));
  if (otm) memset(otm, 0, sizeof(*otm));
  const OobOptions oo = oob ? *oob : OobOptions();
  const bool with_oob = oo.oob || oo.importance;
  const int mtry = plan.mtry, nclass = plan.nclass, ntree = opts.ntree;
  const uint64_t per_tree = (uint64_t)std::min<int64_t>(plan.sampsize, N);      // distinct in-bag rows of a tree, at most
  const uint64_t cap = 2 * per_tree - 1;                                         // nodes of a tree, at most
  // ---- the plan: trees in flight and the device memory they take, before anything is allocated ----
  auto bytes_for = [&](uint64_t T) -> uint64_t {
    const uint64_t Mb = T * per_tree, S = Mb * (uint64_t)mtry;
    uint64_t b = (uint64_t)N * D * 8 + (uint64_t)N;                              // X, classes
    b += (T * (uint64_t)N + 1) * 8;                                              // cnt, pos
    b += Mb * (3 * 4 * 2 + sizeof(NodeRec) * 2 + 1 + 4 + 4 + 16) + 64;           // rows / rcm / p2n x 2, records x 2, term, wbeg, wcut, scans
    b += S * (4 + 4 + 4 + 8 + 4 + 2 * 8 + 2 * 4);                                // vars, segments, results, keys x 2, positions x 2
    b += S * 8;                                                                  // rocPRIM's scratch (bounded below once it is known)
    b += T * (cap * 20 + 4);                                                     // the trees
    b += OobPass::bytes(oo, (uint64_t)N, (uint64_t)D, (uint64_t)nclass, T, cap, (uint64_t)ntree);   // the out-of-bag passes (forest_oob.hip)
    return b;
  };
  size_t free_b = 0, total_b = 0;
  GLIA_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  const uint64_t budget = (uint64_t)(0.85 * (double)free_b);
  uint64_t T = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)ntree, (1ull << 27) / std::max<uint64_t>(1, per_tree * mtry)));
  T = std::min<uint64_t>(T, 65535);                                              // (k_bootstrap_fill: one grid row per tree)
  std::string opt_t;
  if (option("GLIA_HMT_TRAIN_TREES", &opt_t) && atoi(opt_t.c_str()) > 0) T = std::min<uint64_t>(std::min<uint64_t>((uint64_t)ntree, 65535), (uint64_t)atoi(opt_t.c_str()));
  while (T > 1 && (bytes_for(T) > budget || T * per_tree * mtry >= (1ull << 31))) T = (T + 1) / 2;
  if (bytes_for(T) > budget || per_tree * (uint64_t)mtry >= (1ull << 31) || cap >= (1ull << 31)) {
    char b[256];
    snprintf(b, sizeof(b), "forest_train: one tree of %lld rows x %d tried variables needs %.1f MiB of device memory (rows included), %.1f MiB are free",
             (long long)N, mtry, (double)bytes_for(1) / 1048576.0, (double)free_b / 1048576.0);
    set_error(b);
    return GLIA_HMT_ERR_UNSUPPORTED;
  }
  const uint64_t Mb = T * per_tree, S = Mb * (uint64_t)mtry;
  tm->trees_in_flight = (int64_t)T;
  tm->device_bytes = bytes_for(T);

  CallEvents<8> ev;
  int rc;
  if ((rc = ev.create())) return rc;
  DeviceBuffers buf;
  TrainDev d;
  memset(&d, 0, sizeof(d));
  double* dX; uint8_t* dY;
  uint32_t *rows[2], *rcm[2], *p2n[2], *vals[2];
  unsigned long long* keys[2];
  NodeRec* node[2];
  if ((rc = buf.get(&dX, (size_t)N * D, false, stream)) || (rc = buf.get(&dY, (size_t)N, false, stream)) ||
      (rc = buf.get(&d.cnt, T * N + 1, false, stream)) || (rc = buf.get(&d.pos, T * N + 1, false, stream)) ||
      (rc = buf.get(&d.ndbig, T, false, stream)) || (rc = buf.get(&d.o_left, T * cap, false, stream)) ||
      (rc = buf.get(&d.o_var, T * cap, false, stream)) || (rc = buf.get(&d.o_class, T * cap, false, stream)) ||
      (rc = buf.get(&d.o_split, T * cap, false, stream)) || (rc = buf.get(&d.vars, S, false, stream)) ||
      (rc = buf.get(&d.seg_begin, S, false, stream)) || (rc = buf.get(&d.seg_end, S, false, stream)) ||
      (rc = buf.get(&d.seg_crit, S, false, stream)) || (rc = buf.get(&d.seg_idx, S, false, stream)) ||
      (rc = buf.get(&d.term, Mb, false, stream)) || (rc = buf.get(&d.wbeg, Mb, false, stream)) || (rc = buf.get(&d.wcut, Mb, false, stream)) ||
      (rc = buf.get(&d.sc_in, Mb + 1, false, stream)) || (rc = buf.get(&d.sc_out, Mb + 1, false, stream)))
    return rc;
  for (int i = 0; i < 2; ++i)
    if ((rc = buf.get(&rows[i], Mb, false, stream)) || (rc = buf.get(&rcm[i], Mb, false, stream)) || (rc = buf.get(&p2n[i], Mb, false, stream)) ||
        (rc = buf.get(&node[i], Mb, false, stream)) || (rc = buf.get(&keys[i], S, false, stream)) || (rc = buf.get(&vals[i], S, false, stream)))
      return rc;
  // rocPRIM's scratch, sized for the largest call of each kind; a call that asks for more gets a block of its own
  size_t sort_bytes = 0, scan_bytes = 0, scan2_bytes = 0;
  GLIA_HIP_TRY(rocprim::segmented_radix_sort_pairs(nullptr, sort_bytes, keys[0], keys[1], vals[0], vals[1], (unsigned)S, (unsigned)S, d.seg_begin, d.seg_end, 0, 64, stream));
  GLIA_HIP_TRY(rocprim::exclusive_scan(nullptr, scan_bytes, d.sc_in, d.sc_out, 0ull, (size_t)Mb + 1, rocprim::plus<unsigned long long>(), stream));
  const auto inbag = rocprim::make_transform_iterator(rocprim::counting_iterator<size_t>(0), InBag{d.cnt});
  GLIA_HIP_TRY(rocprim::exclusive_scan(nullptr, scan2_bytes, inbag, d.pos, 0u, (size_t)(T * N + 1), rocprim::plus<uint32_t>(), stream));
  size_t tmp_bytes = std::max(std::max(sort_bytes, scan_bytes), std::max(scan2_bytes, (size_t)256));
  char* tmp;
  if ((rc = buf.get(&tmp, tmp_bytes, false, stream))) return rc;
  auto scratch = [&](size_t need, char** p) -> int {
    if (need <= tmp_bytes) { *p = tmp; return GLIA_HMT_OK; }
    return buf.get(p, need, false, stream);
  };

  d.X = dX; d.ycls = dY; d.N = N; d.D = D; d.nclass = nclass; d.mtry = mtry; d.nodesize = opts.nodesize; d.max_depth = opts.max_depth;
  d.sampsize = (uint32_t)plan.sampsize; d.cap = (uint32_t)cap; d.s0 = rf_mix(opts.seed);
  for (int k = 0; k < kC; ++k) d.w[k] = k < nclass ? plan.classwt[k] : 0.0;

  GLIA_HIP_TRY(hipEventRecord(ev.ev[0], stream));
  GLIA_HIP_TRY(hipMemcpyAsync(dX, h_x, sizeof(double) * (size_t)N * D, hipMemcpyHostToDevice, stream));     // once per call
  GLIA_HIP_TRY(hipMemcpyAsync(dY, plan.cls.data(), (size_t)N, hipMemcpyHostToDevice, stream));
  GLIA_HIP_TRY(hipEventRecord(ev.ev[1], stream));
  GLIA_HIP_TRY(hipStreamSynchronize(stream));
  tm->ms_upload = ev.ms(0, 1);

  std::vector<std::vector<int>> t_left((size_t)ntree), t_var((size_t)ntree), t_class((size_t)ntree);
  std::vector<std::vector<double>> t_split((size_t)ntree);
  std::vector<int> ndbig((size_t)ntree, 0);
  OobPass oob_pass;
  if (with_oob && (rc = oob_pass.init(oo, N, D, plan, opts, T, cap, stream, otm))) return rc;
  auto blocks = [](unsigned long long n) { return (unsigned)((n + 255) / 256); };

  for (int tree0 = 0; tree0 < ntree; tree0 += (int)T) {
    const int Tb = std::min<int>((int)T, ntree - tree0);
    d.tree0 = tree0; d.T = Tb;
    ++tm->batches;
    // ---- bootstrap ----
    GLIA_HIP_TRY(hipEventRecord(ev.ev[0], stream));
    const size_t TN = (size_t)Tb * (size_t)N;
    GLIA_HIP_TRY(hipMemsetAsync(d.cnt, 0, sizeof(uint32_t) * (TN + 1), stream));
    GLIA_HIP_TRY(hipMemsetAsync(node[0], 0, sizeof(NodeRec) * (size_t)Tb, stream));
    k_bootstrap_count<<<blocks((unsigned long long)Tb * plan.sampsize), 256, 0, stream>>>(d);
    {
      size_t need = 0;
      GLIA_HIP_TRY(rocprim::exclusive_scan(nullptr, need, inbag, d.pos, 0u, TN + 1, rocprim::plus<uint32_t>(), stream));
      char* t;
      if ((rc = scratch(need, &t))) return rc;
      GLIA_HIP_TRY(rocprim::exclusive_scan((void*)t, need, inbag, d.pos, 0u, TN + 1, rocprim::plus<uint32_t>(), stream));
    }
    k_bootstrap_fill<<<dim3(blocks((unsigned long long)N), (unsigned)Tb), 256, 0, stream>>>(d, node[0], rows[0], rcm[0], p2n[0]);
    std::vector<int> ones((size_t)Tb, 1);
    GLIA_HIP_TRY(hipMemcpyAsync(d.ndbig, ones.data(), sizeof(int) * (size_t)Tb, hipMemcpyHostToDevice, stream));
    uint32_t mrows = 0;
    GLIA_HIP_TRY(hipMemcpyAsync(&mrows, d.pos + TN, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    GLIA_HIP_TRY(hipEventRecord(ev.ev[1], stream));
    GLIA_HIP_TRY(hipStreamSynchronize(stream));
    GLIA_HIP_TRY(hipGetLastError());
    tm->ms_bootstrap += ev.ms(0, 1);
    tm->launches += 3;
    if ((uint64_t)mrows > Mb) { set_error("forest_train: more in-bag rows than planned"); return GLIA_HMT_ERR_INTERNAL; }

    // ---- the levels ----
    uint32_t nn = (uint32_t)Tb;
    int cur = 0;
    for (int depth = 0; nn > 0; ++depth) {
      const int nxt = cur ^ 1;
      const uint32_t nseg = nn * (uint32_t)mtry;
      const unsigned long long nel = (unsigned long long)mrows * mtry;
      GLIA_HIP_TRY(hipEventRecord(ev.ev[0], stream));
      k_prepare<<<blocks((unsigned long long)nn * kGroup), 256, 0, stream>>>(d, node[cur], nn, depth);
      GLIA_HIP_TRY(hipEventRecord(ev.ev[1], stream));
      k_gather<<<blocks(nel), 256, 0, stream>>>(d, node[cur], rows[cur], p2n[cur], mrows, keys[0], vals[0]);
      GLIA_HIP_TRY(hipEventRecord(ev.ev[2], stream));
      {
        size_t need = 0;
        GLIA_HIP_TRY(rocprim::segmented_radix_sort_pairs(nullptr, need, keys[0], keys[1], vals[0], vals[1], (unsigned)nel, nseg, d.seg_begin, d.seg_end, 0, 64, stream));
        char* t;
        if ((rc = scratch(need, &t))) return rc;
        GLIA_HIP_TRY(rocprim::segmented_radix_sort_pairs((void*)t, need, keys[0], keys[1], vals[0], vals[1], (unsigned)nel, nseg, d.seg_begin, d.seg_end, 0, 64, stream));
      }
      GLIA_HIP_TRY(hipEventRecord(ev.ev[3], stream));
      k_eval_small<<<blocks(nseg), 256, 0, stream>>>(d, node[cur], keys[1], vals[1], rcm[cur], nseg);
      k_eval_wave<<<blocks((unsigned long long)nseg * 64), 256, 0, stream>>>(d, node[cur], keys[1], vals[1], rcm[cur], nseg);
      GLIA_HIP_TRY(hipEventRecord(ev.ev[4], stream));
      k_winner<<<blocks((unsigned long long)nn + 1), 256, 0, stream>>>(d, node[cur], nn, keys[1]);
      {
        size_t need = 0;
        GLIA_HIP_TRY(rocprim::exclusive_scan(nullptr, need, d.sc_in, d.sc_out, 0ull, (size_t)nn + 1, rocprim::plus<unsigned long long>(), stream));
        char* t;
        if ((rc = scratch(need, &t))) return rc;
        GLIA_HIP_TRY(rocprim::exclusive_scan((void*)t, need, d.sc_in, d.sc_out, 0ull, (size_t)nn + 1, rocprim::plus<unsigned long long>(), stream));
      }
      k_assign<<<blocks(nn), 256, 0, stream>>>(d, node[cur], node[nxt], nn);
      GLIA_HIP_TRY(hipEventRecord(ev.ev[5], stream));
      k_partition<<<blocks(mrows), 256, 0, stream>>>(d, node[cur], node[nxt], nn, mrows, rows[cur], rcm[cur], p2n[cur], vals[1], rows[nxt], rcm[nxt], p2n[nxt]);
      GLIA_HIP_TRY(hipEventRecord(ev.ev[6], stream));
      unsigned long long lc = 0;                              // splits << 32 | rows of the next level
      GLIA_HIP_TRY(hipMemcpyAsync(&lc, d.sc_out + nn, sizeof(lc), hipMemcpyDeviceToHost, stream));
      GLIA_HIP_TRY(hipStreamSynchronize(stream));
      GLIA_HIP_TRY(hipGetLastError());
      tm->ms_prepare += ev.ms(0, 1); tm->ms_gather += ev.ms(1, 2); tm->ms_sort += ev.ms(2, 3); tm->ms_scan += ev.ms(3, 4);
      tm->ms_split += ev.ms(4, 5); tm->ms_partition += ev.ms(5, 6);
      tm->launches += 9; ++tm->levels;
      const uint32_t splits = (uint32_t)(lc >> 32), next_rows = (uint32_t)lc;
      if (2ull * splits > Mb || next_rows > mrows) { set_error("forest_train: a level grew beyond its plan"); return GLIA_HMT_ERR_INTERNAL; }
      tm->nodes += nn;
      nn = 2u * splits; mrows = next_rows; cur = nxt;
    }
    // ---- the trees of the batch ----
    GLIA_HIP_TRY(hipEventRecord(ev.ev[0], stream));
    GLIA_HIP_TRY(hipMemcpy(&ndbig[tree0], d.ndbig, sizeof(int) * (size_t)Tb, hipMemcpyDeviceToHost));
    for (int t = 0; t < Tb; ++t) {
      const size_t n = (size_t)ndbig[tree0 + t], off = (size_t)t * cap;
      if (n < 1 || n > cap) { set_error("forest_train: a tree outgrew its plan"); return GLIA_HMT_ERR_INTERNAL; }
      t_left[tree0 + t].resize(n); t_var[tree0 + t].resize(n); t_class[tree0 + t].resize(n); t_split[tree0 + t].resize(n);
      GLIA_HIP_TRY(hipMemcpyAsync(t_left[tree0 + t].data(), d.o_left + off, sizeof(int) * n, hipMemcpyDeviceToHost, stream));
      GLIA_HIP_TRY(hipMemcpyAsync(t_var[tree0 + t].data(), d.o_var + off, sizeof(int) * n, hipMemcpyDeviceToHost, stream));
      GLIA_HIP_TRY(hipMemcpyAsync(t_class[tree0 + t].data(), d.o_class + off, sizeof(int) * n, hipMemcpyDeviceToHost, stream));
      GLIA_HIP_TRY(hipMemcpyAsync(t_split[tree0 + t].data(), d.o_split + off, sizeof(double) * n, hipMemcpyDeviceToHost, stream));
    }
    GLIA_HIP_TRY(hipEventRecord(ev.ev[1], stream));
    GLIA_HIP_TRY(hipStreamSynchronize(stream));
    tm->ms_download += ev.ms(0, 1);
    if (with_oob) {
      OobBatch ob;
      ob.X = dX; ob.ycls = dY; ob.cnt = d.cnt; ob.pos = d.pos; ob.o_left = d.o_left; ob.o_var = d.o_var; ob.o_class = d.o_class; ob.ndbig = d.ndbig;
      ob.o_split = d.o_split; ob.tree0 = tree0; ob.T = Tb;
      if ((rc = oob_pass.run(ob, &t_left[tree0], &t_var[tree0]))) return rc;
    }
    if (trace)
      fprintf(stderr, "[trace] forest_train: trees %d..%d of %d done, %lld levels so far; ms: bootstrap %.2f prepare %.2f gather %.2f sort %.2f scan %.2f split %.2f partition %.2f download %.2f\n",
              tree0, tree0 + Tb - 1, ntree, (long long)tm->levels, tm->ms_bootstrap, tm->ms_prepare, tm->ms_gather, tm->ms_sort, tm->ms_scan, tm->ms_split,
              tm->ms_partition, tm->ms_download);
  }

  // ---- the model ----
  ForestModel& m = *out;
  m = ForestModel();
  m.ntree = ntree; m.nclass = nclass; m.mtry = mtry;
  m.nrnodes = *std::max_element(ndbig.begin(), ndbig.end());
  const size_t nr = (size_t)m.nrnodes, nn_all = nr * (size_t)ntree;
  m.xbestsplit.assign(nn_all, 0.0); m.treemap.assign(2 * nn_all, 0); m.nodestatus.assign(nn_all, 0); m.nodeclass.assign(nn_all, 0);
  m.bestvar.assign(nn_all, 0); m.ndbigtree = ndbig;
  for (int t = 0; t < ntree; ++t)
    for (size_t k = 0; k < (size_t)ndbig[t]; ++k) {
      const size_t i = (size_t)t * nr + k;
      const int left = t_left[t][k];
      m.xbestsplit[i] = t_split[t][k]; m.bestvar[i] = t_var[t][k]; m.nodeclass[i] = t_class[t][k];
      m.nodestatus[i] = left ? 1 : -1;
      m.treemap[2 * i] = left; m.treemap[2 * i + 1] = left ? left + 1 : 0;
    }
  m.classwt = plan.classwt;
  m.cutoff.assign(nclass, 1.0 / nclass);
  m.orig_labels = plan.orig_labels;
  m.new_labels.resize(nclass);
  for (int k = 0; k < nclass; ++k) m.new_labels[k] = k + 1;
  if (with_oob && (rc = oob_pass.finish(&m))) return rc;
  tm->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
  if (trace)
    fprintf(stderr, "[trace] forest_train: %d trees (%lld in flight, %lld batches), %lld levels, %lld launches, %.1f MiB planned, %.2f ms in all (upload %.2f)\n", ntree,
            (long long)tm->trees_in_flight, (long long)tm->batches, (long long)tm->levels, (long long)tm->launches, (double)tm->device_bytes / 1048576.0, tm->ms_total, tm->ms_upload);
  return GLIA_HMT_OK;
}

}  // namespace glia
