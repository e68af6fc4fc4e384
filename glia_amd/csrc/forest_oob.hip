// glia_amd/csrc/forest_oob.hip -- what a training call learns from the rows its trees did not see: classRF's errtr,
// outcl, counttr, votes, oob_times, importance and importanceSD (ml/rf/ml_rf_train.cxx:112-159), by this project's own deterministic
// definition (tests/_rfoobdef.py restates it; the tests hold every array to it bit for bit).
//
// The device counts, the host divides (forest_oob.hpp).  Per batch of trees in flight, after the trainer's last level:
//   k_oob_pack    one thread per node: the trainer's four node arrays -> one 16-byte record that carries the CLASS at a terminal node
//                 (the predictor's PackedNode carries a vote for one label); a record that would lead a walk astray stops the call
//   k_oob_walk    one thread per (tree, row): the walk of DESIGN 3.8.  A row outside the bag leaves its class in a [T][N] byte matrix
//                 and its index in the tree's ascending list of out-of-bag rows; a row inside adds its multiplicity to the class counts
//                 of its terminal node (the Gini decreases are computed from these on the host)
//   k_oob_tally   one thread per row, its vote counts in registers: steps through the batch's trees in order and adds the row's
//                 "seen", "wrong" and "out of bag" flags to per-tree, per-class integers -- summed per wave with ballots, per workgroup
//                 in LDS, then one integer atomic per counter.  The counts carry across batches in counttr
//   k_oob_imp     one thread per (tree, out-of-bag rank): walks the row once more and, at the FIRST node of its path that tests a
//                 variable v, walks on from there with x[v] replaced by column v of the row at rank pi(j).  A variable the path never
//                 tests cannot change the row's class, so those walks are not made.  Changed predictions are counted as integers per
//                 (tree, variable, class): in LDS where the table fits, with global integer atomics where it does not
// Integer adds only, so no result depends on the order of arrival or on how many trees are in flight; no workgroup waits for another.
#include <chrono>

#include "forest_train.hpp"
#include "greedy_common.hpp"

namespace glia {

namespace {

constexpr int kC = kTrainMaxClasses;
constexpr int kInBag = 0xFF;          // oobcls of a row inside the bag
constexpr int kTallyTrees = 64;       // trees per LDS round of k_oob_tally
constexpr int kImpLds = 1024;         // (variable, class) counters a workgroup of k_oob_imp keeps in LDS

struct OobNode {
  double split;
  int var;                            // >= 0: tests this column, daughters left and left + 1; < 0: terminal of class -1 - var
  int left;
};

struct OobDev {
  OobBatch b;
  long long N;
  int D, nclass, want_imp;
  uint32_t cap;
  uint64_t s0;                        // mix(seed)
  OobNode* nodes;                     // [T][cap]
  uint8_t* oobcls;                    // [T][N]
  uint32_t* ooblist;                  // [T][N]: the out-of-bag rows of a tree, ascending (its first m_t entries)
  int* leafcnt;                       // [T][cap][nclass]: in-bag class counts of the terminal nodes
  int* counttr;                       // [nclass][N], across batches
  unsigned* errcnt;                   // [ntree][kC][3], across batches: wrong, seen, out-of-bag rows of the class
  int* dcnt;                          // [T][D][nclass]: r_k - r'_k
  unsigned long long* walks;          // permuted walks made
  int* bad;                           // a node record that no tree of the trainer can hold
};

__global__ void __launch_bounds__(256) k_oob_pack(OobDev d) {
  const uint32_t t = blockIdx.y, q = blockIdx.x * 256u + threadIdx.x;
  const int n = d.b.ndbig[t];
  if (q >= d.cap || (int)q >= n) return;
  const size_t slot = (size_t)t * d.cap + q;
  const int left = d.b.o_left[slot], var = d.b.o_var[slot], cls = d.b.o_class[slot];
  OobNode r;
  r.split = d.b.o_split[slot];
  if (left) {
    r.var = var - 1; r.left = left - 1;
    if (r.left <= (int)q || r.left + 1 >= n || r.var < 0 || r.var >= d.D) { *d.bad = 1; r.var = -1; r.left = 0; }   // (daughters come after their mother)
  } else {
    r.var = -cls; r.left = 0;
    if (cls < 1 || cls > d.nclass) { *d.bad = 1; r.var = -1; }
  }
  d.nodes[slot] = r;
}

// the terminal node row x reaches from node q: left iff x[var] <= split
__device__ __forceinline__ int oob_descend(const OobNode* tree, const double* x, int q) {
  OobNode e = tree[q];
  while (e.var >= 0) {
    q = e.left + (x[e.var] <= e.split ? 0 : 1);
    e = tree[q];
  }
  return q;
}

__global__ void __launch_bounds__(256) k_oob_walk(OobDev d) {
  const uint32_t t = blockIdx.y;
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= d.N) return;
  const size_t base = (size_t)t * d.N;
  const OobNode* tree = d.nodes + (size_t)t * d.cap;
  const uint32_t c = d.b.cnt[base + i];
  if (c && !d.want_imp) { d.oobcls[base + i] = (uint8_t)kInBag; return; }
  const int q = oob_descend(tree, d.b.X + (size_t)i * d.D, 0);
  if (c) {
    d.oobcls[base + i] = (uint8_t)kInBag;
    if (d.want_imp) atomicAdd(&d.leafcnt[((size_t)t * d.cap + q) * d.nclass + d.b.ycls[i]], (int)c);
  } else {
    d.oobcls[base + i] = (uint8_t)(-1 - tree[q].var);
    const uint32_t rank = (uint32_t)i - (d.b.pos[base + i] - d.b.pos[base]);       // rows outside the bag in front of this one
    d.ooblist[base + rank] = (uint32_t)i;
  }
}

__global__ void __launch_bounds__(256) k_oob_tally(OobDev d) {
  __shared__ unsigned acc[kTallyTrees][kC][3];
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  const bool live = i < d.N;
  const int lane = threadIdx.x & 63;
  const int cls = live ? d.b.ycls[i] : -1;
  int cnt[kC];
#pragma unroll
  for (int k = 0; k < kC; ++k) cnt[k] = (live && k < d.nclass) ? d.counttr[(size_t)k * d.N + i] : 0;
  for (int t0 = 0; t0 < d.b.T; t0 += kTallyTrees) {
    const int nt = min(kTallyTrees, d.b.T - t0);
    for (int e = threadIdx.x; e < kTallyTrees * kC * 3; e += 256) (&acc[0][0][0])[e] = 0u;
    __syncthreads();
    for (int tt = 0; tt < nt; ++tt) {
      const int o = live ? (int)d.oobcls[(size_t)(t0 + tt) * d.N + i] : kInBag;
      const bool out = o != kInBag;
      int best = 0, bestc = 0, sum = 0;
#pragma unroll
      for (int k = 0; k < kC; ++k) {
        cnt[k] += (out && o == k) ? 1 : 0;
        sum += cnt[k];
        if (cnt[k] > bestc) { bestc = cnt[k]; best = k; }          // ties: the lowest class
      }
      const bool seen = live && sum > 0, wrong = seen && best != cls;
      for (int k = 0; k < d.nclass; ++k) {                          // (wave-uniform)
        const bool mine = cls == k;
        const unsigned long long bw = __ballot(wrong && mine), bs = __ballot(seen && mine), bo = __ballot(out && mine);
        if (lane == 0) {
          if (bw) atomicAdd(&acc[tt][k][0], (unsigned)__popcll(bw));
          if (bs) atomicAdd(&acc[tt][k][1], (unsigned)__popcll(bs));
          if (bo) atomicAdd(&acc[tt][k][2], (unsigned)__popcll(bo));
        }
      }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < nt * kC * 3; e += 256) {
      const unsigned v = (&acc[0][0][0])[e];
      if (v) atomicAdd(&d.errcnt[(size_t)(d.b.tree0 + t0) * kC * 3 + e], v);
    }
    __syncthreads();
  }
  if (live)
#pragma unroll
    for (int k = 0; k < kC; ++k)
      if (k < d.nclass) d.counttr[(size_t)k * d.N + i] = cnt[k];
}

// pi(j) of tree `tree` (its number in the forest) and variable v over [0, m): a four-round Feistel network on b bits, walked until it
// lands inside [0, m)
__device__ __forceinline__ uint32_t oob_perm(uint64_t s0, int tree, int v, uint32_t j, uint32_t m, int half) {
  const uint64_t base = rf_mix(rf_mix(s0 ^ (uint64_t)tree) ^ ((1ull << 32) + (uint64_t)v));
  const uint64_t k0 = rf_mix(base ^ 0ull), k1 = rf_mix(base ^ 1ull), k2 = rf_mix(base ^ 2ull), k3 = rf_mix(base ^ 3ull);
  const uint64_t mask = (1ull << half) - 1ull;
  uint64_t x = j;
  do {
    uint64_t L = x >> half, R = x & mask, n;
    n = L ^ (rf_mix(k0 ^ R) & mask); L = R; R = n;
    n = L ^ (rf_mix(k1 ^ R) & mask); L = R; R = n;
    n = L ^ (rf_mix(k2 ^ R) & mask); L = R; R = n;
    n = L ^ (rf_mix(k3 ^ R) & mask); L = R; R = n;
    x = (L << half) | R;
  } while (x >= (uint64_t)m);
  return (uint32_t)x;
}

// grid (tiles of 256 out-of-bag ranks, T)
__global__ void __launch_bounds__(256) k_oob_imp(OobDev d) {
  __shared__ int loc[kImpLds];
  const uint32_t t = blockIdx.y;
  const size_t base = (size_t)t * d.N;
  const uint32_t m = (uint32_t)d.N - (d.b.pos[base + d.N] - d.b.pos[base]);       // out-of-bag rows of the tree
  if (blockIdx.x * 256u >= m) return;                                             // (uniform over the workgroup)
  const int entries = d.D * d.nclass;
  const bool in_lds = entries <= kImpLds;
  if (in_lds) {
    for (int e = threadIdx.x; e < entries; e += 256) loc[e] = 0;
    __syncthreads();
  }
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  unsigned made = 0;
  if (j < m) {
    int half = 1;
    while ((1ull << (2 * half)) < (unsigned long long)m) ++half;
    const OobNode* tree = d.nodes + (size_t)t * d.cap;
    const uint32_t* list = d.ooblist + base;
    const uint32_t i = list[j];
    const double* x = d.b.X + (size_t)i * d.D;
    const int cls = d.b.ycls[i];
    const int p = -1 - tree[oob_descend(tree, x, 0)].var;
    int* tab = in_lds ? loc : d.dcnt + (size_t)t * entries;
    uint64_t seen0 = 0, seen1 = 0;                                                // variables of the path so far, by v mod 128
    int q = 0;
    OobNode e = tree[0];
    while (e.var >= 0) {
      const int v = e.var;
      const uint64_t bit = 1ull << (v & 63);
      bool first = !(((v & 64) ? seen1 : seen0) & bit);
      if (!first && d.D > 128) {                                                  // another variable may share the bit: look the path over
        first = true;
        int r = 0;
        OobNode a = tree[0];
        while (r != q) {
          if (a.var == v) { first = false; break; }
          r = a.left + (x[a.var] <= a.split ? 0 : 1);
          a = tree[r];
        }
      }
      if (v & 64) seen1 |= bit; else seen0 |= bit;
      if (first) {
        const uint32_t pj = oob_perm(d.s0, d.b.tree0 + (int)t, v, j, m, half);
        const double xv = d.b.X[(size_t)list[pj] * d.D + v];
        int r = q;
        OobNode a = e;
        while (a.var >= 0) {
          const double val = a.var == v ? xv : x[a.var];
          r = a.left + (val <= a.split ? 0 : 1);
          a = tree[r];
        }
        const int p2 = -1 - a.var;
        ++made;
        if (p2 != p) {
          if (p == cls) atomicAdd(&tab[v * d.nclass + cls], 1);
          else if (p2 == cls) atomicAdd(&tab[v * d.nclass + cls], -1);
        }
      }
      q = e.left + (x[v] <= e.split ? 0 : 1);
      e = tree[q];
    }
  }
  for (int o = 32; o; o >>= 1) made += __shfl_xor(made, o);
  if ((threadIdx.x & 63) == 0 && made) atomicAdd(d.walks, (unsigned long long)made);
  if (in_lds) {
    __syncthreads();
    for (int e = threadIdx.x; e < entries; e += 256)
      if (loc[e]) atomicAdd(&d.dcnt[(size_t)t * entries + e], loc[e]);
  }
}

}  // namespace

struct OobPass::Impl {
  OobOptions o;
  OobDev d;
  DeviceBuffers buf;
  CallEvents<4> ev;
  hipStream_t stream = nullptr;
  glia_hmt_forest_oob_timing* tm = nullptr;
  glia_hmt_forest_oob_timing own = {};
  int ntree = 0;
  uint64_t T = 0;
  std::vector<double> w;
  ImportanceSums sums;
};

OobPass::OobPass() : p_(new Impl) {}
OobPass::~OobPass() { delete p_; }

uint64_t OobPass::bytes(const OobOptions& o, uint64_t N, uint64_t D, uint64_t nclass, uint64_t T, uint64_t cap, uint64_t ntree) {
  if (!o.oob && !o.importance) return 0;
  uint64_t b = T * cap * sizeof(OobNode) + T * N * (1 + 4) + nclass * N * 4 + ntree * kC * 3 * 4 + 1024;   // nodes, classes, lists, votes, counters
  if (o.importance) b += T * cap * nclass * 4 + T * D * nclass * 4;                                       // leaf counts, changed predictions
  return b;
}

int OobPass::init(const OobOptions& o, int64_t N, int D, const TrainPlan& plan, const TrainOptions& opts, uint64_t T, uint64_t cap, hipStream_t stream,
                  glia_hmt_forest_oob_timing* timing) {
  Impl& s = *p_;
  s.o = o; s.stream = stream; s.tm = timing ? timing : &s.own; s.ntree = opts.ntree; s.T = T;
  memset(s.tm, 0, sizeof(*s.tm));
  memset(&s.d, 0, sizeof(s.d));
  OobDev& d = s.d;
  d.N = N; d.D = D; d.nclass = plan.nclass; d.want_imp = o.importance ? 1 : 0; d.cap = (uint32_t)cap; d.s0 = rf_mix(opts.seed);
  s.w = plan.classwt;
  s.tm->device_bytes = bytes(o, (uint64_t)N, (uint64_t)D, (uint64_t)plan.nclass, T, cap, (uint64_t)opts.ntree);
  int rc;
  if ((rc = s.ev.create())) return rc;
  if ((rc = s.buf.get(&d.nodes, T * cap, false, stream)) || (rc = s.buf.get(&d.oobcls, T * (uint64_t)N, false, stream)) ||
      (rc = s.buf.get(&d.ooblist, T * (uint64_t)N, false, stream)) || (rc = s.buf.get(&d.counttr, (uint64_t)plan.nclass * N, true, stream)) ||
      (rc = s.buf.get(&d.errcnt, (uint64_t)opts.ntree * kC * 3, true, stream)) || (rc = s.buf.get(&d.walks, 1, true, stream)) ||
      (rc = s.buf.get(&d.bad, 1, true, stream)))
    return rc;
  if (o.importance) {
    if ((rc = s.buf.get(&d.leafcnt, T * cap * plan.nclass, false, stream)) || (rc = s.buf.get(&d.dcnt, T * (uint64_t)D * plan.nclass, false, stream))) return rc;
    s.sums.init(D, plan.nclass);
  }
  return GLIA_HMT_OK;
}

int OobPass::run(const OobBatch& b, const std::vector<int>* h_left, const std::vector<int>* h_var) {
  Impl& s = *p_;
  OobDev& d = s.d;
  d.b = b;
  hipStream_t st = s.stream;
  const int nclass = d.nclass, D = d.D, T = b.T;
  const unsigned row_blocks = (unsigned)((d.N + 255) / 256);
  GLIA_HIP_TRY(hipEventRecord(s.ev.ev[0], st));
  if (s.o.importance) {
    GLIA_HIP_TRY(hipMemsetAsync(d.leafcnt, 0, sizeof(int) * (size_t)T * d.cap * nclass, st));
    GLIA_HIP_TRY(hipMemsetAsync(d.dcnt, 0, sizeof(int) * (size_t)T * D * nclass, st));
  }
  k_oob_pack<<<dim3((d.cap + 255u) / 256u, (unsigned)T), 256, 0, st>>>(d);
  k_oob_walk<<<dim3(row_blocks, (unsigned)T), 256, 0, st>>>(d);
  GLIA_HIP_TRY(hipEventRecord(s.ev.ev[1], st));
  k_oob_tally<<<row_blocks, 256, 0, st>>>(d);
  GLIA_HIP_TRY(hipEventRecord(s.ev.ev[2], st));
  if (s.o.importance) k_oob_imp<<<dim3(row_blocks, (unsigned)T), 256, 0, st>>>(d);
  GLIA_HIP_TRY(hipEventRecord(s.ev.ev[3], st));
  int bad = 0;
  GLIA_HIP_TRY(hipMemcpyAsync(&bad, d.bad, sizeof(int), hipMemcpyDeviceToHost, st));
  std::vector<int> dcnt;
  std::vector<unsigned> err((size_t)T * kC * 3);
  GLIA_HIP_TRY(hipMemcpyAsync(err.data(), d.errcnt + (size_t)b.tree0 * kC * 3, sizeof(unsigned) * err.size(), hipMemcpyDeviceToHost, st));
  std::vector<std::vector<int>> leaf;
  if (s.o.importance) {
    dcnt.resize((size_t)T * D * nclass);
    GLIA_HIP_TRY(hipMemcpyAsync(dcnt.data(), d.dcnt, sizeof(int) * dcnt.size(), hipMemcpyDeviceToHost, st));
    leaf.resize((size_t)T);
    for (int t = 0; t < T; ++t) {
      leaf[t].resize(h_left[t].size() * nclass);
      GLIA_HIP_TRY(hipMemcpyAsync(leaf[t].data(), d.leafcnt + (size_t)t * d.cap * nclass, sizeof(int) * leaf[t].size(), hipMemcpyDeviceToHost, st));
    }
  }
  GLIA_HIP_TRY(hipStreamSynchronize(st));
  GLIA_HIP_TRY(hipGetLastError());
  s.tm->ms_walk += s.ev.ms(0, 1); s.tm->ms_tally += s.ev.ms(1, 2); s.tm->ms_importance += s.ev.ms(2, 3);
  if (bad) { set_error("forest_train: a grown tree holds a node no walk can follow"); count_internal_error(); return GLIA_HMT_ERR_INTERNAL; }
  for (int t = 0; t < T; ++t) {
    long long n_k[kC], m = 0;
    for (int k = 0; k < kC; ++k) { n_k[k] = err[((size_t)t * kC + k) * 3 + 2]; m += n_k[k]; }
    s.tm->oob_rows += m;
    if (!s.o.importance) continue;
    s.tm->walks_nominal += m * D;
    s.sums.add_tree(&dcnt[(size_t)t * D * nclass], n_k);
    std::vector<long long> cnt(leaf[t].begin(), leaf[t].end());
    s.sums.add_tree_gini(h_left[t].data(), h_var[t].data(), h_left[t].size(), &cnt, s.w.data());
  }
  return GLIA_HMT_OK;
}

int OobPass::finish(ForestModel* model) {
  Impl& s = *p_;
  OobDev& d = s.d;
  ForestModel& m = *model;
  const int nclass = d.nclass;
  std::vector<int> counttr((size_t)nclass * d.N);
  std::vector<unsigned> err((size_t)s.ntree * kC * 3);
  unsigned long long walks = 0;
  GLIA_HIP_TRY(hipMemcpyAsync(counttr.data(), d.counttr, sizeof(int) * counttr.size(), hipMemcpyDeviceToHost, s.stream));
  GLIA_HIP_TRY(hipMemcpyAsync(err.data(), d.errcnt, sizeof(unsigned) * err.size(), hipMemcpyDeviceToHost, s.stream));
  GLIA_HIP_TRY(hipMemcpyAsync(&walks, d.walks, sizeof(walks), hipMemcpyDeviceToHost, s.stream));
  GLIA_HIP_TRY(hipStreamSynchronize(s.stream));
  s.tm->walks_done = (int64_t)walks;
  m.oob_rows = d.N; m.oob_dim = d.D;
  if (s.o.oob) {
    std::vector<long long> pairs((size_t)s.ntree * nclass * 2);
    for (int t = 0; t < s.ntree; ++t)
      for (int k = 0; k < nclass; ++k) {
        pairs[((size_t)t * nclass + k) * 2] = err[((size_t)t * kC + k) * 3];
        pairs[((size_t)t * nclass + k) * 2 + 1] = err[((size_t)t * kC + k) * 3 + 1];
      }
    oob_errtr(pairs, s.ntree, nclass, &m.errtr, &m.err_wrong, &m.err_seen);
    oob_votes(counttr, nclass, d.N, &m.outcl, &m.oob_times, &m.votes);
    m.counttr.swap(counttr);
  }
  if (s.o.importance) s.sums.finish(s.ntree, &m.importance, &m.importanceSD);
  return GLIA_HMT_OK;
}

}  // namespace glia
