// glia_amd/csrc/bc_feat_batch.hip -- feature rows of a GIVEN merge order, parallel over merges (glia_hmt_bc_feat_batch).
//
// Reference: hmt/main_bc_feat.cxx:59-95 computes the region features of every tree node and the boundary features of every merge in
// parfor loops (util/mp.hxx:24-106).  The replay of the order through the classifier loop (greedy_bc.hip, req.forced) is one
// contraction at a time on one workgroup; here the tree is known beforehand (tree_paths.hpp), so every set a row looks at is a
// function of the tree and of the leaf / directed-pair records of the accumulation pass:
//   P(x)   = sum of the leaves' region records                      bottom-up by height, pstats_add (the loop's own association)
//   B(x)   = B(c0) + B(c1) - A(x)                                   A(x) = the MUTUAL entries whose leaves are first joined at x
//   Sh(i)  = the entries first joined at R + i: mutual ones, and non-mutual ones whose target leaf is alive inside its side
//   min / max of B(x): every entry applies to the nodes of an ancestor path; two blocks per entry in tables T[j], then one
//            push-down sweep per level (integer atomicMin / atomicMax on the order-preserving words: no arrival order shows)
// A(x) and Sh(i) are reductions of the entries grouped by join node: a stable radix sort on the join node keeps the entries of a node
// in entry order, and one wave per node adds them lane-strided and folds the 64 partial sets in a fixed tree -- one association of the
// f64 sums per input, no f64 atomics.  No kernel waits for another workgroup: a height level is a launch, and runs of levels with few
// nodes are looped over by ONE workgroup with a barrier between levels.  The row kernel calls the feature code of bc_features.hpp
// (region_feats_multi, boundary_feats_multi, finish_features) and writes every column straight to its slot in global memory.
#include <chrono>
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>

#include "bc_features.hpp"
#include "greedy_common.hpp"
#include "tree_paths.hpp"

namespace glia {

namespace {

constexpr uint32_t kSmallLevel = 256;     // (node, channel) items of a height level up to which one workgroup loops over levels

struct FbTree {
  uint32_t R, M;
  size_t nn;
  int levels;
  const uint32_t* anc;        // [levels][nn]
  const uint32_t* pos;        // [R]
  const uint32_t *lo, *hi;    // [nn]
  const uint32_t* depth;      // [nn]
  const uint32_t* forced;     // [M][2]
};
struct FbSets {               // per channel
  PStats* P[kMaxChannels];    // [nn]
  EStats* B[kMaxChannels];    // [nn]   additive fields only; min / max come from the T tables
  EStats* A[kMaxChannels];    // [M]
  EStats* Sh[kMaxChannels];   // [M]
  const uint32_t* prec[kMaxChannels];
  const uint32_t* rrec[kMaxChannels];
  int bins[kMaxChannels];
};
// (c is uniform: scalar selects instead of an indexed load from the argument segment)
#define FB_SEL(s, f, c) ((c) == 1 ? (s).f[1] : (c) == 2 ? (s).f[2] : (c) == 3 ? (s).f[3] : (s).f[0])

__global__ void fb_anc_double(const uint32_t* prev, uint32_t* next, size_t nn) {
  const size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v < nn) next[v] = tp::anc_double(prev, (uint32_t)v);
}

// per directed entry: dense leaves, mutual flag, the climb to the child of the join node
__global__ void fb_entries(FbTree t, const uint32_t* pa, const uint32_t* pb, long long P, const uint32_t* rlabel, uint32_t* ea, uint32_t* eb,
                           uint8_t* eflag, uint32_t* etop, uint32_t* ejoin, uint32_t* eplen) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= P) return;
  const uint32_t la = pa[e], lb = pb[e];
  const uint32_t a = find_label(rlabel, t.R, la), b = find_label(rlabel, t.R, lb);
  const bool mutual = find_pair(pa, pb, P, lb, la) >= 0;
  const tp::Climb c = tp::climb_below(t.anc, t.nn, t.levels, t.lo, t.hi, a, t.pos[b]);
  ea[e] = a; eb[e] = b; eflag[e] = mutual ? 1 : 0;
  etop[e] = c.top;
  ejoin[e] = t.anc[c.top];                                     // anc[0] = parent
  eplen[e] = tp::path_nodes(mutual, c.steps, t.depth[a]);
}

// per leaf: its run of entries (they ascend by source label), non-mutual out-entries, extreme positions of its mutual partners
__global__ void fb_leaf_alive(FbTree t, const uint32_t* pa, long long P, const uint32_t* rlabel, const uint32_t* eb, const uint8_t* eflag,
                              uint32_t* le_start, uint32_t* nm_out, uint32_t* pmin, uint32_t* pmax) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r > t.R) return;
  if (r == t.R) { le_start[r] = (uint32_t)P; return; }
  const uint32_t key = rlabel[r];
  long long lo = 0, hi = P;
  while (lo < hi) { const long long mid = (lo + hi) >> 1; if (pa[mid] < key) lo = mid + 1; else hi = mid; }
  le_start[r] = (uint32_t)lo;
  uint32_t nm = 0, mn = tp::kNoNode, mx = 0;
  for (long long i = lo; i < P && pa[i] == key; ++i) {
    if (!(eflag[i] & 1)) { ++nm; continue; }
    const uint32_t q = t.pos[eb[i]];
    mn = q < mn ? q : mn; mx = q > mx ? q : mx;
  }
  nm_out[r] = nm; pmin[r] = mn; pmax[r] = mx;
}

// sort key (merge index of the join node; kNoNode: never joined) and the shared-boundary flag of every entry:
// "alive" (boundaryWith, type/region.hxx:42-51): the target leaf owns a non-mutual entry, or a mutual partner outside its side
__global__ void fb_keys(FbTree t, long long P, const uint32_t* eb, const uint32_t* etop, const uint32_t* ejoin, uint8_t* eflag, const uint32_t* nm_out,
                        const uint32_t* pmin, const uint32_t* pmax, uint32_t* keys, uint32_t* vals) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= P) return;
  const uint32_t join = ejoin[e];
  vals[e] = (uint32_t)e;
  if (join == tp::kNoNode) { keys[e] = tp::kNoNode; return; }
  const uint32_t m = join - t.R;
  keys[e] = m;
  uint8_t f = eflag[e];
  bool in_sh = f & 1;
  if (!in_sh) {
    const uint32_t c0 = t.forced[2 * (size_t)m], c1 = t.forced[2 * (size_t)m + 1];
    const uint32_t side = c0 == etop[e] ? c1 : c0;             // the side of the merge that holds the target leaf
    const uint32_t b = eb[e];
    in_sh = nm_out[b] > 0 || (pmin[b] != tp::kNoNode && (pmin[b] < t.lo[side] || pmax[b] >= t.hi[side]));
  }
  if (in_sh) eflag[e] = f | 2;
}

__device__ __forceinline__ void fb_load_entry(const uint32_t* w, int bins, int nthr, EStats& s) {
  s.n = w[P_CNT];
#pragma unroll
  for (int i = 0; i < GLIA_HMT_MAX_THRESH; ++i) s.thr[i] = i < nthr ? w[P_THR + i] : 0;
  s.mn = ord_float(~w[P_MIN]); s.mx = ord_float(w[P_MAX]);
  memcpy(&s.sum, &w[P_SUM], 8); memcpy(&s.sq, &w[P_SQ], 8);
#pragma unroll
  for (int k = 0; k < GLIA_HMT_MAX_BINS; ++k) s.hist[k] = k < bins ? w[P_HIST + k] : 0;
}

// one wave per merge: A = the mutual entries joined there, Sh = its shared boundary (entries sorted by join node, in entry order)
__global__ __launch_bounds__(64) void fb_reduce_join(const uint32_t* ks, const uint32_t* vs, long long P, uint32_t M, const uint8_t* eflag, const uint32_t* prec,
                                                     int bins, int nthr, EStats* A, EStats* Sh) {
  __shared__ EStats sa[64], ss[64];
  const uint32_t m = blockIdx.x, lane = threadIdx.x;
  if (m >= M) return;
  long long lo = 0, hi = P;
  while (lo < hi) { const long long mid = (lo + hi) >> 1; if (ks[mid] < m) lo = mid + 1; else hi = mid; }
  const long long begin = lo;
  hi = P;
  while (lo < hi) { const long long mid = (lo + hi) >> 1; if (ks[mid] <= m) lo = mid + 1; else hi = mid; }
  const long long end = lo;
  EStats a, s, x;
  estats_clear(a); estats_clear(s);
  for (long long i = begin + lane; i < end; i += 64) {
    const uint32_t e = vs[i];
    const uint8_t f = eflag[e];
    fb_load_entry(prec + (size_t)e * kPairWords, bins, nthr, x);
    if (f & 1) estats_add(a, x);
    if (f & 2) estats_add(s, x);
  }
  sa[lane] = a; ss[lane] = s;
  __syncthreads();
  for (uint32_t d = 32; d >= 1; d >>= 1) {
    if (lane < d) { estats_add(sa[lane], sa[lane + d]); estats_add(ss[lane], ss[lane + d]); }
    __syncthreads();
  }
  if (lane == 0) { A[m] = sa[0]; Sh[m] = ss[0]; }
}

// leaves: P from the region record, B = the leaf's entries in entry order
__global__ void fb_leaves(uint32_t R, const uint32_t* rrec, const uint32_t* prec, const uint32_t* le_start, int bins, int nthr, PStats* Pn, EStats* Bn) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const uint32_t* w = &rrec[(size_t)r * kRegionWords];
  PStats p;
  p.n = w[R_CNT]; p.border = w[R_BORDER];
  for (int d = 0; d < 3; ++d) { p.lo[d] = (int)(0x7fffffffu - w[R_LO + d]); p.hi[d] = (int)w[R_HI + d] - 1; }
  p.mn = ord_float(~w[R_MIN]); p.mx = ord_float(w[R_MAX]);
  memcpy(&p.sum, &w[R_SUM], 8); memcpy(&p.sq, &w[R_SQ], 8);
#pragma unroll
  for (int k = 0; k < GLIA_HMT_MAX_BINS; ++k) p.hist[k] = k < bins ? w[R_HIST + k] : 0;
  Pn[r] = p;
  EStats b, x;
  estats_clear(b);
  for (uint32_t i = le_start[r]; i < le_start[r + 1]; ++i) { fb_load_entry(prec + (size_t)i * kPairWords, bins, nthr, x); estats_add(b, x); }
  Bn[r] = b;
}

// an inner node from its children (both lower: written by an earlier launch, or before the last barrier of this workgroup)
__device__ __forceinline__ void fb_node(const FbSets& s, int c, uint32_t x, uint32_t R, const uint32_t* forced) {
  const uint32_t m = x - R, c0 = forced[2 * (size_t)m], c1 = forced[2 * (size_t)m + 1];
  PStats* Pn = FB_SEL(s, P, c);
  EStats* Bn = FB_SEL(s, B, c);
  const EStats* An = FB_SEL(s, A, c);
  PStats p = Pn[c0];
  pstats_add(p, Pn[c1]);
  Pn[x] = p;
  EStats b = Bn[c0];
  estats_add(b, Bn[c1]);
  estats_sub_additive(b, An[m]);
  Bn[x] = b;
}
__global__ void fb_level(FbSets s, int K, const uint32_t* byh, uint32_t off, uint32_t cnt, uint32_t R, const uint32_t* forced) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= cnt * (uint32_t)K) return;
  fb_node(s, (int)(g % (uint32_t)K), byh[off + g / (uint32_t)K], R, forced);
}
// heights h0 .. h1, each with at most kSmallLevel items: one workgroup, a barrier between levels
__global__ __launch_bounds__(256) void fb_levels_small(FbSets s, int K, const uint32_t* byh, const uint32_t* level_off, uint32_t h0, uint32_t h1, uint32_t R,
                                                       const uint32_t* forced) {
  for (uint32_t h = h0; h <= h1; ++h) {
    const uint32_t off = level_off[h], cnt = level_off[h + 1] - off;
    for (uint32_t g = threadIdx.x; g < cnt * (uint32_t)K; g += blockDim.x) fb_node(s, (int)(g % (uint32_t)K), byh[off + g / (uint32_t)K], R, forced);
    __syncthreads();
  }
}

// min / max of the boundary sets: T[c][j][v], words in the order of the values (min: 0xFFFFFFFF = none, max: 0 = none)
__global__ void fb_paths(FbTree t, long long P, int K, FbSets s, const uint32_t* ea, const uint32_t* eplen, uint32_t* Tmin, uint32_t* Tmax) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= P) return;
  const uint32_t a = ea[e], k = eplen[e];
  for (int c = 0; c < K; ++c) {
    const uint32_t* w = FB_SEL(s, prec, c) + (size_t)e * kPairWords;
    const uint32_t omin = ~w[P_MIN], omax = w[P_MAX];
    uint32_t* tmn = Tmin + (size_t)c * t.levels * t.nn;
    uint32_t* tmx = Tmax + (size_t)c * t.levels * t.nn;
    tp::path_update(t.anc, t.nn, t.levels, a, k, [&](int j, uint32_t v) {
      atomicMin(&tmn[(size_t)j * t.nn + v], omin);
      atomicMax(&tmx[(size_t)j * t.nn + v], omax);
    });
  }
}
__global__ void fb_push(FbTree t, int j, int K, uint32_t* Tmin, uint32_t* Tmax) {
  const size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= t.nn) return;
  for (int c = 0; c < K; ++c) {
    uint32_t* tmn = Tmin + (size_t)c * t.levels * t.nn;
    uint32_t* tmx = Tmax + (size_t)c * t.levels * t.nn;
    tp::push_down(t.anc, t.nn, j, (uint32_t)v, [&](int jj, uint32_t x) { return tmn[(size_t)jj * t.nn + x]; },
                  [&](int jj, uint32_t x, uint32_t val) { if (val != 0xFFFFFFFFu) atomicMin(&tmn[(size_t)jj * t.nn + x], val); });
    tp::push_down(t.anc, t.nn, j, (uint32_t)v, [&](int jj, uint32_t x) { return tmx[(size_t)jj * t.nn + x]; },
                  [&](int jj, uint32_t x, uint32_t val) { if (val != 0u) atomicMax(&tmx[(size_t)jj * t.nn + x], val); });
  }
}

// ---- row assembly: one thread per merge, every column written straight to its slot (no private feature array) ----
struct FbNodeView {
  const FbSets* s; const uint32_t* Tmin; const uint32_t* Tmax; size_t nn; int levels; uint32_t x;
  __device__ __forceinline__ const PStats* P(int cc) const { return FB_SEL(*s, P, cc) + x; }
  __device__ __forceinline__ const EStats* B(int cc) const { return FB_SEL(*s, B, cc) + x; }
  __device__ __forceinline__ float bmn(int cc) const { const uint32_t o = Tmin[(size_t)cc * levels * nn + x]; return o == 0xFFFFFFFFu ? __builtin_inff() : ord_float(o); }
  __device__ __forceinline__ float bmx(int cc) const { const uint32_t o = Tmax[(size_t)cc * levels * nn + x]; return o == 0u ? -__builtin_inff() : ord_float(o); }
};
__device__ __forceinline__ void fb_region_block(const BcCfg& c, const FbNodeView& v, double* out, double& area, double& perim) {
  const PStats* p0 = v.P(0);
  const EStats* b0 = v.B(0);
  feat::ShapeIn r;
  r.n = p0->n; r.border = p0->border; r.bn = b0->n;
  for (int i = 0; i < 3; ++i) { r.lo[i] = p0->lo[i]; r.hi[i] = p0->hi[i]; }
  for (int i = 0; i < GLIA_HMT_MAX_THRESH; ++i) r.thr[i] = b0->thr[i];
  auto src = [&c, &v](int kind, int i) -> feat::ImgSrc {
    const int cc = kind == 0 ? c.rc[i] : (kind == 1 ? c.lc[i] : c.bc[i]);
    if (kind < 2) { const PStats* p = v.P(cc); return feat::ImgSrc{p->hist, nullptr, nullptr, p->n, p->sum, p->sq, p->mn, p->mx, nullptr}; }
    const EStats* b = v.B(cc);
    return feat::ImgSrc{b->hist, nullptr, nullptr, b->n, b->sum, b->sq, v.bmn(cc), v.bmx(cc), nullptr};
  };
  feat::region_feats_multi(c, r, src, out, area, perim);
}
__global__ __launch_bounds__(64) void fb_rows(BcCfg c, FbSets s, const uint32_t* Tmin, const uint32_t* Tmax, size_t nn, int levels, uint32_t R, uint32_t M,
                                              const uint32_t* forced, double* rows, int stride) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  double* out = rows + (size_t)i * stride;
  const FbNodeView v0{&s, Tmin, Tmax, nn, levels, forced[2 * (size_t)i]}, v1{&s, Tmin, Tmax, nn, levels, forced[2 * (size_t)i + 1]},
      v3{&s, Tmin, Tmax, nn, levels, R + i};
  // x1 = the region of smaller normalised area (main_bc_feat.cxx:88-91); ties keep the order's first region first
  const bool swap = feat::sdiv((double)v0.P(0)->n, c.norm_area, 0.0) > feat::sdiv((double)v1.P(0)->n, c.norm_area, 0.0);
  const FbNodeView& x1 = swap ? v1 : v0;
  const FbNodeView& x2 = swap ? v0 : v1;
  double ar1, pe1, ar2, pe2, ar3, pe3;
  fb_region_block(c, x1, out + c.bfdim, ar1, pe1);
  fb_region_block(c, x2, out + c.bfdim + c.rfdim, ar2, pe2);
  fb_region_block(c, v3, out + c.bfdim + 2 * c.rfdim, ar3, pe3);
  auto src_of = [&c](const FbNodeView& v) {
    return [&c, &v](int kind, int k) -> feat::ImgSrc {
      const PStats* p = v.P(kind == 0 ? c.rc[k] : c.lc[k]);
      return feat::ImgSrc{p->hist, nullptr, nullptr, p->n, p->sum, p->sq, p->mn, p->mx, nullptr};
    };
  };
  const EStats* sh0 = FB_SEL(s, Sh, 0) + i;
  auto srcSh = [&](int k) -> feat::ImgSrc {
    const int cc = c.bc[k];
    const EStats* sh = FB_SEL(s, Sh, cc) + i;
    return feat::ImgSrc{sh->hist, nullptr, nullptr, sh->n, sh->sum, sh->sq, sh->mn, sh->mx, nullptr};
  };
  feat::boundary_feats_multi(c, sh0->n, sh0->thr, ar1, pe1, ar2, pe2, src_of(x1), src_of(x2), srcSh, nullptr, out);
  feat::finish_features(c, out);
}

template <class T> int fb_upload(DeviceBuffers& buf, const std::vector<T>& h, T** d, hipStream_t stream) {
  if (int rc = buf.get(d, h.size(), false, stream)) return rc;
  if (!h.empty()) GLIA_HIP_TRY(hipMemcpyAsync(*d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice, stream));
  return GLIA_HMT_OK;
}
inline unsigned fb_grid(size_t n, unsigned block = 256) { return (unsigned)((n + block - 1) / block); }

}  // namespace

int bc_feat_batch_rows(const RagArrays& rag, const BcCfg& cfg, const uint32_t* forced, int64_t M, hipStream_t stream, std::vector<double>* rows,
                       BcFeatBatchInfo* info) {
  const auto t_begin = std::chrono::steady_clock::now();
  *info = BcFeatBatchInfo();
  const int64_t R = rag.R;
  const long long P = rag.P;
  const int K = cfg.K;
  // the limit of the replay (greedy_bc), with its message: both routes accept and refuse the same configurations
  if (bc_full_dim(cfg) > kMaxFeat || cfg.fdim > kMaxFeat) {
    set_error("merge_order_bc: feature vector too long (" + std::to_string(bc_full_dim(cfg)) + " columns before --simpf, limit " + std::to_string(kMaxFeat) + ")");
    return GLIA_HMT_ERR_ARG;
  }
  rows->assign((size_t)M * cfg.fdim, 0.0);
  if (M <= 0) return GLIA_HMT_OK;
  if (K < 1 || K > kMaxChannels) { set_error("bc_feat_batch: more than " + std::to_string(kMaxChannels) + " image channels"); return GLIA_HMT_ERR_UNSUPPORTED; }
  const size_t nn = (size_t)R + (size_t)M;
  if (nn >= 0x7FFFFFFFull || P >= 0x7FFFFFFFll) { set_error("bc_feat_batch: more than 2^31 tree nodes or directed pairs"); return GLIA_HMT_ERR_UNSUPPORTED; }
  // ---- host plan, O(R + M): tree tables, nodes by height ----
  std::vector<int64_t> parent;
  std::vector<uint32_t> pos, at, lo, hi, depth, height;
  tp::tree_intervals(forced, (uint32_t)R, M, &parent, &pos, &at, &lo, &hi);
  const std::pair<uint32_t, uint32_t> dh = tp::tree_depth_height(forced, (uint32_t)R, M, parent, &depth, &height);
  const int levels = tp::levels_for(dh.first);
  const uint32_t H = dh.second;
  // memory: ancestor and T tables nn x levels x (1 + 2 K) words, the sets (nn + M) x K x (120 + 112) bytes
  const unsigned long long need = (unsigned long long)nn * levels * (1 + 2 * K) * 4 + (unsigned long long)(nn + M) * K * (sizeof(PStats) + sizeof(EStats)) +
                                  (unsigned long long)P * 40;
  if (need > (48ull << 30)) {
    set_error("bc_feat_batch: the tables of this merge order need " + std::to_string(need >> 20) + " MiB (" + std::to_string(nn) + " nodes, " +
              std::to_string(levels) + " ancestor levels, " + std::to_string(K) + " channels), more than the bound of 48 GiB");
    return GLIA_HMT_ERR_UNSUPPORTED;
  }
  std::vector<uint32_t> anc0(nn), level_off((size_t)H + 2, 0), byh((size_t)M), forced_v(forced, forced + 2 * (size_t)M);
  for (size_t x = 0; x < nn; ++x) anc0[x] = parent[x] < 0 ? tp::kNoNode : (uint32_t)parent[x];
  for (int64_t i = 0; i < M; ++i) level_off[height[(size_t)R + i] + 1] += 1;       // counting sort of the inner nodes by height (>= 1)
  for (size_t h = 1; h < level_off.size(); ++h) level_off[h] += level_off[h - 1];   // level_off[h] = nodes of height < h
  {
    std::vector<uint32_t> fill(level_off.begin(), level_off.end() - 1);
    for (int64_t i = 0; i < M; ++i) byh[fill[height[(size_t)R + i]]++] = (uint32_t)(R + i);
  }
  DeviceBuffers buf;
  int rc;
  CallEvents<3> ev;
  if ((rc = ev.create())) return rc;
  uint32_t *d_anc, *d_pos, *d_lo, *d_hi, *d_depth, *d_forced, *d_byh, *d_level_off;
  if ((rc = buf.get(&d_anc, nn * (size_t)levels, false, stream))) return rc;
  GLIA_HIP_TRY(hipMemcpyAsync(d_anc, anc0.data(), 4 * nn, hipMemcpyHostToDevice, stream));
  if ((rc = fb_upload(buf, pos, &d_pos, stream)) || (rc = fb_upload(buf, lo, &d_lo, stream)) || (rc = fb_upload(buf, hi, &d_hi, stream)) ||
      (rc = fb_upload(buf, depth, &d_depth, stream)) || (rc = fb_upload(buf, forced_v, &d_forced, stream)) || (rc = fb_upload(buf, byh, &d_byh, stream)) ||
      (rc = fb_upload(buf, level_off, &d_level_off, stream))) return rc;
  const FbTree t{(uint32_t)R, (uint32_t)M, nn, levels, d_anc, d_pos, d_lo, d_hi, d_depth, d_forced};
  FbSets s;
  memset(&s, 0, sizeof(s));
  for (int c = 0; c < K; ++c) {
    if ((rc = buf.get(&s.P[c], nn, false, stream)) || (rc = buf.get(&s.B[c], nn, false, stream)) || (rc = buf.get(&s.A[c], (size_t)M, false, stream)) ||
        (rc = buf.get(&s.Sh[c], (size_t)M, false, stream))) return rc;
    s.prec[c] = rag.c_prec[c];
    s.rrec[c] = rag.c_rrec[c];
    s.bins[c] = cfg.cbins[c];
  }
  uint32_t *d_ea, *d_eb, *d_etop, *d_ejoin, *d_eplen, *d_keys, *d_vals, *d_ks, *d_vs, *d_le_start, *d_nm, *d_pmin, *d_pmax, *d_tmin, *d_tmax;
  uint8_t* d_eflag;
  const size_t Pn = (size_t)(P ? P : 1), tsize = (size_t)K * levels * nn;
  if ((rc = buf.get(&d_ea, Pn, false, stream)) || (rc = buf.get(&d_eb, Pn, false, stream)) || (rc = buf.get(&d_etop, Pn, false, stream)) ||
      (rc = buf.get(&d_ejoin, Pn, false, stream)) || (rc = buf.get(&d_eplen, Pn, false, stream)) || (rc = buf.get(&d_keys, Pn, false, stream)) ||
      (rc = buf.get(&d_vals, Pn, false, stream)) || (rc = buf.get(&d_ks, Pn, false, stream)) || (rc = buf.get(&d_vs, Pn, false, stream)) ||
      (rc = buf.get(&d_eflag, Pn, false, stream)) || (rc = buf.get(&d_le_start, (size_t)R + 1, false, stream)) || (rc = buf.get(&d_nm, (size_t)R, false, stream)) ||
      (rc = buf.get(&d_pmin, (size_t)R, false, stream)) || (rc = buf.get(&d_pmax, (size_t)R, false, stream)) || (rc = buf.get(&d_tmin, tsize, false, stream)) ||
      (rc = buf.get(&d_tmax, tsize, false, stream))) return rc;
  double* d_rows;
  const int stride = bc_full_dim(cfg) > cfg.fdim ? bc_full_dim(cfg) : cfg.fdim;     // the simple selection is compacted in place
  if ((rc = buf.get(&d_rows, (size_t)M * stride, false, stream))) return rc;
  GLIA_HIP_TRY(hipMemsetAsync(d_tmin, 0xFF, 4 * tsize, stream));
  GLIA_HIP_TRY(hipMemsetAsync(d_tmax, 0, 4 * tsize, stream));
  info->ms_plan = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  int64_t launches = 0;
  GLIA_HIP_TRY(hipEventRecord(ev.ev[0], stream));
  // ---- ancestor tables by doubling ----
  for (int j = 1; j < levels; ++j, ++launches)
    hipLaunchKernelGGL(fb_anc_double, dim3(fb_grid(nn)), dim3(256), 0, stream, d_anc + (size_t)(j - 1) * nn, d_anc + (size_t)j * nn, nn);
  // ---- entries: join node, path length, aliveness, grouping by join node ----
  hipLaunchKernelGGL(fb_entries, dim3(fb_grid(Pn)), dim3(256), 0, stream, t, rag.d_pa, rag.d_pb, P, rag.d_rlabel, d_ea, d_eb, d_eflag, d_etop, d_ejoin, d_eplen);
  hipLaunchKernelGGL(fb_leaf_alive, dim3(fb_grid((size_t)R + 1)), dim3(256), 0, stream, t, rag.d_pa, P, rag.d_rlabel, d_eb, d_eflag, d_le_start, d_nm, d_pmin, d_pmax);
  hipLaunchKernelGGL(fb_keys, dim3(fb_grid(Pn)), dim3(256), 0, stream, t, P, d_eb, d_etop, d_ejoin, d_eflag, d_nm, d_pmin, d_pmax, d_keys, d_vals);
  launches += 3;
  GLIA_HIP_TRY(hipGetLastError());
  if (P) {
    if ((rc = rocprim_run(buf, stream, [&](void* tmp, size_t& b) { return rocprim::radix_sort_pairs(tmp, b, d_keys, d_ks, d_vals, d_vs, (size_t)P, 0, 32, stream); }))) return rc;
    ++launches;
  }
  // ---- A(x), Sh(i); leaves; inner nodes bottom-up by height ----
  for (int c = 0; c < K; ++c, launches += 2) {
    hipLaunchKernelGGL(fb_reduce_join, dim3((unsigned)M), dim3(64), 0, stream, d_ks, d_vs, P, (uint32_t)M, d_eflag, s.prec[c], s.bins[c], cfg.T, s.A[c], s.Sh[c]);
    hipLaunchKernelGGL(fb_leaves, dim3(fb_grid((size_t)R)), dim3(256), 0, stream, (uint32_t)R, s.rrec[c], s.prec[c], d_le_start, s.bins[c], cfg.T, s.P[c], s.B[c]);
  }
  GLIA_HIP_TRY(hipGetLastError());
  for (uint32_t h = 1; h <= H;) {
    const uint32_t cnt = level_off[h + 1] - level_off[h];
    if ((unsigned long long)cnt * K > kSmallLevel) {
      hipLaunchKernelGGL(fb_level, dim3(fb_grid((size_t)cnt * K, 128)), dim3(128), 0, stream, s, K, d_byh, level_off[h], cnt, (uint32_t)R, d_forced);
      ++h;
    } else {
      uint32_t h1 = h;
      while (h1 + 1 <= H && (unsigned long long)(level_off[h1 + 2] - level_off[h1 + 1]) * K <= kSmallLevel) ++h1;
      hipLaunchKernelGGL(fb_levels_small, dim3(1), dim3(256), 0, stream, s, K, d_byh, d_level_off, h, h1, (uint32_t)R, d_forced);
      h = h1 + 1;
    }
    ++launches;
  }
  GLIA_HIP_TRY(hipGetLastError());
  // ---- min / max of the boundary sets along the entries' paths ----
  if (P) { hipLaunchKernelGGL(fb_paths, dim3(fb_grid(Pn)), dim3(256), 0, stream, t, P, K, s, d_ea, d_eplen, d_tmin, d_tmax); ++launches; }
  for (int j = levels - 1; j >= 1; --j, ++launches) hipLaunchKernelGGL(fb_push, dim3(fb_grid(nn)), dim3(256), 0, stream, t, j, K, d_tmin, d_tmax);
  GLIA_HIP_TRY(hipGetLastError());
  GLIA_HIP_TRY(hipEventRecord(ev.ev[1], stream));
  // ---- rows ----
  hipLaunchKernelGGL(fb_rows, dim3(fb_grid((size_t)M, 64)), dim3(64), 0, stream, cfg, s, d_tmin, d_tmax, nn, levels, (uint32_t)R, (uint32_t)M, d_forced, d_rows, stride);
  ++launches;
  GLIA_HIP_TRY(hipGetLastError());
  GLIA_HIP_TRY(hipEventRecord(ev.ev[2], stream));
  GLIA_HIP_TRY(hipMemcpy2DAsync(rows->data(), sizeof(double) * cfg.fdim, d_rows, sizeof(double) * stride, sizeof(double) * cfg.fdim, (size_t)M, hipMemcpyDeviceToHost, stream));
  GLIA_HIP_TRY(hipStreamSynchronize(stream));
  info->ms_sets = ev.ms(0, 1); info->ms_rows = ev.ms(1, 2);
  info->height = H; info->launches = launches; info->path_updates = 2ll * P * K;
  return GLIA_HMT_OK;
}

}  // namespace glia
