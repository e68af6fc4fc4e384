// glia_amd/csrc/bc_label.cpp -- truth-based merge labels for a GIVEN merge order (hmt/main_bc_label_ri.cxx, main_bc_label_vi.cxx).
//
// The device counts the (label, truth) pairs (label_overlap.hip) and one walk over that table maps its labels to leaves
// (leaf_truth_counts, dense_order.hpp): the leaf x truth contingency table.  Here, per tree node x and truth t != 0 (BG_VAL is
// excluded) with c_xt voxels of x:  n(x) = sum_t c_xt,  size(x) = all voxels of x,  Q(x) = sum_t c_xt^2,  E(x) = sum_t c_xt log2 c_xt.
// A list L of regions that partitions x (r0 + r1, the merged region, a best-split list) then has (stats::pairStats,
// util/stats.hxx:189-229, and stats::vi, util/image_stats.hxx:69-110)
//   TP = sum_L (Q(i) - n(i)) / 2            pairs in one region = sum_L n(i) (n(i) - 1) / 2
//   pairs with one truth label = (Q(x) - n(x)) / 2,  all pairs = n(x) (n(x) - 1) / 2
//   VI * size(x) = E(x) + sum_L n(i) log2 n(i) - 2 sum_L E(i)          (terms with a count of 0 skipped, as the reference does)
// so a list is carried as two sums and every rule of the reference runs in O(merges) after the per-node values.
//
// Stage (b), the per-node values: small-to-large merging of per-node truth -> count maps along the merge order.  A merge moves
// the smaller map into the larger, so a leaf's entry moves O(log R) times: O(entries log R) in all, whatever the tree's depth.
// Q and n stay exact (Q grows by 2 a c for a truth met on both sides); E is carried in long double (64-bit significand) and grows by
// f(a + c) - f(a) - f(c), f(c) = c log2 c with log2 the host libm's.  The per-node alternative -- every (node, truth) pair visited
// once -- costs sum over nodes of their truth labels, which a deep order makes quadratic (DESIGN 3.7 has the measurement).
#include <algorithm>
#include <cmath>
#include <memory>
#include <queue>
#include <unordered_map>

#include "hmt_internal.hpp"

namespace glia {

namespace {

constexpr double kFEPS = 2.22e-16;                                   // glia_base.hxx:57
inline bool isfeq(double a, double b) { return std::fabs(a - b) < kFEPS; }   // glia_base.hxx:71-72
constexpr int kMerge = -1, kSplit = 1;                               // BC_LABEL_MERGE / BC_LABEL_SPLIT (hmt/bc_label.hxx:9-11)
typedef __int128 I128;

inline long double xlog2x(unsigned long long c) { return c ? (long double)c * (long double)std::log2((double)c) : 0.0L; }

// a list's pair sums: TP = sum_L (Q - n) / 2, same-region pairs = sum_L n (n - 1) / 2
struct ListSum {
  I128 tp = 0, same = 0;
  void add(const ListSum& o) { tp += o.tp; same += o.same; }
};

struct PairRates { double prec, rec, f1; };

// pairStats on the counts (util/stats.hxx:189-229), then precision / recall / f1 (:242-261) operation for operation.
// BigInt -> double: the counts are exact here; a count above 2^53 rounds to nearest (Boost's int512_t conversion is not pinned).
inline void pair_stats(const ListSum& L, unsigned long long n, unsigned long long Q, I128* TP, I128* TN, I128* FP, I128* FN) {
  const I128 nPair = (I128)n * ((I128)n - 1) / 2, key1 = ((I128)Q - (I128)n) / 2, key0 = L.same;
  *TP = L.tp;
  *TN = nPair - key1 + *TP - key0;
  *FP = key0 - *TP;
  *FN = key1 - *TP;
}
inline PairRates pair_f1(const ListSum& L, unsigned long long n, unsigned long long Q) {
  I128 TP, TN, FP, FN;
  pair_stats(L, n, Q, &TP, &TN, &FP, &FN);
  PairRates r;
  double den = (double)(TP + FP);
  r.prec = (double)TP / (!isfeq(den, 0.0) ? den : (den + kFEPS));
  den = (double)(TP + FN);
  r.rec = (double)TP / (!isfeq(den, 0.0) ? den : (den + kFEPS));
  r.f1 = 2.0 * r.prec * r.rec / (r.prec + r.rec);                    // 0 / 0 = NaN: mergeF1 > splitF1 is then false
  return r;
}
inline double rand_index(const ListSum& L, unsigned long long n, unsigned long long Q) {
  I128 TP, TN, FP, FN;
  pair_stats(L, n, Q, &TP, &TN, &FP, &FN);
  const double num = (double)(TP + TN);
  double den = (double)(FP + FN);
  den += num;
  return num / (!isfeq(den, 0.0) ? den : (den + kFEPS));
}

// majority over {-1, +1} (util/container.hxx:356-377): the counts live in a libstdc++ unordered_map<int, int>, which walks its
// two keys in reverse order of insertion; the first key with the largest count wins, so a tie goes to the label x[0] is not.
inline int majority(const int* x, int n) {
  int pos = 0;
  for (int i = 0; i < n; ++i) pos += x[i] == kSplit;
  if (2 * pos == n) return -x[0];
  return 2 * pos > n ? kSplit : kMerge;
}

}  // namespace

void node_truth_stats(const std::vector<TruthCount>& cnt, uint32_t R, const uint32_t* forced, int64_t M, NodeTruthStats* out, int64_t* moves,
                      int64_t* node_pairs) {
  const size_t nn = (size_t)R + (size_t)M;
  out->n.assign(nn, 0); out->size.assign(nn, 0); out->Q.assign(nn, 0); out->E.assign(nn, 0.0L);
  typedef std::unordered_map<uint32_t, unsigned long long> Map;
  std::vector<std::unique_ptr<Map>> maps(nn);
  int64_t mv = 0, np = 0;
  for (size_t i = 0; i < cnt.size();) {
    const uint32_t leaf = cnt[i].leaf;
    size_t j = i;
    while (j < cnt.size() && cnt[j].leaf == leaf) ++j;
    std::unique_ptr<Map> m(new Map);
    m->reserve(j - i);
    for (size_t k = i; k < j; ++k) {
      const unsigned long long c = cnt[k].count;
      out->size[leaf] += c;
      if (cnt[k].truth == 0) continue;                               // BG_VAL: in the region's size only
      (*m)[cnt[k].truth] = c;
      out->n[leaf] += c; out->Q[leaf] += c * c; out->E[leaf] += xlog2x(c);
    }
    np += (int64_t)m->size();
    maps[leaf] = std::move(m);
    i = j;
  }
  for (int64_t k = 0; k < M; ++k) {
    const uint32_t a = forced[2 * k], b = forced[2 * k + 1];
    const size_t x = (size_t)R + (size_t)k;
    std::unique_ptr<Map> big = std::move(maps[a]), small = std::move(maps[b]);
    if (!big) big.reset(new Map);
    if (!small) small.reset(new Map);
    if (big->size() < small->size()) std::swap(big, small);
    unsigned long long cross = 0;
    long double dE = 0.0L;
    for (const auto& e : *small) {
      unsigned long long& v = (*big)[e.first];
      if (v) { cross += v * e.second; dE += xlog2x(v + e.second) - xlog2x(v) - xlog2x(e.second); }
      v += e.second;
    }
    mv += (int64_t)small->size();
    out->n[x] = out->n[a] + out->n[b];
    out->size[x] = out->size[a] + out->size[b];
    out->Q[x] = out->Q[a] + out->Q[b] + 2 * cross;
    out->E[x] = out->E[a] + out->E[b] + dE;
    np += (int64_t)big->size();
    maps[x] = std::move(big);
  }
  if (moves) *moves = mv;
  if (node_pairs) *node_pairs = np;
}

int bc_label_rules(const std::vector<NodeTruthStats>& st, uint32_t R, const uint32_t* forced, int64_t M, const glia_hmt_bc_label_opts& o,
                   int32_t* labels) {
  const int nt = (int)st.size();
  const NodeTruthStats& s0 = st[0];
  auto own = [&](size_t x) {
    ListSum L;
    L.tp = ((I128)s0.Q[x] - (I128)s0.n[x]) / 2;
    L.same = (I128)s0.n[x] * ((I128)s0.n[x] - 1) / 2;
    return L;
  };
  // VI of a list over x per truth (stats::vi): (E(x) + sum_L f(n) - 2 sum_L E) / nPoint, nPoint = size(x)
  struct ViSum { std::vector<long double> fn, e; };
  auto vi_own = [&](size_t x) {
    ViSum v; v.fn.resize(nt); v.e.resize(nt);
    for (int t = 0; t < nt; ++t) { v.fn[t] = xlog2x(st[t].n[x]); v.e[t] = st[t].E[x]; }
    return v;
  };
  auto vi = [&](int t, size_t x, const ViSum& L) { return (st[t].E[x] + L.fn[t] - 2.0L * L.e[t]) / (long double)st[t].size[x]; };
  std::vector<int> tmp((size_t)nt);
  if (o.global_opt == 0) {
    if (o.metric == GLIA_HMT_BC_LABEL_VI) {                          // main_bc_label_vi.cxx:44-56, bc_label.hxx:16-26
      for (int64_t i = 0; i < M; ++i) {
        const size_t a = forced[2 * i], b = forced[2 * i + 1], x = (size_t)R + (size_t)i;
        ViSum sp = vi_own(a);
        const ViSum vb = vi_own(b), me = vi_own(x);
        for (int t = 0; t < nt; ++t) { sp.fn[t] += vb.fn[t]; sp.e[t] += vb.e[t]; }
        for (int t = 0; t < nt; ++t) tmp[t] = vi(t, x, me) < vi(t, x, sp) ? kMerge : kSplit;
        labels[i] = majority(tmp.data(), nt);
      }
      return GLIA_HMT_OK;
    }
    if (o.metric == GLIA_HMT_BC_LABEL_RI) {                          // main_bc_label_ri.cxx:85-90, bc_label.hxx:94-109
      for (int64_t i = 0; i < M; ++i) {
        const size_t a = forced[2 * i], b = forced[2 * i + 1], x = (size_t)R + (size_t)i;
        ListSum sp = own(a);
        sp.add(own(b));
        const double splitRI = rand_index(sp, s0.n[x], s0.Q[x]), mergeRI = rand_index(own(x), s0.n[x], s0.Q[x]);
        labels[i] = mergeRI > splitRI ? kMerge : kSplit;
      }
      return GLIA_HMT_OK;
    }
    // pair F1 (main_bc_label_ri.cxx:47-56, bc_label.hxx:44-66)
    std::vector<double> mergeF1((size_t)M);
    for (int64_t i = 0; i < M; ++i) {
      const size_t a = forced[2 * i], b = forced[2 * i + 1], x = (size_t)R + (size_t)i;
      ListSum sp = own(a);
      sp.add(own(b));
      const PairRates s = pair_f1(sp, s0.n[x], s0.Q[x]), m = pair_f1(own(x), s0.n[x], s0.Q[x]);
      mergeF1[i] = m.f1;
      int l;
      if (o.max_prec_drop < 1.0 && s.prec - m.prec > o.max_prec_drop) l = kSplit;
      else if (o.tweak)
        l = (m.f1 > s.f1 || (s.prec < kFEPS && s.rec < kFEPS && m.prec < kFEPS && m.rec < kFEPS) || (s.f1 == m.f1 && s.prec > 0.9 && m.prec > 0.9))
                ? kMerge : kSplit;
      else l = m.f1 > s.f1 ? kMerge : kSplit;
      labels[i] = l;
    }
    if (o.opt_split) {                                               // main_bc_label_ri.cxx:57-83: the best split list of every key
      std::vector<ListSum> best((size_t)R + (size_t)M);
      for (size_t x = 0; x < R; ++x) best[x] = own(x);               // a key not yet listed: its own region
      for (int64_t i = 0; i < M; ++i) {
        const size_t a = forced[2 * i], b = forced[2 * i + 1], x = (size_t)R + (size_t)i;
        ListSum sp = best[a];
        sp.add(best[b]);
        if (labels[i] == kSplit) best[x] = sp;
        else if (mergeF1[i] > pair_f1(sp, s0.n[x], s0.Q[x]).f1) best[x] = own(x);
        else { labels[i] = kSplit; best[x] = sp; }
      }
    }
    return GLIA_HMT_OK;
  }
  // global assignment over the tree of genTree (main_bc_label_ri.cxx:91-151, main_bc_label_vi.cxx:57-126): the inner nodes are
  // the merges in order, children before parents; F1 for the RI tool whatever --f1 says, VI (majority over truths) for the VI tool
  const bool use_vi = o.metric == GLIA_HMT_BC_LABEL_VI;
  const size_t nn = (size_t)R + (size_t)M;
  std::vector<ListSum> best(use_vi ? 0 : nn);
  std::vector<ViSum> vbest(use_vi ? nn : 0);
  for (size_t x = 0; x < R; ++x) { if (use_vi) vbest[x] = vi_own(x); else best[x] = own(x); }
  std::vector<int> lab((size_t)M);
  for (int64_t i = 0; i < M; ++i) {
    const size_t a = forced[2 * i], b = forced[2 * i + 1], x = (size_t)R + (size_t)i;
    bool merge;
    if (use_vi) {
      ViSum sp = vbest[a];
      for (int t = 0; t < nt; ++t) { sp.fn[t] += vbest[b].fn[t]; sp.e[t] += vbest[b].e[t]; }
      const ViSum me = vi_own(x);
      for (int t = 0; t < nt; ++t) tmp[t] = vi(t, x, me) < vi(t, x, sp) ? kMerge : kSplit;
      merge = majority(tmp.data(), nt) == kMerge;
      vbest[x] = merge ? me : sp;
    } else {
      ListSum sp = best[a];
      sp.add(best[b]);
      merge = pair_f1(own(x), s0.n[x], s0.Q[x]).f1 > pair_f1(sp, s0.n[x], s0.Q[x]).f1;
      best[x] = merge ? own(x) : sp;
    }
    lab[i] = merge ? kMerge : kSplit;
  }
  if (M > 0 && o.global_opt == 1) {                                  // path consistency by merging: BFS from the root (the last node)
    std::queue<int64_t> q;
    q.push(M - 1);
    while (!q.empty()) {
      const int64_t k = q.front();
      q.pop();
      if (lab[k] == kMerge) {
        std::vector<int64_t> stack{k};
        while (!stack.empty()) {
          const int64_t y = stack.back();
          stack.pop_back();
          lab[y] = kMerge;
          for (int s = 0; s < 2; ++s) if (forced[2 * y + s] >= R) stack.push_back((int64_t)forced[2 * y + s] - R);
        }
      } else {
        for (int s = 0; s < 2; ++s) if (forced[2 * k + s] >= R) q.push((int64_t)forced[2 * k + s] - R);
      }
    }
  } else if (o.global_opt == 2) {                                    // by splitting: a split node splits all its ancestors
    for (int64_t i = 0; i < M; ++i)                                  // children come first: one pass upwards
      for (int s = 0; s < 2; ++s)
        if (forced[2 * i + s] >= R && lab[forced[2 * i + s] - R] == kSplit) lab[i] = kSplit;
  }
  for (int64_t i = 0; i < M; ++i) labels[i] = lab[i];
  return GLIA_HMT_OK;
}

}  // namespace glia
