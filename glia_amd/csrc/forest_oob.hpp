// glia_amd/csrc/forest_oob.hpp -- the host half of the out-of-bag outputs of a training call: everything that is a
// double.  The device (forest_oob.hip) hands over integers only -- votes, (wrong, seen) pairs, changed predictions d_k, out-of-bag rows
// per class n_k, in-bag class counts of the leaves -- and every division, sum and square root below is one IEEE operation in a stated
// order, so tests/_rfoobdef.py can be held to it bit for bit.  These are classRF's outputs errtr, outcl, counttr, votes, oob_times,
// importance and importanceSD (ml/rf/ml_rf_train.cxx:112-159,728-784).  Host-only and header-only: cli/forest_oob_check.cpp builds
// it alone.
#pragma once
#include "forest_model.hpp"

namespace glia {

struct OobOptions {
  int oob = 0, importance = 0;
};

inline double oob_ratio(long long num, long long den) { return den == 0 ? 0.0 : (double)num / (double)den; }

// outcl, oob_times, votes from counttr [nclass][N]: the most votes, ties to the lowest class; 0 where a row was never out of bag
inline void oob_votes(const std::vector<int>& counttr, int nclass, int64_t N, std::vector<int>* outcl, std::vector<int>* oob_times, std::vector<int>* votes) {
  outcl->assign((size_t)N, 0); oob_times->assign((size_t)N, 0); votes->assign((size_t)N * nclass, 0);
  for (int64_t i = 0; i < N; ++i) {
    int best = 0, sum = 0;
    for (int k = 0; k < nclass; ++k) {
      const int c = counttr[(size_t)k * N + i];
      (*votes)[(size_t)i * nclass + k] = c;
      sum += c;
      if (c > counttr[(size_t)best * N + i]) best = k;
    }
    (*oob_times)[i] = sum;
    (*outcl)[i] = sum ? best + 1 : 0;
  }
}

// errtr [ntree][nclass + 1] from the per-class pairs of every tree (pairs[(t * nclass + k) * 2] = wrong, + 1 = seen): column 0 is all rows
inline void oob_errtr(const std::vector<long long>& pairs, int ntree, int nclass, std::vector<double>* errtr, std::vector<long long>* wrong,
                      std::vector<long long>* seen) {
  const size_t w = (size_t)nclass + 1;
  errtr->assign((size_t)ntree * w, 0.0); wrong->assign((size_t)ntree * w, 0); seen->assign((size_t)ntree * w, 0);
  for (int t = 0; t < ntree; ++t) {
    long long aw = 0, as = 0;
    for (int k = 0; k < nclass; ++k) {
      const long long kw = pairs[((size_t)t * nclass + k) * 2], ks = pairs[((size_t)t * nclass + k) * 2 + 1];
      (*wrong)[t * w + 1 + k] = kw; (*seen)[t * w + 1 + k] = ks;
      aw += kw; as += ks;
    }
    (*wrong)[t * w] = aw; (*seen)[t * w] = as;
    for (size_t c = 0; c < w; ++c) (*errtr)[t * w + c] = oob_ratio((*wrong)[t * w + c], (*seen)[t * w + c]);
  }
}

// The sums of a forest's importance, tree by tree in ascending order.
struct ImportanceSums {
  int D = 0, nclass = 0;
  std::vector<double> sum, sq;       // [D][nclass + 1]: terms and their squares (column nclass: all classes)
  std::vector<double> gini;          // [D]
  void init(int dim, int classes) {
    D = dim; nclass = classes;
    sum.assign((size_t)D * (nclass + 1), 0.0); sq = sum; gini.assign((size_t)D, 0.0);
  }
  // one tree: d [D][nclass] changed predictions (r_k - r'_k), n_k [nclass] its out-of-bag rows of every class
  void add_tree(const int* d, const long long* n_k) {
    long long m = 0;
    for (int k = 0; k < nclass; ++k) m += n_k[k];
    if (m == 0) return;
    for (int v = 0; v < D; ++v) {
      long long all = 0;
      for (int k = 0; k <= nclass; ++k) {
        const long long num = k < nclass ? (long long)d[(size_t)v * nclass + k] : all, den = k < nclass ? n_k[k] : m;
        if (k < nclass) all += num;
        const double term = oob_ratio(num, den);
        const double term2 = term * term;
        double& s = sum[(size_t)v * (nclass + 1) + k];
        double& q = sq[(size_t)v * (nclass + 1) + k];
        s = s + term; q = q + term2;
      }
    }
  }
  // G of a node's in-bag class counts, in the arithmetic of crit
  static double gini_of(const double* w, const long long* n, int nclass) {
    double num = 0.0, den = 0.0;
    for (int k = 0; k < nclass; ++k) {
      const double t = w[k] * (double)n[k];
      const double t2 = t * t;
      num = num + t2; den = den + t;
    }
    return num / den;
  }
  // one tree: left [nodes] (1-based left daughter, 0 at terminals), var [nodes] (1-based), cnt [nodes][nclass] in-bag counts of the
  // TERMINAL nodes (the others are filled here: daughters come after their mother in level order)
  void add_tree_gini(const int* left, const int* var, size_t nodes, std::vector<long long>* cnt, const double* w) {
    std::vector<long long>& c = *cnt;
    for (size_t q = nodes; q-- > 0;)
      if (left[q])
        for (int k = 0; k < nclass; ++k) c[q * nclass + k] = c[(size_t)(left[q] - 1) * nclass + k] + c[(size_t)left[q] * nclass + k];
    for (size_t q = 0; q < nodes; ++q)
      if (left[q]) {
        const double gl = gini_of(w, &c[(size_t)(left[q] - 1) * nclass], nclass), gr = gini_of(w, &c[(size_t)left[q] * nclass], nclass);
        const double both = gl + gr;
        const double dec = both - gini_of(w, &c[q * nclass], nclass);
        gini[(size_t)(var[q] - 1)] = gini[(size_t)(var[q] - 1)] + dec;
      }
  }
  // importance [D][nclass + 2] and importanceSD [D][nclass + 1]
  void finish(int ntree, std::vector<double>* importance, std::vector<double>* sd) const {
    const double nt = (double)ntree;
    importance->assign((size_t)D * (nclass + 2), 0.0); sd->assign((size_t)D * (nclass + 1), 0.0);
    for (int v = 0; v < D; ++v) {
      for (int c = 0; c <= nclass; ++c) {
        const double mean = sum[(size_t)v * (nclass + 1) + c] / nt;
        const double msq = sq[(size_t)v * (nclass + 1) + c] / nt;
        const double mean2 = mean * mean;
        const double var = (msq - mean2) / nt;
        (*importance)[(size_t)v * (nclass + 2) + c] = mean;
        (*sd)[(size_t)v * (nclass + 1) + c] = std::sqrt(var > 0.0 ? var : 0.0);
      }
      (*importance)[(size_t)v * (nclass + 2) + nclass + 1] = gini[v] / nt;
    }
  }
};

// b of the permutation: the smallest even number of bits >= 2 with 2^b >= m
inline int oob_perm_bits(uint64_t m) {
  int b = 2;
  while ((1ull << b) < m) b += 2;
  return b;
}

}  // namespace glia
