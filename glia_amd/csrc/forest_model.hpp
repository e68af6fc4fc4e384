// glia_amd/csrc/forest_model.hpp -- a whole random-forest model on the host (every array of rf_old::Model that the GLIA model file
// holds, ml/rf/ml_rf.h:97-156), the one C++ writer of that file (rf_old::writeModelToBinaryFile, ml/rf/ml_rf_model.cxx:378-455) and
// the option arithmetic around rf_old::train (ml/rf/main_train_rf.cxx:40-61, ml/rf/ml_rf_train.cxx:362,376).  Host-only and
// header-only: the library uses it (forest_train.hip, forest.cpp, api_loops.cpp) and cli/forest_model_check.cpp builds it alone.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace glia {

// HostForest's fuller sibling.  Tree arrays are "node fastest within a tree" -- the memory layout after the reader's transposes
// (forest.cpp) and what synth_forest.py holds: 1-based daughters and variables, 0 at terminals; nodestatus 1 / -1; nodeclass 1-based at
// terminals.  Nodes beyond ndbigtree[t] are all zero.
struct ForestModel {
  int ntree = 0, nrnodes = 0, nclass = 0, mtry = 0;
  std::vector<double> xbestsplit;   // [ntree][nrnodes]
  std::vector<int> treemap;         // [ntree][nrnodes][2]
  std::vector<int> nodestatus, nodeclass, bestvar;   // [ntree][nrnodes]
  std::vector<int> ndbigtree;       // [ntree]
  std::vector<double> classwt, cutoff;               // [nclass]
  std::vector<int> orig_labels, new_labels;          // [nclass]
  // Optional: what the trainer learned on rows its trees did not see (the slots of ml/rf/ml_rf.h:131-156, shaped as
  // ml/rf/ml_rf_train.cxx:728-784 leaves them).  oob_rows == 0: none; importance.empty(): no importance.
  int64_t oob_rows = 0;             // N
  int oob_dim = 0;                  // D
  std::vector<int> outcl, oob_times;                 // [N]: 1-based class of the most out-of-bag votes (0: never out of bag), their number
  std::vector<int> counttr, votes;                   // [nclass][N] and the same counts as [N][nclass]
  std::vector<double> errtr;                         // [ntree][nclass + 1]: error over trees 0..t, all rows and per class
  std::vector<long long> err_wrong, err_seen;        // [ntree][nclass + 1]: the integers errtr divides (not in the file)
  std::vector<double> importance, importanceSD;      // [D][nclass + 2], [D][nclass + 1]
  bool has_oob() const { return oob_rows > 0 && !outcl.empty(); }
  bool has_importance() const { return oob_rows > 0 && !importance.empty(); }
};

struct TrainOptions {
  int ntree = 255, mtry = 0;
  double sample_ratio = 0.7;
  int nodesize = 1, balance = 1, max_depth = 0;
  uint64_t seed = 0x9E3779B97F4A7C15ull;
};

constexpr int kTrainMaxClasses = 8;

// What a training call derives from its inputs before any tree grows.
struct TrainPlan {
  int nclass = 0, mtry = 0;
  int64_t sampsize = 0;
  std::vector<int> orig_labels;          // ascending
  std::vector<long long> class_count;    // rows of each class
  std::vector<double> classwt;
  std::vector<uint8_t> cls;              // [n_rows] class index of every row
};

// Returns an empty string, or the message the call is refused with.
inline std::string train_plan(const double* x, int64_t n_rows, int dim, const int32_t* y, const TrainOptions& o, TrainPlan* p) {
  if (n_rows <= 0) return "Data X has 0 rows...";
  if (dim <= 0) return "forest_train: data X has 0 columns";
  if (n_rows >= (1ll << 28)) return "forest_train: more than 2^28 - 1 rows";
  if (dim > 32767) return "forest_train: more than 32767 columns";
  if (o.ntree < 1) return "forest_train: ntree < 1";
  if (o.nodesize < 1) return "forest_train: nodesize < 1";
  if (o.max_depth < 0) return "forest_train: max_depth < 0";
  if (!(o.sample_ratio == o.sample_ratio)) return "forest_train: sample_ratio is not a number";
  for (int64_t i = 0; i < n_rows * dim; ++i)
    if (!std::isfinite(x[i])) {
      char b[160];
      snprintf(b, sizeof(b), "forest_train: non-finite value in row %lld, column %lld", (long long)(i / dim), (long long)(i % dim));
      return b;
    }
  p->orig_labels.clear();
  for (int64_t i = 0; i < n_rows; ++i) {
    auto it = std::lower_bound(p->orig_labels.begin(), p->orig_labels.end(), y[i]);
    if (it != p->orig_labels.end() && *it == y[i]) continue;
    if ((int)p->orig_labels.size() == kTrainMaxClasses) return "forest_train: more than 8 classes";
    p->orig_labels.insert(it, y[i]);
  }
  p->nclass = (int)p->orig_labels.size();
  if (p->nclass < 2) return "Need at least two classes for classification...";
  p->cls.resize((size_t)n_rows);
  p->class_count.assign(p->nclass, 0);
  for (int64_t i = 0; i < n_rows; ++i) {
    const int k = (int)(std::lower_bound(p->orig_labels.begin(), p->orig_labels.end(), y[i]) - p->orig_labels.begin());
    p->cls[i] = (uint8_t)k;
    ++p->class_count[k];
  }
  // main_train_rf.cxx:46-60
  p->classwt.assign(p->nclass, 1.0);
  if (o.balance) {
    long long maxcnt = -1;
    for (long long c : p->class_count) maxcnt = std::max(maxcnt, c);
    for (int k = 0; k < p->nclass; ++k) p->classwt[k] = (double)maxcnt / (double)p->class_count[k];
  }
  // main_train_rf.cxx:40-44 (FEPS = 1e-6); without the option classRF samples N rows
  if (o.sample_ratio > 1e-6) {
    const double s = (double)(float)n_rows * o.sample_ratio + 0.5;
    if (!(s >= 1.0) || s >= (double)n_rows + 1.0) return "forest_train: the sample size is outside [1, rows]";
    p->sampsize = (int64_t)(int)s;
  } else p->sampsize = n_rows;
  if (p->sampsize < 1 || p->sampsize > n_rows) return "forest_train: the sample size is outside [1, rows]";
  // ml_rf_train.cxx:362,376
  int mtry = o.mtry;
  if (mtry <= 0 || mtry > dim) mtry = (int)std::floor(std::sqrt((double)dim));
  p->mtry = std::max(1, std::min(dim, mtry));
  return std::string();
}

namespace model_file {
constexpr size_t kHeaderBytes = 520;
// offsets of the int n[2] pairs / scalars inside the struct dump (x86-64, libstdc++; forest.cpp reads the same ones)
constexpr size_t O_NRNODES = 128, O_NTREE = 132, O_N_XBEST = 144, O_N_CLASSWT = 160, O_N_CUTOFF = 176, O_N_TREEMAP = 192,
                 O_N_NODESTATUS = 208, O_N_NODECLASS = 224, O_N_BESTVAR = 240, O_N_NDBIGTREE = 256, O_MTRY = 264, O_N_ORIG = 280,
                 O_N_NEW = 296, O_NCLASS = 304, O_N_OUTCL = 320, O_N_COUNTTR = 352, O_N_IMPORTANCE = 416, O_N_IMPORTANCESD = 432,
                 O_N_ERRTR = 448, O_N_VOTES = 496, O_N_OOB_TIMES = 512;
// writeArray (ml_rf_model.cxx:20-46) for an array kept dense: a flag byte in front of arrays longer than 128 elements
template <typename T> bool array(FILE* f, const T* a, size_t n) {
  if (n == 0) return true;
  if (n > 128) { const unsigned char dense = 0; if (fwrite(&dense, 1, 1, f) != 1) return false; }
  return fwrite(a, sizeof(T), n, f) == n;
}
// memory (node fastest: n1 runs of n0) -> file (row-major n0 x n1); undone by the reader's transpose
template <typename T> std::vector<T> filemat(const std::vector<T>& mem, size_t n0, size_t n1) {
  std::vector<T> r(n0 * n1);
  for (size_t c = 0; c < n1; ++c)
    for (size_t k = 0; k < n0; ++k) r[k * n1 + c] = mem[c * n0 + k];
  return r;
}
}  // namespace model_file

inline std::string model_check(const ForestModel& m) {
  const size_t nn = (size_t)m.ntree * (size_t)m.nrnodes;
  if (m.ntree < 1 || m.nrnodes < 1 || m.nclass < 1) return "forest_model: empty model";
  if (m.xbestsplit.size() != nn || m.treemap.size() != 2 * nn || m.nodestatus.size() != nn || m.nodeclass.size() != nn ||
      m.bestvar.size() != nn || m.ndbigtree.size() != (size_t)m.ntree || m.classwt.size() != (size_t)m.nclass ||
      m.cutoff.size() != (size_t)m.nclass || m.orig_labels.size() != (size_t)m.nclass || m.new_labels.size() != (size_t)m.nclass)
    return "forest_model: inconsistent array sizes";
  const size_t N = (size_t)m.oob_rows, nc = (size_t)m.nclass, D = (size_t)m.oob_dim;
  if (m.oob_rows < 0 || m.oob_rows >= (1ll << 28) || m.oob_dim < 0) return "forest_model: inconsistent out-of-bag sizes";
  if (m.has_oob() && (m.outcl.size() != N || m.oob_times.size() != N || m.counttr.size() != nc * N || m.votes.size() != nc * N ||
                      m.errtr.size() != (size_t)m.ntree * (nc + 1)))
    return "forest_model: inconsistent out-of-bag array sizes";
  if (!m.has_oob() && !(m.outcl.empty() && m.oob_times.empty() && m.counttr.empty() && m.votes.empty() && m.errtr.empty()))
    return "forest_model: inconsistent out-of-bag array sizes";
  if (!m.importance.empty() && (m.oob_rows <= 0 || D == 0 || m.importance.size() != D * (nc + 2) || m.importanceSD.size() != D * (nc + 1)))
    return "forest_model: inconsistent importance array sizes";
  if (m.importance.empty() && !m.importanceSD.empty()) return "forest_model: inconsistent importance array sizes";
  return std::string();
}

// Returns an empty string, or a message.
inline std::string write_forest_model(const ForestModel& m, const char* path) {
  using namespace model_file;
  const std::string bad = model_check(m);
  if (!bad.empty()) return bad;
  unsigned char hdr[kHeaderBytes];
  memset(hdr, 0, sizeof(hdr));
  auto n2 = [&](size_t off, int a, int b) { memcpy(hdr + off, &a, 4); memcpy(hdr + off + 4, &b, 4); };
  auto n1 = [&](size_t off, int a) { memcpy(hdr + off, &a, 4); };
  n2(O_N_XBEST, m.nrnodes, m.ntree); n2(O_N_CLASSWT, m.nclass, 1); n2(O_N_CUTOFF, m.nclass, 1);
  n2(O_N_TREEMAP, m.nrnodes, 2 * m.ntree); n2(O_N_NODESTATUS, m.nrnodes, m.ntree); n2(O_N_NODECLASS, m.nrnodes, m.ntree);
  n2(O_N_BESTVAR, m.nrnodes, m.ntree); n2(O_N_NDBIGTREE, m.ntree, 1); n2(O_N_ORIG, m.nclass, 1); n2(O_N_NEW, m.nclass, 1);
  n1(O_NRNODES, m.nrnodes); n1(O_NTREE, m.ntree); n1(O_MTRY, m.mtry); n1(O_NCLASS, m.nclass);
  // the out-of-bag slots, n[2] as ml_rf_train.cxx:728-784 sets them: a transposed array is {columns, rows} of classRF's, errtr and votes
  // keep {rows, columns}; the slots between them (outclts, proximities, localImp, errts, inbag) stay empty
  const int N = (int)m.oob_rows;
  if (m.has_oob()) {
    n2(O_N_OUTCL, N, 1); n2(O_N_COUNTTR, m.nclass, N); n2(O_N_ERRTR, m.ntree, m.nclass + 1); n2(O_N_VOTES, N, m.nclass); n2(O_N_OOB_TIMES, N, 1);
  }
  if (m.has_importance()) { n2(O_N_IMPORTANCE, m.oob_dim, m.nclass + 2); n2(O_N_IMPORTANCESD, m.oob_dim, m.nclass + 1); }
  FILE* f = fopen(path, "wb");
  if (!f) return std::string("Error: cannot create file ") + path;
  const size_t n0 = (size_t)m.nrnodes, nt = (size_t)m.ntree, nn = n0 * nt;
  bool ok = fwrite(hdr, 1, sizeof(hdr), f) == sizeof(hdr);
  ok = ok && fwrite(&m.nrnodes, 4, 1, f) == 1 && fwrite(&m.ntree, 4, 1, f) == 1;
  ok = ok && array(f, filemat(m.xbestsplit, n0, nt).data(), nn);
  ok = ok && array(f, m.classwt.data(), m.classwt.size()) && array(f, m.cutoff.data(), m.cutoff.size());
  ok = ok && array(f, filemat(m.treemap, n0, 2 * nt).data(), 2 * nn);
  ok = ok && array(f, filemat(m.nodestatus, n0, nt).data(), nn);
  ok = ok && array(f, filemat(m.nodeclass, n0, nt).data(), nn);
  ok = ok && array(f, filemat(m.bestvar, n0, nt).data(), nn);
  ok = ok && array(f, m.ndbigtree.data(), nt);
  ok = ok && fwrite(&m.mtry, 4, 1, f) == 1;
  ok = ok && array(f, m.orig_labels.data(), m.orig_labels.size()) && array(f, m.new_labels.data(), m.new_labels.size());
  ok = ok && fwrite(&m.nclass, 4, 1, f) == 1;
  if (m.has_oob()) ok = ok && array(f, m.outcl.data(), m.outcl.size()) && array(f, m.counttr.data(), m.counttr.size());      // ml_rf_model.cxx:428-432
  if (m.has_importance()) ok = ok && array(f, m.importance.data(), m.importance.size()) && array(f, m.importanceSD.data(), m.importanceSD.size());   // :439-442
  if (m.has_oob()) ok = ok && array(f, m.errtr.data(), m.errtr.size()) && array(f, m.votes.data(), m.votes.size()) &&       // :443-448
                        array(f, m.oob_times.data(), m.oob_times.size());
  ok = (fclose(f) == 0) && ok;
  return ok ? std::string() : std::string("Error: cannot write file ") + path;
}

}  // namespace glia
