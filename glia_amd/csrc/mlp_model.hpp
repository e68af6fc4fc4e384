// glia_amd/csrc/mlp_model.hpp -- the second boundary classifier on the host: alg::MLP2v / alg::EnsembleMLP2v (alg/nn.hxx:14-254: two
// ReLU hidden layers, a sigmoid output) and alg::Logsig (alg/function.hxx:33-34), as sshmt/main_pred_mlp.cxx and
// sshmt/main_pred_logsig.cxx apply them to feature rows.  This header holds the parser of the model and min/max files, the shape
// arithmetic, the layout the kernel takes (mlp_predict.hip) and a plain forward pass over rows, written with mlp_forward.hpp -- THE
// definition of the arithmetic, which the classifier loop shares:
// every sum starts at 0.0 and takes its terms in ascending index order, a multiply and an add rounded separately (no FMA).  Host-only
// and header-only: the library uses it (api_mlp.cpp, mlp_predict.hip) and cli/mlp_model_check.cpp builds it alone.
#pragma once
#include <stdint.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "mlp_forward.hpp"

namespace glia {

constexpr double kMlpFeps = 2.22e-16;      // FEPS of stats::rescale (util/stats.hxx:265-277, glia_base.hxx)
constexpr int kMlpMaxHidden = 256;         // N1, N2 <= this
constexpr int kMlpMaxDim = 65535;          // columns of a row <= this
constexpr int kMlpLoopMaxHidden = 32;      // N1, N2 <= this inside the classifier loop (greedy_bc.hip: per-thread arrays of the initial-edge kernel)
constexpr int kMlpSlots = 4;               // waves of a workgroup: they share a tile of rows and split a layer's units
constexpr int kMlpUnitBlock = 16;          // hidden units a thread accumulates in registers at a time, at most
constexpr int kMlpLdsBytes = 64 * 1024;    // tile budget of a workgroup

// One model, or three behind opt::ThresholdModelDistributor (type/function.hxx:80-84).  n1 == n2 == 0: the logsig model.
struct HostMlp {
  int n_models = 0, n1 = 0, n2 = 0;
  int D = 0;                               // columns of a row + 1 (the bias)
  std::vector<double> w[3];                // w0 (D x n1, column-major), w1 ((n1 + 1) x n2, column-major), w2 (n2 + 1); logsig: w (D)
  bool rescale = false;
  std::vector<double> mn, mx;              // [D - 1]
  int dim0 = 0, dim1 = 0;                  // indices into the rescaled, bias-appended vector: [0, D - 1]
  double threshold = 0.0;
};

// readData(w, file, true): every whitespace-separated double of the file.  Returns an empty string, or a message.  Values are read
// with strtod, as the tools read feature rows (cli/text_io.hpp): wider than the reference's stream extraction, which refuses "nan",
// "inf", "nan(...)" and hexadecimal floats -- a file the reference reads is read the same here, a file with such values is read too.
inline std::string mlp_read_doubles(const char* path, std::vector<double>* out) {
  out->clear();
  FILE* f = fopen(path, "rb");
  if (!f) return std::string("Error: cannot open file ") + path;
  std::string text;
  char buf[1 << 16];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, got);
  fclose(f);
  const char* p = text.c_str();
  const char* const end = p + text.size();
  for (;;) {
    while (p < end && (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r' || *p == '\f' || *p == '\v')) ++p;
    if (p >= end) break;
    char* q = nullptr;
    const double v = strtod(p, &q);
    if (q == p) return std::string("Error: invalid value in data file ") + path;
    out->push_back(v);
    p = q;
  }
  return std::string();
}

// The min/max file of --fmm: two rows, minima then maxima (readData of a matrix: one row per line, blank lines skipped).
inline std::string mlp_read_minmax(const char* path, std::vector<double>* mn, std::vector<double>* mx) {
  mn->clear(); mx->clear();
  FILE* f = fopen(path, "rb");
  if (!f) return std::string("Error: cannot open file ") + path;
  std::string text;
  char buf[1 << 16];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, got);
  fclose(f);
  int row = 0;
  size_t pos = 0;
  while (pos < text.size() && row < 2) {
    size_t eol = text.find('\n', pos);
    if (eol == std::string::npos) eol = text.size();
    const std::string line = text.substr(pos, eol - pos);
    pos = eol + 1;
    std::vector<double>* dst = row == 0 ? mn : mx;
    const char* p = line.c_str();
    for (;;) {
      char* q = nullptr;
      const double v = strtod(p, &q);
      if (q == p) break;
      dst->push_back(v);
      p = q;
    }
    while (*p == ' ' || *p == '\t' || *p == '\r') ++p;
    if (*p) return std::string("Error: invalid value in data file ") + path;
    if (!dst->empty()) ++row;
  }
  if (row < 2) return std::string("mlp: the min/max file needs two rows, minima then maxima: ") + path;
  return std::string();
}

// MLP2::initialize(isWholeD = true) (alg/nn.hxx:28-35) without its silent truncation: D from the number of weights W.  Returns an
// empty string, or the message the shape is refused with; *beyond_limits (optional) tells whether the shape is a valid one that this
// library does not take (layers or rows beyond its limits: GLIA_HMT_ERR_UNSUPPORTED) rather than an invalid one (GLIA_HMT_ERR_ARG).
inline std::string mlp_shape(long long W, int n1, int n2, int* D, bool* beyond_limits = nullptr) {
  *D = 0;
  if (beyond_limits) *beyond_limits = false;
  if (n1 < 0 || n2 < 0 || (n1 == 0) != (n2 == 0)) return "mlp: hidden sizes must both be positive (or both 0: the logsig model)";
  if (n1 > kMlpMaxHidden || n2 > kMlpMaxHidden) {
    if (beyond_limits) *beyond_limits = true;
    return "mlp: more than " + std::to_string(kMlpMaxHidden) + " units in a hidden layer are not supported";
  }
  if (W <= 0) return "mlp: the model holds no weights";
  long long d = W;
  if (n1 > 0) {
    const long long rest = W - (long long)(n1 + 1) * n2 - n2 - 1;
    if (rest <= 0 || rest % n1) {
      return "mlp: " + std::to_string(W) + " weights do not fit hidden layers of " + std::to_string(n1) + " and " + std::to_string(n2) +
             " units (D * N1 + (N1 + 1) * N2 + N2 + 1 with a whole D)";
    }
    d = rest / n1;
  }
  if (d < 2) return "mlp: a model for rows of no columns (D < 2)";
  if (d - 1 > kMlpMaxDim) {
    if (beyond_limits) *beyond_limits = true;
    return "mlp: rows of more than " + std::to_string(kMlpMaxDim) + " columns are not supported";
  }
  *D = (int)d;
  return std::string();
}

// Whether the model is one the forward pass may run; an empty string, or a message.
inline std::string mlp_check(const HostMlp& m) {
  if (m.n_models != 1 && m.n_models != 3) return "mlp: one model, or three models with distributor arguments, expected";
  for (int i = 0; i < m.n_models; ++i) {
    int D = 0;
    const std::string bad = mlp_shape((long long)m.w[i].size(), m.n1, m.n2, &D);
    if (!bad.empty()) return bad;
    if (D != m.D) return "mlp: the models are for rows of different lengths";
  }
  if (m.rescale && (m.mn.size() < (size_t)(m.D - 1) || m.mx.size() < (size_t)(m.D - 1)))
    return "mlp: fewer min/max entries than columns (" + std::to_string(m.D - 1) + ")";
  if (m.n_models == 3 && (m.dim0 < 0 || m.dim1 < 0 || m.dim0 > m.D - 1 || m.dim1 > m.D - 1))
    return "mlp: distributor dimension outside [0, " + std::to_string(m.D - 1) + "]";
  return std::string();
}

inline double mlp_rescale(double x, double mn, double mx) { return mlp_rescale_den(x, mn, (mx - mn) + kMlpFeps); }
struct MlpRowPtr {         // a vector that is all there
  const double* p;
  double operator()(int j) const { return p[j]; }
};
inline int mlp_pick(const HostMlp& m, const double* x) {     // x: rescaled, bias appended
  return mlp_pick_of(m.n_models, m.dim0, m.dim1, m.threshold, MlpRowPtr{x});
}
inline double mlp_sigmoid(double h3) { return 1.0 / (1.0 + std::exp(-h3)); }
// model i as the forward pass takes it: the file's matrices, column-major
inline MlpWeights mlp_host_weights(const HostMlp& m, int i) {
  const double* w = m.w[i].data();
  MlpWeights v;
  v.D = m.D; v.n1 = m.n1; v.n2 = m.n2; v.ub1 = 1; v.ub2 = 1;
  v.w0 = w; v.w1 = w + (size_t)m.D * m.n1; v.w2 = m.n1 ? v.w1 + (size_t)(m.n1 + 1) * m.n2 : w;
  return v;
}

// The forward pass (mlp_forward.hpp): rows [n_rows][D - 1] at a stride of row_stride doubles; pred and logit may each be NULL.
inline void mlp_forward(const HostMlp& m, const double* rows, int64_t n_rows, int64_t row_stride, double* pred, double* logit) {
  const int D = m.D, dim = D - 1;
  std::vector<double> x((size_t)D), a1((size_t)m.n1 + 1), a2((size_t)m.n2 + 1);
  for (int64_t r = 0; r < n_rows; ++r) {
    const double* src = rows + r * row_stride;
    for (int j = 0; j < dim; ++j) x[j] = m.rescale ? mlp_rescale(src[j], m.mn[j], m.mx[j]) : src[j];
    x[dim] = 1.0;
    const double h3 = mlp_logit(mlp_host_weights(m, mlp_pick(m, x.data())), MlpRowPtr{x.data()}, a1.data(), a2.data());
    if (logit) logit[r] = h3;
    if (pred) pred[r] = mlp_sigmoid(h3);
  }
}

// ---- what the kernel takes (mlp_predict.hip) ----
// Units a wave accumulates at a time for a layer of n units: the waves of a workgroup split the layer evenly, up to kMlpUnitBlock each.
inline int mlp_unit_block(int n) {
  static const int sizes[] = {1, 2, 3, 4, 6, 8, 12, 16};
  const int want = (n + kMlpSlots - 1) / kMlpSlots;
  for (int s : sizes) if (s >= want) return s;
  return kMlpUnitBlock;
}
// A column-major din x n weight matrix in blocks of ub units: [block][j][ub], units beyond n are 0.0 (computed, never stored).
inline std::vector<double> mlp_block_weights(const double* w, int din, int n, int ub) {
  const int nb = (n + ub - 1) / ub;
  std::vector<double> out((size_t)nb * din * ub, 0.0);
  for (int k = 0; k < n; ++k)
    for (int j = 0; j < din; ++j) out[((size_t)(k / ub) * din + j) * ub + k % ub] = w[j + (size_t)din * k];
  return out;
}
// The tile of a workgroup: tile_rows rows (64, 32, 16 or 8), each `stride` doubles of LDS (odd); staged: the rescaled, bias-appended
// row lies there too, else it is read from global memory by every wave.  A row holds region A = the row, later the second layer's
// activations, and region B = the first layer's activations.  compact (both layers of at most kMlpSlots * kMlpUnitBlock units, so one
// block per slot): a slot holds its activations in registers across a barrier and they overwrite the layer's input -- one region.
// Rows are staged when 32 of them fit the budget.
struct MlpPlan { int staged = 0, compact = 0, tile_rows = 0, stride = 0, region_a = 0; };
inline MlpPlan mlp_plan(int dim, int n1, int n2) {
  const int D = dim + 1, cap = kMlpSlots * kMlpUnitBlock;
  MlpPlan p;
  p.compact = n1 > 0 && n1 <= cap && n2 <= cap;
  const int b = n1 && !p.compact ? n1 + 1 : 0;                               // region B
  const int a2 = !n1 ? 0 : (p.compact ? (n1 > n2 ? n1 : n2) + 1 : n2 + 1);   // what region A holds after the row
  const long long ss = (long long)((D > a2 ? D : a2) + b) | 1;
  if (ss * 32 * 8 <= kMlpLdsBytes) {
    p.staged = 1; p.stride = (int)ss; p.region_a = D > a2 ? D : a2;
    p.tile_rows = ss * 64 * 8 <= kMlpLdsBytes ? 64 : 32;
    return p;
  }
  p.stride = (a2 + b) | 1; p.region_a = a2;
  p.tile_rows = 64;
  while (p.tile_rows > 8 && (long long)p.stride * p.tile_rows * 8 > kMlpLdsBytes) p.tile_rows >>= 1;
  return p;
}
// the longest row that is staged under hidden layers of n1 and n2 units (0: none)
inline int mlp_stage_max_dim(int n1, int n2) {
  int lo = 0, hi = kMlpMaxDim;            // staged(dim) is monotone: true up to a limit
  while (lo < hi) {
    const int mid = lo + (hi - lo + 1) / 2;
    if (mlp_plan(mid, n1, n2).staged) lo = mid; else hi = mid - 1;
  }
  return lo;
}

}  // namespace glia
