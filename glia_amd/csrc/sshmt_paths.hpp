// glia_amd/csrc/sshmt_paths.hpp -- the merge-path (unsupervised) term of train_sshmt_mlp / train_sshmt_logsig, stated
// ONCE for the host and the device on top of mlp_backward.hpp.
//
// Part 1 (host + device): one path.  A path of n <= kSshmtMaxPath merges has classifier outputs f_0 .. f_{n-1}; the monotonic DNF of
// alg/dnf.hxx:191-201,234-311 is D = 1 - prod_j F_j with F_j = T_n - c_j, c_j = prod_{i<j} f_i prod_{i>=j} (1 - f_i), j = 0 .. n, the
// residual e = t_n - D and a_i = dD/df_i (dnf.hxx:270-309).  Every product is a chain from 1.0 in ascending index order, the sum
// of a_i a chain from +0.0; mlp_mul / mlp_add / mlp_sub, nothing contracted.  T_n = mergeTarget^n and t_n = pathTarget^n come from two
// tables the host fills once with its own pow (input.hxx:36-39, dnf.hxx:199): the device never calls pow.
// Part 2 (host): merge_paths, the bounded genMergePaths of hmt/tree_build.hxx:150-180; the two-level reductions -- paths in chunks of
// kSshmtPathChunk consecutive paths for L_U = sum e_p^2, a row's coefficient c_r the chain of q = e_p a_{p,i} over the (path, slot)
// pairs that name it in ascending path order, rows in chunks of kMlpTrainChunk for grad_U = -sum_r c_r g_r -- and the host evaluator.
// The order IS the result.  No parity with Eigen's last bits is possible or claimed.  Host code: -ffp-contract=off.
#pragma once
#include "mlp_backward.hpp"

namespace glia {

constexpr int kSshmtMaxPath = 8;        // members of a path <= this: mergeTarget^n leaves the doubles long before a tree's depth
constexpr int kSshmtPathChunk = 64;     // paths of a chunk of L_U's reduction: part of the definition

struct SshmtTables {                    // [n], n = 1 .. kSshmtMaxPath; [0] unused
  double T[kSshmtMaxPath + 1], t[kSshmtMaxPath + 1];
};

// x_kj: column j of dnf.hxx:178-180's matrix, f_k left of the diagonal and 1 - f_k from the diagonal on
GLIA_MLP_HD double sshmt_x(const double* f, const double* u, int k, int j) { return k < j ? f[k] : u[k]; }

// One path: returns e = t_n - D; q [n] (or NULL) receives q_i = e * a_i.
GLIA_MLP_HD double sshmt_path(const double* f, int n, double Tn, double tn, double* q) {
  double u[kSshmtMaxPath], F[kSshmtMaxPath + 1];
  for (int i = 0; i < n; ++i) u[i] = mlp_sub(1.0, f[i]);
  double P = 1.0;
  for (int j = 0; j <= n; ++j) {
    double c = 1.0;
    for (int i = 0; i < n; ++i) c = mlp_mul(c, sshmt_x(f, u, i, j));
    F[j] = mlp_sub(Tn, c);
    P = mlp_mul(P, F[j]);
  }
  const double e = mlp_sub(tn, mlp_sub(1.0, P));
  if (!q) return e;
  double EC[kSshmtMaxPath + 1];
  for (int j = 0; j <= n; ++j) {
    double c = 1.0;
    for (int k = 0; k <= n; ++k) if (k != j) c = mlp_mul(c, F[k]);
    EC[j] = c;
  }
  for (int i = 0; i < n; ++i) {
    double a = 0.0;
    for (int j = 0; j <= n; ++j) {
      double m = 1.0;
      for (int k = 0; k < n; ++k) if (k != i) m = mlp_mul(m, sshmt_x(f, u, k, j));
      a = mlp_add(a, mlp_mul(EC[j], j <= i ? -m : m));      // dnf.hxx:306: the columns up to the diagonal change sign
    }
    q[i] = mlp_mul(e, a);
  }
  return e;
}

}  // namespace glia

// ---------------------------------------------------------------------------------------------------------------------------------
// host only from here
#include <unordered_map>
#include <unordered_set>

#include "dense_order.hpp"

namespace glia {

inline std::string sshmt_bad_lengths(int max_len, int min_len) {
  if (max_len < 0) return "merge_paths: max_path_length < 0 (paths of unbounded length) is not supported";
  if (max_len > kSshmtMaxPath) return "merge_paths: max_path_length above " + std::to_string(kSshmtMaxPath) + " is not supported";
  if (min_len < 1 || min_len > max_len) return "merge_paths: 1 <= min_path_length <= max_path_length does not hold";
  return std::string();
}

// order [n][3] = (key, key, created key), validated by dense_order over its own leaves (the operands no merge creates): an operand that
// is created later or was merged before, a created key seen before.  Returns the first bad merge or -1.
inline int64_t sshmt_check_order(const uint32_t* order, int64_t n) {
  std::unordered_set<uint32_t> created;
  for (int64_t i = 0; i < n; ++i) created.insert(order[3 * i + 2]);
  std::vector<uint32_t> leaves;
  for (int64_t i = 0; i < n; ++i)
    for (int s = 0; s < 2; ++s) if (!created.count(order[3 * i + s])) leaves.push_back(order[3 * i + s]);
  std::sort(leaves.begin(), leaves.end());
  leaves.erase(std::unique(leaves.begin(), leaves.end()), leaves.end());      // a leaf merged twice is an operand merged before
  std::vector<uint32_t> dense;
  const DenseOrderResult r = dense_order(leaves.data(), (int64_t)leaves.size(), order, n, &dense);
  return r.error == kDenseOrderOk ? -1 : r.merge;
}

// hmt/tree_build.hxx:150-180.  For every merge i ascending a path starts at i and follows the merge in which the current merge's
// created key is an operand, until it has max_len members or reaches a root; kept with exactly max_len members, or with at least
// min_len when neither operand of merge i is a created key.  CSR: offsets [P + 1], members (merge indices + row0), bottom-up.
inline void merge_paths(const uint32_t* order, int64_t n, int max_len, int min_len, int64_t row0, std::vector<int64_t>* offsets,
                        std::vector<int64_t>* members) {
  std::unordered_map<uint32_t, int64_t> child_of, created;
  child_of.reserve((size_t)n * 4); created.reserve((size_t)n * 2);
  for (int64_t i = 0; i < n; ++i) { child_of[order[3 * i]] = i; child_of[order[3 * i + 1]] = i; created[order[3 * i + 2]] = i; }
  if (offsets->empty()) offsets->push_back(0);
  int64_t path[kSshmtMaxPath];
  for (int64_t i = 0; i < n; ++i) {
    int len = 0;
    path[len++] = i;
    auto it = child_of.find(order[3 * i + 2]);
    while (it != child_of.end() && len < max_len) {
      path[len++] = it->second;
      it = child_of.find(order[3 * it->second + 2]);
    }
    if (len == max_len || (len >= min_len && !created.count(order[3 * i]) && !created.count(order[3 * i + 1]))) {
      for (int k = 0; k < len; ++k) members->push_back(path[k] + row0);
      offsets->push_back((int64_t)members->size());
    }
  }
}

// row -> the (path, slot) pairs that name it, as indices path * kSshmtMaxPath + slot into q, ascending (so: paths ascending)
inline void sshmt_incidence(const std::vector<int64_t>& offsets, const std::vector<int64_t>& members, int64_t n_rows,
                            std::vector<int64_t>* inc_off, std::vector<uint32_t>* inc) {
  const int64_t P = (int64_t)offsets.size() - 1;
  inc_off->assign((size_t)n_rows + 1, 0);
  for (int64_t r : members) (*inc_off)[(size_t)r + 1] += 1;
  for (int64_t r = 0; r < n_rows; ++r) (*inc_off)[(size_t)r + 1] += (*inc_off)[(size_t)r];
  inc->assign(members.size(), 0);
  std::vector<int64_t> fill(inc_off->begin(), inc_off->end() - 1);
  for (int64_t p = 0; p < P; ++p)
    for (int64_t k = offsets[p]; k < offsets[p + 1]; ++k)
      (*inc)[(size_t)fill[(size_t)members[k]]++] = (uint32_t)(p * kSshmtMaxPath + (k - offsets[p]));
}

inline void sshmt_fill_tables(double merge_target, double path_target, SshmtTables* tb) {
  tb->T[0] = tb->t[0] = 1.0;
  for (int n = 1; n <= kSshmtMaxPath; ++n) { tb->T[n] = std::pow(merge_target, n); tb->t[n] = std::pow(path_target, n); }
}

// what the evaluators share: the prepared unlabelled rows of all blocks, the paths, the incidence lists, the tables
struct SshmtInput {
  int D = 0;
  int64_t n_rows = 0;
  std::vector<double> X;                        // [n_rows][D]
  std::vector<int64_t> offsets{0}, members;     // paths
  std::vector<int64_t> inc_off;
  std::vector<uint32_t> inc;
  SshmtTables tb;
  int64_t n_paths() const { return (int64_t)offsets.size() - 1; }
};

// L_U = sum e_p^2 and, when grad != NULL, grad_U = -sum_r c_r g_r, by the orders above.
inline void sshmt_loss_grad_host(const double* w, int n1, int n2, const SshmtInput& in, double* L, double* grad) {
  const MlpWeights m = mlp_train_weights(w, in.D, n1, n2);
  const int64_t N = in.n_rows, P = in.n_paths();
  std::vector<double> f((size_t)N), e((size_t)P), q(grad ? (size_t)P * kSshmtMaxPath : 0), c(grad ? (size_t)N : 0);
  std::vector<uint8_t> named(grad ? (size_t)N : 0, 0);
  mlp_chunk_grad_host(m, in.X.data(), N, [&](int64_t r, double fr, double*) { f[(size_t)r] = fr; return false; }, nullptr);
  for (int64_t p = 0; p < P; ++p) {
    const int n = (int)(in.offsets[p + 1] - in.offsets[p]);
    double fp[kSshmtMaxPath];
    for (int i = 0; i < n; ++i) fp[i] = f[(size_t)in.members[in.offsets[p] + i]];
    e[(size_t)p] = sshmt_path(fp, n, in.tb.T[n], in.tb.t[n], grad ? &q[(size_t)p * kSshmtMaxPath] : nullptr);
  }
  *L = mlp_chunk_sqsum_host(e.data(), P, kSshmtPathChunk);
  if (!grad) return;
  for (int64_t r = 0; r < N; ++r) {
    double acc = 0.0;
    for (int64_t k = in.inc_off[r]; k < in.inc_off[r + 1]; ++k) {
      if (mlp_feq0(e[in.inc[k] / kSshmtMaxPath])) continue;      // dnf's caller skips the path (alg/function.hxx:195)
      acc = mlp_add(acc, q[in.inc[k]]);
      named[(size_t)r] = 1;
    }
    c[(size_t)r] = acc;
  }
  mlp_chunk_grad_host(m, in.X.data(), N, [&](int64_t r, double, double* cr) { *cr = c[(size_t)r]; return named[(size_t)r] != 0; }, grad);
}

struct SshmtHostEval : MlpTrainEval {
  int n1 = 0, n2 = 0;
  const SshmtInput* in = nullptr;
  int eval(const double* w, double* L, double* grad) override { sshmt_loss_grad_host(w, n1, n2, *in, L, grad); return 0; }
  // the batch's named rows in ascending order and its paths in batch order are an input of their own
  int batch_grad(const double* w, const MlpBatchView& b, double* grad) override {
    double L;
    if (!b.rows) return eval(w, &L, grad);
    SshmtInput sub;
    sub.D = in->D; sub.n_rows = b.n; sub.tb = in->tb;
    sub.X.resize((size_t)b.n * in->D);
    for (long long i = 0; i < b.n; ++i)
      std::copy(in->X.begin() + (size_t)b.rows[i] * in->D, in->X.begin() + (size_t)(b.rows[i] + 1) * in->D, sub.X.begin() + (size_t)i * in->D);
    sub.offsets.assign(b.offsets, b.offsets + b.P + 1);
    sub.members.assign(b.members, b.members + b.offsets[b.P]);
    sub.inc_off.assign(b.inc_off, b.inc_off + b.n + 1);
    sub.inc.assign(b.inc, b.inc + b.offsets[b.P]);
    sshmt_loss_grad_host(w, n1, n2, sub, &L, grad);
    return 0;
  }
};

// glia_hmt_sshmt_train_opts_default: main_train_sshmt_mlp.cxx:20-53
inline void sshmt_train_opts_default(glia_hmt_sshmt_train_opts* o) {
  mlp_train_opts_default(&o->base);
  o->sigma_u = 0.0; o->merge_target = 0.95; o->path_target = 1.0; o->max_path_length = 3; o->min_path_length = 2;
}
inline std::string sshmt_train_bad_opts(const glia_hmt_sshmt_train_opts& o) {
  const std::string bad = mlp_train_bad_opts(o.base, true);
  if (!bad.empty()) return bad;
  if (!std::isfinite(o.base.wu) || !std::isfinite(o.sigma_u) || !std::isfinite(o.merge_target) || !std::isfinite(o.path_target))
    return "sshmt_train: wu, sigma_u, merge_target or path_target is not finite";
  if (!mlp_isfeq(o.base.wu, 0.0) && o.sigma_u == 0.0 && !o.base.update_sigma_u)
    return "sshmt_train: sigma_u is 0 and update_sigma_u is off: the unsupervised term divides by sigma_u^2";
  return std::string();
}

}  // namespace glia
