// glia_amd/csrc/mlp_backward.hpp -- training the MLP / logsig boundary classifier: the supervised part of
// train_sshmt_mlp / train_sshmt_logsig (sshmt/main_train_sshmt_mlp.cxx:96-168), stated ONCE for the host and the device.
//
// Part 1 (host + device): the backward pass of one row (alg/nn.hxx:73-107, alg/function.hxx:36-40) as elementwise IEEE operations on
// top of mlp_forward.hpp -- the same mlp_mul / mlp_add, nothing contracted into an FMA, every chain from +0.0 in ascending order.
// Part 2 (host): the reduction over rows -- chunks of kMlpTrainChunk consecutive rows, chunk sums in row order, the gradient the sum
// of the chunk sums in chunk order; the order IS the result -- and the trainer: energy (type/energy_function.hxx:164-230), the three
// updates and two step rules of alg/gd.hxx, the sigma rule and outer loop of sshmt_util.hxx:140-207.  The trainer asks an evaluator for
// L = sum e_i^2 and grad = -sum g_i e_i; the host evaluator is below, the device's is mlp_train.hip.  Everything else of an iteration
// runs in this one place, on the host, whichever evaluator is used.
//
// No parity with the reference's last bits is possible or claimed: Eigen's summation order, Boost's Gaussian and the OpenMP per-thread
// partial sums (alg/function.hxx:185-198) are not reproducible.  Host code must be built with -ffp-contract=off.
#pragma once
#include <stdint.h>

#include "mlp_forward.hpp"

namespace glia {

constexpr int kMlpTrainChunk = 64;          // rows of a chunk: part of the definition, not of the launch
constexpr int kMlpTrainMaxHidden = 32;      // N1, N2 <= this (the classifier loop's limit, kMlpLoopMaxHidden)
constexpr int kMlpTrainMaxDim = 384;        // columns of a row <= this (kMaxFeat)
constexpr double kMlpTrainFeps = 2.22e-16;  // FEPS of isfeq (glia_base.hxx:57,71)

GLIA_MLP_HD double mlp_sub(double a, double b) {
#ifdef __HIP_DEVICE_COMPILE__
  return __dsub_rn(a, b);
#else
  return a - b;
#endif
}
// isfeq(e, 0.0): a row whose residual is this small adds nothing to the gradient (alg/function.hxx:195); a NaN is not small
GLIA_MLP_HD bool mlp_feq0(double e) { return __builtin_fabs(e) < kMlpTrainFeps; }

// The weights of one model in the file's layout (column-major matrices, one after the other); logsig: w2 = the D weights.
GLIA_MLP_HD MlpWeights mlp_train_weights(const double* w, int D, int n1, int n2) {
  MlpWeights v;
  v.D = D; v.n1 = n1; v.n2 = n2; v.ub1 = 1; v.ub2 = 1;
  v.w0 = w; v.w1 = w + (size_t)D * (size_t)n1; v.w2 = n1 ? v.w1 + (size_t)(n1 + 1) * (size_t)n2 : w;
  return v;
}
GLIA_MLP_HD long long mlp_train_n_weights(int D, int n1, int n2) {
  return n1 ? (long long)D * n1 + (long long)(n1 + 1) * n2 + n2 + 1 : D;
}

// Pre-activations h[0 .. n) at a stride of s doubles, seen as the next layer's input: relu(h[j]), then the bias 1.0.
struct MlpActs {
  const double* h;
  int n, s;
  GLIA_MLP_HD double operator()(int j) const { return j < n ? mlp_relu(h[(size_t)j * (size_t)s]) : 1.0; }
};
struct MlpRow {      // a prepared row: rescaled, the 1.0 appended
  const double* p;
  GLIA_MLP_HD double operator()(int j) const { return p[j]; }
};

// nn.hxx:96: dh3 = f * (1 - f)
GLIA_MLP_HD double mlp_dh3(double f) { return mlp_mul(f, mlp_sub(1.0, f)); }
// nn.hxx:98-100: dh2[k] = dh3 * w2[k], +0.0 where the unit is dead (h2[k] <= 0.0; a NaN is not dead)
GLIA_MLP_HD double mlp_dh2(const MlpWeights& m, int k, double h2k, double dh3) { return h2k <= 0.0 ? 0.0 : mlp_mul(dh3, m.w2[k]); }
// nn.hxx:102-104: dh1[j] = sum_k dh2[k] * w1[j, k], k ascending from +0.0; +0.0 where h1[j] <= 0.0.  dh2 at a stride of s doubles.
GLIA_MLP_HD double mlp_dh1(const MlpWeights& m, int j, double h1j, const double* dh2, int s) {
  double acc = 0.0;
  for (int k = 0; k < m.n2; ++k) acc = mlp_add(acc, mlp_mul(dh2[(size_t)k * (size_t)s], m.w1[(size_t)j + (size_t)(m.n1 + 1) * (size_t)k]));
  return h1j <= 0.0 ? 0.0 : acc;
}
// Element p of the row's gradient g_i (nn.hxx:97,101,105; function.hxx:38): one product.  h1, h2, dh1, dh2 at a stride of s doubles.
template <class X> GLIA_MLP_HD double mlp_grad_elem(const MlpWeights& m, long long p, const X& x, const double* h1, const double* h2,
                                                    const double* dh1, const double* dh2, double dh3, int s) {
  if (m.n1 == 0) return mlp_mul(dh3, x((int)p));
  const long long o1 = (long long)m.D * m.n1, o2 = o1 + (long long)(m.n1 + 1) * m.n2;
  if (p < o1) return mlp_mul(x((int)(p % m.D)), dh1[(size_t)(p / m.D) * (size_t)s]);
  if (p < o2) {
    const long long q = p - o1;
    return mlp_mul(MlpActs{h1, m.n1, s}((int)(q % (m.n1 + 1))), dh2[(size_t)(q / (m.n1 + 1)) * (size_t)s]);
  }
  return mlp_mul(MlpActs{h2, m.n2, s}((int)(p - o2)), dh3);
}

// The splitmix64 finaliser (the same function as forest_train.hpp's rf_mix, restated so that host-only programs can include this header).
GLIA_MLP_HD uint64_t mlp_mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// Initial weight p of an MLP: Gaussian(0, 0.01) by Irwin-Hall -- twelve uniforms u_k = (mix(h ^ (k + 1)) >> 11) * 2^-53 with
// h = mix(mix(seed) ^ p), summed from +0.0 for k ascending; w = (sum - 6.0) * 0.01.  Exact conversions and IEEE adds only: no libm.
GLIA_MLP_HD double mlp_init_weight(uint64_t seed, uint64_t p) {
  const uint64_t h = mlp_mix(mlp_mix(seed) ^ p);
  double s = 0.0;
  for (uint64_t k = 0; k < 12; ++k) s = mlp_add(s, mlp_mul((double)(mlp_mix(h ^ (k + 1)) >> 11), 0x1p-53));
  return mlp_mul(mlp_sub(s, 6.0), 0.01);
}

// The correctly rounded quotient and square root (the host's / and std::sqrt).
GLIA_MLP_HD double mlp_div(double a, double b) {
#ifdef __HIP_DEVICE_COMPILE__
  return __ddiv_rn(a, b);
#else
  return a / b;
#endif
}
GLIA_MLP_HD double mlp_sqrt(double a) {
#ifdef __HIP_DEVICE_COMPILE__
  return __dsqrt_rn(a);
#else
  return __builtin_sqrt(a);
#endif
}
// How the terms' gradients become g and how g moves a weight, per weight: stated once for the trainer's full-data iteration and for the
// batch steps of DESIGN 3.17, on the host and in k_batch_step (mlp_batch.hip).  *_one: isfeq(weight, 1.0), the reference's shortcut.
struct MlpStepRule {
  int optimizer, use_r, use_u, use_s, r_one, u_one, s_one;
  double wr, wu, ws, sigma_u2, sigma2;
};
constexpr double kMlpMomentum = 0.5, kMlpAdamBeta1 = 0.5, kMlpAdamBeta2 = 0.9, kMlpAdamEps = 1e-8;      // alg/gd.hxx:289,347-349
// type/energy_function.hxx:164-230: from +0.0 the regulariser, the unsupervised term, the supervised term
GLIA_MLP_HD double mlp_energy_grad_elem(const MlpStepRule& k, double w, double gu, double gs) {
  double g = 0.0;
  if (k.use_r) g = mlp_add(g, k.r_one ? w : mlp_mul(k.wr, w));
  if (k.use_u) { const double t = mlp_div(gu, k.sigma_u2); g = mlp_add(g, k.u_one ? t : mlp_mul(k.wu, t)); }
  if (k.use_s) { const double t = mlp_div(gs, k.sigma2); g = mlp_add(g, k.s_one ? t : mlp_mul(k.ws, t)); }
  return g;
}
// alg/gd.hxx:73-79 (1: vanilla), 367-384 (2: Adam), 307-315 (3: momentum)
GLIA_MLP_HD void mlp_update_elem(int optimizer, double step, double g, double* w, double* om, double* ov) {
  if (optimizer == 1) *w = mlp_sub(*w, mlp_mul(g, step));
  else if (optimizer == 3) { const double u = mlp_add(g, mlp_mul(kMlpMomentum, *ov)); *w = mlp_sub(*w, mlp_mul(step, u)); *ov = u; }
  else {
    const double b1c = mlp_sub(1.0, kMlpAdamBeta1), b2c = mlp_sub(1.0, kMlpAdamBeta2);
    *om = mlp_add(mlp_mul(kMlpAdamBeta1, *om), mlp_mul(b1c, g));
    *ov = mlp_add(mlp_mul(kMlpAdamBeta2, *ov), mlp_mul(mlp_mul(b2c, g), g));
    *w = mlp_sub(*w, mlp_div(mlp_mul(step, *om), mlp_sqrt(mlp_add(*ov, kMlpAdamEps))));
  }
}

}  // namespace glia

// ---------------------------------------------------------------------------------------------------------------------------------
// host only from here
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/glia_hmt.h"

namespace glia {

inline double mlp_train_sigmoid(double h3) { return 1.0 / (1.0 + std::exp(-h3)); }      // the host's exp (mlp_model.hpp: mlp_sigmoid)

// The forward pass of one prepared row x [D]: the pre-activations to a [n1] and b [n2] (logsig: untouched); returns f by the host's sigmoid.
inline double mlp_forward_row_host(const MlpWeights& m, const double* x, double* a, double* b) {
  double h3;
  if (m.n1 == 0) h3 = mlp_unit(m.w2, m.D, 1, 0, MlpRow{x});
  else {
    for (int k = 0; k < m.n1; ++k) a[k] = mlp_unit(m.w0, m.D, 1, k, MlpRow{x});
    for (int k = 0; k < m.n2; ++k) b[k] = mlp_unit(m.w1, m.n1 + 1, 1, k, MlpActs{a, m.n1, 1});
    h3 = mlp_unit(m.w2, m.n2 + 1, 1, 0, MlpActs{b, m.n2, 1});
  }
  return mlp_train_sigmoid(h3);
}

// The reduction both terms of the energy end in, by the two-level order: grad = -sum_r c_r g_r over prepared rows X [n][D].  Every
// row r ascending runs the forward pass and asks term(r, f_r, &c_r) for its coefficient; false: the row is skipped.  grad == NULL:
// the forward pass and the term's questions alone.
template <class Term>
inline void mlp_chunk_grad_host(const MlpWeights& m, const double* X, int64_t n, Term term, double* grad) {
  const int C = kMlpTrainChunk, D = m.D, n1 = m.n1, n2 = m.n2;
  const long long d = mlp_train_n_weights(D, n1, n2);
  std::vector<double> h1((size_t)C * (n1 + 1)), h2((size_t)C * (n2 + 1)), dh1((size_t)C * (n1 + 1)), dh2((size_t)C * (n2 + 1)), dh3(C), c(C);
  std::vector<uint8_t> used(C);
  if (grad) for (long long p = 0; p < d; ++p) grad[p] = 0.0;
  for (int64_t r0 = 0; r0 < n; r0 += C) {
    const int nr = (int)(n - r0 < C ? n - r0 : C);
    for (int r = 0; r < nr; ++r) {
      double *a = &h1[(size_t)r * (n1 + 1)], *b = &h2[(size_t)r * (n2 + 1)];
      const double f = mlp_forward_row_host(m, X + (size_t)(r0 + r) * D, a, b);
      used[r] = term(r0 + r, f, &c[r]) && grad;
      if (!used[r]) continue;
      dh3[r] = mlp_dh3(f);
      double *da = &dh1[(size_t)r * (n1 + 1)], *db = &dh2[(size_t)r * (n2 + 1)];
      for (int k = 0; k < n2; ++k) db[k] = mlp_dh2(m, k, b[k], dh3[r]);
      for (int j = 0; j < n1; ++j) da[j] = mlp_dh1(m, j, a[j], db, 1);
    }
    if (!grad) continue;
    for (long long p = 0; p < d; ++p) {
      double S = 0.0;
      for (int r = 0; r < nr; ++r) {
        if (!used[r]) continue;
        const double g = mlp_grad_elem(m, p, MlpRow{X + (size_t)(r0 + r) * D}, &h1[(size_t)r * (n1 + 1)], &h2[(size_t)r * (n2 + 1)],
                                       &dh1[(size_t)r * (n1 + 1)], &dh2[(size_t)r * (n2 + 1)], dh3[r], 1);
        S = mlp_sub(S, mlp_mul(g, c[r]));
      }
      grad[p] = mlp_add(grad[p], S);
    }
  }
}

// sum v_i^2 over chunks of `chunk` consecutive entries: the chunk sums from +0.0 in order, their sum from +0.0 in chunk order
inline double mlp_chunk_sqsum_host(const double* v, int64_t n, int chunk) {
  double L = 0.0;
  for (int64_t i0 = 0; i0 < n; i0 += chunk) {
    double Lc = 0.0;
    for (int64_t i = i0; i < n && i < i0 + chunk; ++i) Lc = mlp_add(Lc, mlp_mul(v[i], v[i]));
    L = mlp_add(L, Lc);
  }
  return L;
}

// The supervised term: c_r = e_r = t_r - f_r, a row with |e_r| < FEPS skipped; L = sum e_r^2 by row chunks.  grad == NULL: L alone.
inline void mlp_loss_grad_host(const double* w, int D, int n1, int n2, const double* X, const double* t, int64_t n, double* L, double* grad) {
  std::vector<double> e((size_t)n);
  mlp_chunk_grad_host(mlp_train_weights(w, D, n1, n2), X, n,
                      [&](int64_t r, double f, double* c) { *c = e[(size_t)r] = mlp_sub(t[r], f); return !mlp_feq0(*c); }, grad);
  *L = mlp_chunk_sqsum_host(e.data(), n, kMlpTrainChunk);
}

// One term's share of a batch, in the memory its evaluator works in.  rows == NULL: the term has no sampler and takes
// all its rows.  Supervised term: rows [n] = the batch, in batch order.  Path term: rows [n] = the rows the batch's paths name, ascending;
// the batch's P paths in batch order as a CSR over positions in rows; the rows' incidence lists restricted to the batch (sshmt_incidence
// over that CSR: entries position-in-batch * kSshmtMaxPath + slot, ascending).
struct MlpBatchView {
  const int32_t* rows = nullptr;
  long long n = 0, P = 0;
  const long long *offsets = nullptr, *members = nullptr, *inc_off = nullptr;
  const uint32_t* inc = nullptr;
};
// Whoever computes L and grad for the trainer; grad == NULL: L alone.  Returns a GLIA_HMT_* code.
struct MlpTrainEval {
  virtual ~MlpTrainEval() {}
  virtual int eval(const double* w, double* L, double* grad) = 0;
  // The term's gradient over a batch: the full-data definition applied to the batch's rows in batch order; no energy value.
  virtual int batch_grad(const double* w, const MlpBatchView& b, double* grad) = 0;
  // Device evaluators: the kernels of batch_grad up to the chunk partials, enqueued without a wait, the weights read from device memory;
  // *part_S [*n_chunks][d] is where the partials will lie.
  virtual int enqueue_batch(const double* d_w, const MlpBatchView& b, const double** part_S, long long* n_chunks) { return GLIA_HMT_ERR_INTERNAL; }
};
struct MlpTrainHostEval : MlpTrainEval {
  int D, n1, n2;
  const double *X, *t;
  int64_t n;
  int eval(const double* w, double* L, double* grad) override { mlp_loss_grad_host(w, D, n1, n2, X, t, n, L, grad); return 0; }
  int batch_grad(const double* w, const MlpBatchView& b, double* grad) override {
    double L;
    if (!b.rows) return eval(w, &L, grad);
    std::vector<double> Xb((size_t)b.n * D), tb((size_t)b.n);
    for (long long i = 0; i < b.n; ++i) {
      std::copy(X + (size_t)b.rows[i] * D, X + (size_t)(b.rows[i] + 1) * D, Xb.begin() + (size_t)i * D);
      tb[(size_t)i] = t[b.rows[i]];
    }
    mlp_loss_grad_host(w, D, n1, n2, Xb.data(), tb.data(), b.n, &L, grad);
    return 0;
  }
};
// The mini-batch step that takes the place of one update when a sampler is on (alg/gd.hxx:86-157; mlp_batch.hpp): every
// draw, gradient and update of the step, from w, om, ov to those after its last batch.
struct MlpBatchStep {
  virtual ~MlpBatchStep() {}
  virtual int run(const MlpStepRule& k, double step, std::vector<double>& w, std::vector<double>& om, std::vector<double>& ov) = 0;
};

struct MlpTrainResult {
  int D = 0, n1 = 0, n2 = 0;
  int64_t n_used = 0;                                 // rows with label +1 or -1
  std::vector<std::vector<double>> round_w;           // the weights after every sigma round
  std::vector<glia_hmt_mlp_train_record> trace;
  std::vector<double> sigma2, sigma2_eval;            // after every updateSigmaS: before round 0, then after each round
  int stopped_nonfinite = 0;
  std::vector<double> mn, mx;                         // the table the rows were rescaled by (empty: none)
  std::vector<double> sigma_u2, sigma_u2_eval;        // the unsupervised term's, after every updateSigmaU; 0.0 while it is off
  int64_t n_paths = 0, n_uns_rows = 0;                // merge paths and unlabelled rows of the unsupervised term
};
// The unsupervised term of the energy (sshmt_paths.hpp): its evaluator gives L_U = sum e_p^2 and grad_U = -sum e_p grad D_p.
struct MlpTrainUns {
  MlpTrainEval* ev = nullptr;
  int64_t n_paths = 0, n_rows = 0;
  double wu = 0.0, sigma_u = 0.0, min_sigma2 = 0.0;
  int update_sigma_u = 0;
};

inline bool mlp_isfeq(double a, double b) { return std::fabs(a - b) < kMlpTrainFeps; }
inline double mlp_max(double a, double b) { return a < b ? b : a; }      // std::max(a, b)
inline double mlp_sqnorm(const double* v, long long d) {
  double s = 0.0;
  for (long long p = 0; p < d; ++p) s = s + v[p] * v[p];
  return s;
}

// The defaults of the tool (main_train_sshmt_mlp.cxx:20-38,46-47); the floor of sigma^2 is what the tool passes (:138,160), 0.0.
inline void mlp_train_opts_default(glia_hmt_mlp_train_opts* o) {
  o->n1 = 10; o->n2 = 10; o->wr = 0.0; o->ws = 0.0; o->sigma_s = 0.0; o->update_sigma_s = 0; o->optimizer = 1; o->step = 0.0;
  o->step_decay = 1.0; o->fixed_step_decay_iterations = -1; o->sigma_update_step_period = -1; o->max_iterations = 0;
  o->n_sigma_updates = 0; o->pos_target = 0.05; o->neg_target = 0.95; o->min_sigma2 = 0.0; o->seed = 0;
  o->wu = 0.0; o->update_sigma_u = 0; o->sup_batch_size = -1; o->uns_batch_size = -1; o->balance_sup_batch = 0; o->alt_su = 0;
}
// What this library does not train (message, or empty), then what no trainer can run (message, or empty).
// with_u: the caller is the trainer that has the unsupervised term (sshmt_paths.hpp)
// batches: the caller is one of the *_train_batches entry points, which honour the three batch fields (mlp_batch.hpp)
inline std::string mlp_train_unsupported(const glia_hmt_mlp_train_opts& o, bool with_u = false, bool batches = false) {
  if (!with_u && !mlp_isfeq(o.wu, 0.0)) return "mlp_train: the unsupervised term (wu != 0; --uo, --uf, --wu) is not supported";
  if (!with_u && o.update_sigma_u) return "mlp_train: update_sigma_u (--usu) belongs to the unsupervised term, which is not supported";
  if (!batches && o.sup_batch_size > 0) return "mlp_train: sup_batch_size (--bss): batch samplers are not supported";
  if (!batches && o.uns_batch_size > 0) return "mlp_train: uns_batch_size (--bsu): batch samplers are not supported";
  if (!batches && o.balance_sup_batch) return "mlp_train: balance_sup_batch (--bb): batch samplers are not supported";
  if (o.alt_su) return "mlp_train: alt_su is not supported";
  if (o.n1 > kMlpTrainMaxHidden || o.n2 > kMlpTrainMaxHidden)
    return "mlp_train: more than " + std::to_string(kMlpTrainMaxHidden) + " units in a hidden layer are not supported";
  return std::string();
}
inline std::string mlp_train_bad_opts(const glia_hmt_mlp_train_opts& o, bool with_u = false) {
  if (o.n1 < 0 || o.n2 < 0 || (o.n1 == 0) != (o.n2 == 0)) return "mlp_train: hidden sizes must both be positive (or both 0: the logsig model)";
  if (with_u && mlp_isfeq(o.wr, 0.0) && mlp_isfeq(o.ws, 0.0) && mlp_isfeq(o.wu, 0.0)) return "sshmt_train: wr, wu and ws are all 0: no term of the energy is on";
  if (!with_u && mlp_isfeq(o.wr, 0.0) && mlp_isfeq(o.ws, 0.0)) return "mlp_train: wr and ws are both 0: no term of the energy is on";
  if (!mlp_isfeq(o.ws, 0.0) && o.sigma_s == 0.0 && !o.update_sigma_s) return "mlp_train: sigma_s is 0 and update_sigma_s is off: the supervised term divides by sigma^2";
  if (o.optimizer < 1 || o.optimizer > 3) return "Error: unsupported optimizer type...";
  if (o.max_iterations < 0 || o.n_sigma_updates < 0) return "mlp_train: max_iterations and n_sigma_updates must not be negative";
  if (!std::isfinite(o.wr) || !std::isfinite(o.ws) || !std::isfinite(o.sigma_s) || !std::isfinite(o.step) || !std::isfinite(o.step_decay) ||
      !std::isfinite(o.pos_target) || !std::isfinite(o.neg_target) || !std::isfinite(o.min_sigma2))
    return "mlp_train: an option is not finite";
  return std::string();
}

// The trainer.  w: the initial weights, the final ones on return; n: labelled rows; ev: the supervised term's evaluator (asked, and so
// needed, only while ws is on).  Returns the evaluator's code if it fails.
// U (optional): the unsupervised term; it is off without a path (sshmt/input.hxx:120-121).  The terms enter fx and g in the order
// regulariser, unsupervised, supervised (type/energy_function.hxx:164-230); without U not one operation differs from the supervised trainer.
// B (optional): the mini-batch step; without it not one operation differs from the full-batch trainer.
inline int mlp_train_run(const glia_hmt_mlp_train_opts& o, int64_t n, std::vector<double>& w, MlpTrainEval* ev, MlpTrainResult* R,
                         const MlpTrainUns* U = nullptr, MlpBatchStep* B = nullptr) {
  const long long d = (long long)w.size();
  const bool use_r = !mlp_isfeq(o.wr, 0.0), use_s = !mlp_isfeq(o.ws, 0.0);
  const bool use_u = U && U->ev && U->n_paths > 0 && !mlp_isfeq(U->wu, 0.0);
  double sigma_u2 = U ? U->sigma_u * U->sigma_u : 0.0;
  std::vector<double> gu(use_u ? (size_t)w.size() : 0);
  const double min_step = 1e-10, grad_tol = 1e-16, fixed_decay = 0.5;   // alg/gd.hxx:19-28
  double sigma2 = o.sigma_s * o.sigma_s;
  std::vector<double> g((size_t)d), gs((size_t)d), backup, om((size_t)d), ov((size_t)d);
  int rc = 0;
  auto rule = [&]() {
    MlpStepRule k;
    k.optimizer = o.optimizer; k.use_r = use_r; k.use_u = use_u; k.use_s = use_s;
    k.r_one = mlp_isfeq(o.wr, 1.0); k.u_one = use_u && mlp_isfeq(U->wu, 1.0); k.s_one = mlp_isfeq(o.ws, 1.0);
    k.wr = o.wr; k.wu = use_u ? U->wu : 0.0; k.ws = o.ws; k.sigma_u2 = sigma_u2; k.sigma2 = sigma2;
    return k;
  };

  // type/energy_function.hxx:164-230 with alg/function.hxx:72-77,257-267
  auto energy = [&](bool want_grad, double* fx) -> int {
    double L = 0.0, Lu = 0.0;
    if (use_u && (rc = U->ev->eval(w.data(), &Lu, want_grad ? gu.data() : nullptr))) return rc;
    if (use_s && (rc = ev->eval(w.data(), &L, want_grad ? gs.data() : nullptr))) return rc;
    double ret = 0.0;
    if (use_r) ret = ret + o.wr * (mlp_sqnorm(w.data(), d) / 2.0);
    if (use_u) ret = ret + U->wu * ((0.5 * Lu) / sigma_u2 + ((double)U->n_paths * std::log(sigma_u2)) / 2.0);
    if (use_s) ret = ret + o.ws * ((0.5 * L) / sigma2 + ((double)n * std::log(sigma2)) / 2.0);
    if (want_grad) {
      const MlpStepRule k = rule();
      for (long long p = 0; p < d; ++p) g[p] = mlp_energy_grad_elem(k, w[p], use_u ? gu[p] : 0.0, use_s ? gs[p] : 0.0);
    }
    *fx = ret;
    return 0;
  };
  // alg/gd.hxx:73-79 (1), 367-384 (2), 307-315 (3)
  auto update = [&](double step) -> int {
    if (B) return B->run(rule(), step, w, om, ov);      // alg/gd.hxx:191,238,249: helperMiniBatchGD in the update's place
    for (long long p = 0; p < d; ++p) mlp_update_elem(o.optimizer, step, g[p], &w[p], &om[p], &ov[p]);
    return 0;
  };
  // sshmt_util.hxx:140-145,188-207: sigma^2 = max(floor, L / n) when it is updated; the evaluated value is recorded either way
  // updateSigmaU (sshmt_util.hxx:148-185), after updateSigmaS (:210-222): sigma_u^2 = max(floor, L_U / P) when it is updated, and
  // the evaluated value is then sigma_u^2 itself either way (at the floor by the rule, above it because L_U / P is not negative)
  auto update_sigma_u = [&]() -> int {
    if (!use_u) { R->sigma_u2.push_back(sigma_u2); R->sigma_u2_eval.push_back(0.0); return 0; }
    double Lu = 0.0;
    if ((rc = U->ev->eval(w.data(), &Lu, nullptr))) return rc;
    const double v = Lu / (double)U->n_paths;
    if (U->update_sigma_u) sigma_u2 = mlp_max(U->min_sigma2, v);
    R->sigma_u2.push_back(sigma_u2);
    R->sigma_u2_eval.push_back(U->update_sigma_u ? sigma_u2 : mlp_max(0.0, v));
    return 0;
  };
  auto update_sigma_s = [&]() -> int {
    if (!use_s) { R->sigma2.push_back(sigma2); R->sigma2_eval.push_back(0.0); return 0; }
    double L = 0.0;
    if ((rc = ev->eval(w.data(), &L, nullptr))) return rc;
    const double v = L / (double)n;
    if (o.update_sigma_s) sigma2 = mlp_max(o.min_sigma2, v);
    R->sigma2.push_back(sigma2);
    R->sigma2_eval.push_back(o.update_sigma_s && sigma2 != o.min_sigma2 ? sigma2 : mlp_max(0.0, v));
    return 0;
  };
  auto update_sigma = [&]() -> int {
    if ((rc = update_sigma_s())) return rc;
    return update_sigma_u();
  };
  auto record = [&](int round, int t, int kind, double fx, double xx, double gg, double step, int rollbacks) {
    glia_hmt_mlp_train_record r;
    r.fx = fx; r.xnorm = std::sqrt(xx); r.gnorm = std::sqrt(gg); r.step = step; r.sigma2 = sigma2;
    r.round = round; r.t = t; r.kind = kind; r.rollbacks = rollbacks;
    R->trace.push_back(r);
  };

  double cur_step = o.step;
  if ((rc = update_sigma())) return rc;
  for (int round = 0; round < o.n_sigma_updates && !R->stopped_nonfinite; ++round) {
    if (o.sigma_update_step_period > 0 && round > 0 && round % o.sigma_update_step_period == 0) cur_step = mlp_max(cur_step * 0.5, min_step);
    if (o.max_iterations > 0) {
      std::fill(om.begin(), om.end(), 0.0);
      std::fill(ov.begin(), ov.end(), 0.0);
      bool have_backup = false;
      double step = cur_step, fx = 0.0, gg = 0.0;
      auto stop_nonfinite = [&](int t, double xx, int rollbacks) {
        record(round, t, 2, fx, xx, gg, step, rollbacks);
        if (have_backup) w = backup;
        R->stopped_nonfinite = 1;
      };
      if (mlp_isfeq(o.step_decay, 1.0)) {                 // fixedStepGD (alg/gd.hxx:159-208)
        for (int t = 0; t <= o.max_iterations; ++t) {     // t == max_iterations: the final statistics
          const bool last = t == o.max_iterations;
          if (!last && o.fixed_step_decay_iterations > 0 && t > 0 && t % o.fixed_step_decay_iterations == 0) step = mlp_max(min_step, step * fixed_decay);
          if ((rc = energy(true, &fx))) return rc;
          gg = mlp_sqnorm(g.data(), d);
          const double xx = mlp_sqnorm(w.data(), d);
          if (!std::isfinite(fx) || !std::isfinite(gg)) { stop_nonfinite(t, xx, 0); break; }
          record(round, t, last ? 1 : 0, fx, xx, gg, step, 0);
          if (last) break;
          if (std::sqrt(gg) < grad_tol) t = o.max_iterations - 1;      // stop: only the final statistics are left
          else { backup = w; have_backup = true; if ((rc = update(step))) return rc; }
        }
      } else {                                            // adaptiveStepGD (alg/gd.hxx:210-272)
        int t = 0;
        while (t < o.max_iterations) {
          if ((rc = energy(true, &fx))) return rc;
          gg = mlp_sqnorm(g.data(), d);
          const double xx = mlp_sqnorm(w.data(), d);
          if (!std::isfinite(fx) || !std::isfinite(gg)) { stop_nonfinite(t, xx, 0); break; }
          if (std::sqrt(gg) < grad_tol) break;
          backup = w; have_backup = true;
          if ((rc = update(step))) return rc;
          const double fx_prev = fx;
          int rollbacks = 0;
          if ((rc = energy(false, &fx))) return rc;
          while (step > min_step && fx >= fx_prev) {
            step = mlp_max(min_step, step * o.step_decay);
            if (step == min_step) break;
            w = backup;
            if ((rc = update(step))) return rc;
            if ((rc = energy(false, &fx))) return rc;
            ++rollbacks;
          }
          record(round, t, 0, fx_prev, xx, gg, step, rollbacks);
          if (!std::isfinite(fx)) { stop_nonfinite(t, xx, rollbacks); break; }
          ++t;
        }
        if (!R->stopped_nonfinite) record(round, t, 1, fx, mlp_sqnorm(w.data(), d), gg, step, 0);
      }
    }
    R->round_w.push_back(w);
    if (R->stopped_nonfinite) break;
    if ((rc = update_sigma())) return rc;
  }
  return 0;
}

// stats::rescale's table over several row blocks (util/stats.hxx:280-314): per-column minimum and maximum.  The minimum starts at
// DBL_MAX and the maximum at DBL_MIN, the smallest positive normal (glia_base.hxx:46-47): a column without a positive value keeps it.
inline void mlp_rows_minmax(const double* const* blocks, const int64_t* n_rows, int n_blocks, int dim, double* mn, double* mx) {
  for (int j = 0; j < dim; ++j) { mn[j] = 1.7976931348623157e308; mx[j] = 2.2250738585072014e-308; }
  for (int b = 0; b < n_blocks; ++b)
    for (int64_t r = 0; r < n_rows[b]; ++r)
      for (int j = 0; j < dim; ++j) {
        const double f = blocks[b][(size_t)r * dim + j];
        if (f < mn[j]) mn[j] = f;
        if (f > mx[j]) mx[j] = f;
      }
}

// The rows the trainer sees (sshmt_util.hxx:11-27, input.hxx:74-91): rows with label +1 / -1 in input order, rescaled when a table
// is given (mlp_rescale_den with den = (max - min) + FEPS), a 1.0 appended; targets pos_target / neg_target.
inline void mlp_train_prepare(const double* rows, int64_t n_rows, int dim, const int32_t* labels, const double* mn, const double* mx,
                              double pos_target, double neg_target, std::vector<double>* X, std::vector<double>* t) {
  X->clear(); t->clear();
  for (int64_t r = 0; r < n_rows; ++r) {
    if (labels[r] != 1 && labels[r] != -1) continue;
    for (int j = 0; j < dim; ++j) {
      const double v = rows[(size_t)r * dim + j];
      X->push_back(mn ? mlp_rescale_den(v, mn[j], (mx[j] - mn[j]) + kMlpTrainFeps) : v);
    }
    X->push_back(1.0);
    t->push_back(labels[r] == 1 ? pos_target : neg_target);
  }
}

}  // namespace glia
