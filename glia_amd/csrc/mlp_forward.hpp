// glia_amd/csrc/mlp_forward.hpp -- the forward pass of the MLP classifier stated ONCE for the host and the
// device: the host definition (mlp_model.hpp: mlp_forward) and the classifier loop (greedy_bc.hip: the initial edges one thread per
// edge, the rounds one thread per (record, hidden unit)) are both written with the functions below, so they cannot drift apart.  The
// batch predictor (mlp_predict.hip) keeps its own register-blocked loops and is held to this definition by its tests.
//
// Every sum starts at +0.0 and takes its terms in ascending index order; a multiply and an add are rounded separately (host code is
// built with -ffp-contract=off, device code says so per operation); a chain is never split.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define GLIA_MLP_HD __host__ __device__ inline
#else
#define GLIA_MLP_HD inline
#endif

namespace glia {

GLIA_MLP_HD double mlp_mul(double a, double b) {
#ifdef __HIP_DEVICE_COMPILE__
  return __dmul_rn(a, b);
#else
  return a * b;
#endif
}
GLIA_MLP_HD double mlp_add(double a, double b) {
#ifdef __HIP_DEVICE_COMPILE__
  return __dadd_rn(a, b);
#else
  return a + b;
#endif
}
// step 1, stats::rescale (util/stats.hxx:265-277) with den = (max - min) + FEPS, which does not depend on the row
GLIA_MLP_HD double mlp_rescale_den(double x, double mn, double den) {
#ifdef __HIP_DEVICE_COMPILE__
  return __dadd_rn(__ddiv_rn(__dmul_rn(2.0, __dsub_rn(x, mn)), den), -1.0);
#else
  return ((2.0 * (x - mn)) / den) + (-1.0);
#endif
}
// step 3, opt::ThresholdModelDistributor (type/function.hxx:80-84) on the rescaled, bias-appended vector; x(j) = its column j
template <class X> GLIA_MLP_HD int mlp_pick_of(int n_models, int dim0, int dim1, double threshold, const X& x) {
  if (n_models == 1) return 0;
  return x(dim1) < threshold ? 0 : (x(dim0) < threshold ? 1 : 2);
}
GLIA_MLP_HD double mlp_relu(double h) { return h > 0.0 ? h : 0.0; }      // a NaN becomes 0

// One model's weights.  A layer of din inputs and n units lies in blocks of ub units, [block][j][ub]: ub = 1 is the model file's
// column-major matrix (host), ub > 1 the layout the device holds (mlp_block_weights).
struct MlpWeights {
  int D, n1, n2;           // D = columns of a row + 1; n1 == 0: logsig, w2 holds its D weights
  int ub1, ub2;
  const double *w0, *w1, *w2;
};
// steps 4 to 6: unit k of a layer = the chain over its din inputs in(0), in(1), ...
template <class In> GLIA_MLP_HD double mlp_unit(const double* w, int din, int ub, int k, const In& in) {
  const double* p = w + (size_t)(k / ub) * (size_t)din * (size_t)ub + (size_t)(k % ub);
  double h = 0.0;
  for (int j = 0; j < din; ++j) h = mlp_add(h, mlp_mul(in(j), p[(size_t)j * (size_t)ub]));
  return h;
}
// an array with a 1.0 behind its n entries (the bias input of a layer)
struct MlpBiased {
  const double* p;
  int n;
  GLIA_MLP_HD double operator()(int j) const { return j < n ? p[j] : 1.0; }
};
// The logit of one row: x(j) = column j of the rescaled, bias-appended vector; a1 [n1] and a2 [n2] are scratch.
template <class X> GLIA_MLP_HD double mlp_logit(const MlpWeights& m, const X& x, double* a1, double* a2) {
  if (m.n1 == 0) return mlp_unit(m.w2, m.D, 1, 0, x);
  for (int k = 0; k < m.n1; ++k) a1[k] = mlp_relu(mlp_unit(m.w0, m.D, m.ub1, k, x));
  for (int k = 0; k < m.n2; ++k) a2[k] = mlp_relu(mlp_unit(m.w1, m.n1 + 1, m.ub2, k, MlpBiased{a1, m.n1}));
  return mlp_unit(m.w2, m.n2 + 1, 1, 0, MlpBiased{a2, m.n2});
}

}  // namespace glia
