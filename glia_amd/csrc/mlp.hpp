// glia_amd/csrc/mlp.hpp -- the MLP / logsig classifier as the device sees it (mlp_predict.hip; host side: mlp_model.hpp).
#pragma once
#include <memory>

#include "hmt_internal.hpp"
#include "mlp_model.hpp"

namespace glia {

struct DeviceMlp {
  int n_models;            // 1 or 3
  int n1, n2, D;           // hidden units (0 / 0: logsig), columns of a row + 1
  int ub1, nb1, ub2, nb2;  // unit block and blocks of the two hidden layers (mlp_unit_block)
  int rescale;
  int dim0, dim1;
  double threshold;
  const double* w0[3];     // [nb1][D][ub1]       (mlp_block_weights)
  const double* w1[3];     // [nb2][n1 + 1][ub2]
  const double* w2[3];     // [n2 + 1]; logsig: [D]
  const double* mn;        // [D - 1] when rescale: the minima
  const double* den;       //                       (max - min) + FEPS
};

// logit[i] and / or pred[i] for row i (device arrays; row i starts at d_rows + i * row_stride); either output may be NULL
int launch_mlp_predict(const DeviceMlp& mlp, const double* d_rows, long long n_rows, long long row_stride, double* d_pred, double* d_logit,
                       hipStream_t stream);

// ---- training: the device evaluators (MlpTrainEval, mlp_backward.hpp) of the two terms of the energy ----
// Resident for the evaluator's lifetime: the prepared rows X [n][D] and targets [n] (mlp_train.hip: L = sum e^2, grad = -sum g_i e_i), or
// the unlabelled rows, paths and incidence lists of `in` (sshmt_train.hip; the definition: sshmt_paths.hpp: L_U = sum e_p^2,
// grad_U = -sum_r c_r g_r).  create: a memory plan beyond 85 % of the free device memory is GLIA_HMT_ERR_UNSUPPORTED.  The evaluator adds
// its device times and counts to *tm, which outlives it (of glia_hmt_sshmt_train_timing: all but sup).
struct MlpTrainEval;
struct SshmtInput;
int mlp_train_device_create(const double* h_X, const double* h_t, long long n, int D, int n1, int n2, int exp_variant, hipStream_t stream,
                            glia_hmt_mlp_train_timing* tm, std::unique_ptr<MlpTrainEval>* out);
int sshmt_train_device_create(const SshmtInput& in, int n1, int n2, int exp_variant, hipStream_t stream, glia_hmt_sshmt_train_timing* tm,
                              std::unique_ptr<MlpTrainEval>* out);
// The mini-batch step over device evaluators (mlp_batch.hip): route GLIA_HMT_BATCH_STREAM | GLIA_HMT_BATCH_STEP, d weights.
// The caller fills the step's options, samplers, input and evaluators (mlp_batch.hpp).
struct MlpBatchHostStep;
int mlp_batch_device_create(hipStream_t stream, int route, long long d, std::unique_ptr<MlpBatchHostStep>* out);

}  // namespace glia
