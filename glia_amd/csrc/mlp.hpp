// glia_amd/csrc/mlp.hpp -- the MLP / logsig classifier as the device sees it (mlp_predict.hip; host side: mlp_model.hpp).
#pragma once
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

// ---- training (mlp_train.hip; the definition: mlp_backward.hpp) ----
// The device evaluator of the trainer: prepared rows X [n][D] and targets [n] resident for the state's lifetime.  create: a memory plan
// beyond 85 % of the free device memory is GLIA_HMT_ERR_UNSUPPORTED.  eval: L = sum e^2 and, when h_grad != NULL, grad = -sum g_i e_i
// for the weights h_w, in the two-level order of the definition.
struct MlpTrainDevice;
int mlp_train_device_create(const double* h_X, const double* h_t, long long n, int D, int n1, int n2, int exp_variant, hipStream_t stream,
                            MlpTrainDevice** out);
int mlp_train_device_eval(MlpTrainDevice* st, const double* h_w, double* L, double* h_grad);
void mlp_train_device_timing(const MlpTrainDevice* st, glia_hmt_mlp_train_timing* out);      // adds the device times, sets device_bytes
void mlp_train_device_free(MlpTrainDevice* st);

// ---- the merge-path term (sshmt_train.hip; the definition: sshmt_paths.hpp) ----
// The device evaluator of the unsupervised term: the unlabelled rows, paths and incidence lists of `in` resident for the state's
// lifetime.  eval: L_U = sum e_p^2 and, when h_grad != NULL, grad_U = -sum_r c_r g_r.  Memory plan as above.
struct SshmtInput;
struct SshmtTrainDevice;
int sshmt_train_device_create(const SshmtInput& in, int n1, int n2, int exp_variant, hipStream_t stream, SshmtTrainDevice** out);
int sshmt_train_device_eval(SshmtTrainDevice* st, const double* h_w, double* L, double* h_grad);
void sshmt_train_device_timing(const SshmtTrainDevice* st, glia_hmt_sshmt_train_timing* out);      // fills all but out->sup
void sshmt_train_device_free(SshmtTrainDevice* st);

}  // namespace glia
