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

}  // namespace glia
