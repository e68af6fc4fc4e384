// glia_amd/csrc/forest_train.hpp -- growing the boundary classifier's forest on the device (forest_train.hip).
#pragma once
#include "forest_model.hpp"
#include "hmt_internal.hpp"

namespace glia {

// the splitmix64 finaliser and the one source of randomness of a training call: h(t, a, b) = mix(mix(mix(mix(seed) ^ t) ^ a) ^ b)
__host__ __device__ inline uint64_t rf_mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// Grows plan/opts' forest on rows x [n_rows][dim] (host, validated by train_plan) and fills *out.  A plan whose device memory does
// not fit: GLIA_HMT_ERR_UNSUPPORTED.
int forest_train_device(const double* h_x, int64_t n_rows, int dim, const TrainPlan& plan, const TrainOptions& opts, hipStream_t stream,
                        ForestModel* out, glia_hmt_forest_train_timing* timing);

}  // namespace glia
