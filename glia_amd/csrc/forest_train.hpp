// glia_amd/csrc/forest_train.hpp -- growing the boundary classifier's forest on the device (forest_train.hip) and what the
// trees say about rows they did not see (forest_oob.hip).
#pragma once
#include "forest_model.hpp"
#include "forest_oob.hpp"
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
// not fit: GLIA_HMT_ERR_UNSUPPORTED.  oob (may be NULL: neither) asks for the out-of-bag arrays and / or the importances of *out;
// oob_timing is written whenever it is not NULL.
int forest_train_device(const double* h_x, int64_t n_rows, int dim, const TrainPlan& plan, const TrainOptions& opts, hipStream_t stream,
                        ForestModel* out, glia_hmt_forest_train_timing* timing, const OobOptions* oob = nullptr,
                        glia_hmt_forest_oob_timing* oob_timing = nullptr);

// A batch of grown trees as forest_train.hip holds them on the device when the out-of-bag passes run.
struct OobBatch {
  const double* X; const uint8_t* ycls;          // rows [N][D], class of every row
  const uint32_t *cnt, *pos;                     // [T * N (+ 1)] bootstrap multiplicities and the exclusive scan of "in bag"
  const int *o_left, *o_var, *o_class, *ndbig;   // [T][cap] 1-based left daughter / variable / class, [T] nodes of every tree
  const double* o_split;
  int tree0, T;                                  // first tree of the batch, trees in it
};

// The out-of-bag passes of one training call (forest_oob.hip): memory planned with the trainer's, one run per batch of trees, and the
// arrays of the model at the end.
class OobPass {
 public:
  OobPass();
  ~OobPass();
  OobPass(const OobPass&) = delete;
  OobPass& operator=(const OobPass&) = delete;
  // device bytes the passes take with T trees in flight
  static uint64_t bytes(const OobOptions& o, uint64_t N, uint64_t D, uint64_t nclass, uint64_t T, uint64_t cap, uint64_t ntree);
  int init(const OobOptions& o, int64_t N, int D, const TrainPlan& plan, const TrainOptions& opts, uint64_t T, uint64_t cap, hipStream_t stream,
           glia_hmt_forest_oob_timing* timing);
  // h_left / h_var: the batch's trees on the host ([t] -> nodes, 1-based as the model holds them), for the Gini decreases
  int run(const OobBatch& b, const std::vector<int>* h_left, const std::vector<int>* h_var);
  int finish(ForestModel* model);
 private:
  struct Impl;
  Impl* p_;
};

}  // namespace glia
