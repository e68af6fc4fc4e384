// glia_amd/csrc/mlp_train_device.hpp -- what the device evaluators of both terms of the energy share (mlp_train.hip: the supervised
// term, sshmt_train.hip: the merge-path term): the chunk kernel of grad = -sum_r c_r g_r, stated once over a term
// policy that says where c_r comes from, and TrainCall, the owner of an evaluator's device state.
//
// k_train_chunk: one workgroup per chunk of kMlpTrainChunk = 64 consecutive rows.  Phase A runs the forward and backward pass of the
// chunk's rows: the pre-activations, dh1 / dh2, dh3 and c of every row (and the merge-path term's flag) lie in LDS, unit-major ([unit][row]: the lanes of
// a wave are rows, so a wave reads and writes 64 consecutive doubles), one thread per (row, unit) for the layers and for dh1, one thread
// per row for the logit, the sigmoid, the term's coefficient and dh2.  Phase B: every thread owns weights p, p + 256, ... and walks the
// chunk's rows in ascending order, S = S - (g_r[p] * c_r); with the model's column-major layout consecutive threads read consecutive
// columns of a row.  The chunk sums go to partials [chunk][weight]; k_train_fold (mlp_train.hip) adds them per weight in ascending
// chunk order.  No atomics: the order is the result.
#pragma once
#include <vector>

#include "hmt_internal.hpp"
#include "glibc_math.hpp"
#include "mlp_backward.hpp"

namespace glia {

static_assert(kMlpTrainChunk == 64, "the chunk kernel maps one row to one lane of a wave");
constexpr int kTrainThreads = 256;

// The supervised term: c_r = e_r = t_r - f_r, a row with |e_r| < FEPS skipped; part_L[chunk] = the chunk's sum of e_r^2, with or
// without the gradient.
struct TermSupervised {
  static constexpr bool kLossByChunk = true;
  static constexpr bool kGather = false;
  const double* tgt;
  double* part_L;
  __device__ void row(long long r, double f, int want_grad, double* c, uint32_t* named) const { *c = mlp_sub(tgt[r], f); }
  static __device__ bool skipped(double c, const uint32_t* named) { return mlp_feq0(c); }
};
// The merge-path term: c_r and whether a live path names the row from k_sshmt_gather; without the gradient the kernel is the forward
// pass alone, f to f_out.
struct TermPaths {
  static constexpr bool kLossByChunk = false;
  static constexpr bool kGather = false;
  const double* coef;
  const uint32_t* named;
  double* f_out;
  __device__ void row(long long r, double f, int want_grad, double* c, uint32_t* is_named) const {
    if (!want_grad) { f_out[r] = f; return; }
    *c = coef[r];
    *is_named = named[r];
  }
  static __device__ bool skipped(double c, const uint32_t* is_named) { return !*is_named; }
};

// The terms over a batch: row r of the kernel is X[rows[r]] -- the row-indirected instances of the chunk kernel.  A batch
// has no energy value.  Supervised: rows = the batch in batch order, the targets by row.  Paths: rows = the rows the batch's paths
// name, ascending; c, named and f by position in rows.
struct TermSupervisedBatch {
  static constexpr bool kLossByChunk = false;
  static constexpr bool kGather = true;
  const int32_t* rows;
  const double* tgt;
  __device__ void row(long long r, double f, int want_grad, double* c, uint32_t* named) const { *c = mlp_sub(tgt[rows[r]], f); }
  static __device__ bool skipped(double c, const uint32_t* named) { return mlp_feq0(c); }
};
struct TermPathsBatch {
  static constexpr bool kLossByChunk = false;
  static constexpr bool kGather = true;
  const int32_t* rows;
  TermPaths local;
  __device__ void row(long long r, double f, int want_grad, double* c, uint32_t* is_named) const { local.row(r, f, want_grad, c, is_named); }
  static __device__ bool skipped(double c, const uint32_t* is_named) { return TermPaths::skipped(c, is_named); }
};

template <int NMAX, class Term>
__global__ __launch_bounds__(kTrainThreads) void k_train_chunk(const double* __restrict__ X, long long n, int D, int n1, int n2,
                                                              const double* __restrict__ w, long long d, int exp_variant, int want_grad,
                                                              Term term, double* __restrict__ part_S) {
  constexpr int C = kMlpTrainChunk;
  __shared__ double s_h1[NMAX * C], s_h2[NMAX * C], s_dh1[NMAX * C], s_dh2[NMAX * C], s_dh3[C], s_c[C];
  __shared__ uint32_t s_named[C];      // (TermPaths alone)
  const long long chunk = blockIdx.x, r0 = chunk * C;
  const int nr = (int)(n - r0 < C ? n - r0 : C);
  const int tid = threadIdx.x;
  const MlpWeights m = mlp_train_weights(w, D, n1, n2);
  const double* Xc = X + (size_t)r0 * (size_t)D;
  __shared__ int32_t s_row[Term::kGather ? C : 1];      // (the batch terms alone)
  if constexpr (Term::kGather) {
    if (tid < nr) s_row[tid] = term.rows[r0 + tid];
    __syncthreads();
  }
  auto xrow = [&](int r) -> const double* {
    if constexpr (Term::kGather) return X + (size_t)s_row[r] * (size_t)D;
    else return Xc + (size_t)r * (size_t)D;
  };

  // ---- phase A: forward ----
  if (n1 > 0) {
    for (int q = tid; q < C * n1; q += kTrainThreads) {
      const int r = q & (C - 1), k = q >> 6;
      if (r < nr) s_h1[k * C + r] = mlp_unit(m.w0, D, 1, k, MlpRow{xrow(r)});
    }
    __syncthreads();
    for (int q = tid; q < C * n2; q += kTrainThreads) {
      const int r = q & (C - 1), k = q >> 6;
      if (r < nr) s_h2[k * C + r] = mlp_unit(m.w1, n1 + 1, 1, k, MlpActs{s_h1 + r, n1, C});
    }
    __syncthreads();
  }
  if (tid < nr) {
    const int r = tid;
    const double h3 = n1 > 0 ? mlp_unit(m.w2, n2 + 1, 1, 0, MlpActs{s_h2 + r, n2, C}) : mlp_unit(m.w2, D, 1, 0, MlpRow{xrow(r)});
    const double f = glibc::sigmoid(h3, exp_variant);
    term.row(r0 + r, f, want_grad, &s_c[r], &s_named[r]);
    if (want_grad) {
      const double dh3 = mlp_dh3(f);
      s_dh3[r] = dh3;
      for (int k = 0; k < n2; ++k) s_dh2[k * C + r] = mlp_dh2(m, k, s_h2[k * C + r], dh3);
    }
  }
  if (!Term::kLossByChunk && !want_grad) return;      // (the same in every thread)
  __syncthreads();
  if constexpr (Term::kLossByChunk) {
    if (tid == 0) {
      double Lc = 0.0;
      for (int r = 0; r < nr; ++r) Lc = mlp_add(Lc, mlp_mul(s_c[r], s_c[r]));
      term.part_L[chunk] = Lc;
    }
    if (!want_grad) return;
  }
  // ---- phase A: backward ----
  if (n1 > 0) {
    for (int q = tid; q < C * n1; q += kTrainThreads) {
      const int r = q & (C - 1), j = q >> 6;
      if (r < nr) s_dh1[j * C + r] = mlp_dh1(m, j, s_h1[j * C + r], s_dh2 + r, C);
    }
    __syncthreads();
  }
  // ---- phase B: the chunk sums ----
  double* out = part_S + (size_t)chunk * (size_t)d;
  for (long long p = tid; p < d; p += kTrainThreads) {
    double S = 0.0;
    for (int r = 0; r < nr; ++r) {
      const double c = s_c[r];
      if (Term::skipped(c, s_named + r)) continue;
      const double g = mlp_grad_elem(m, p, MlpRow{xrow(r)}, s_h1 + r, s_h2 + r, s_dh1 + r, s_dh2 + r, s_dh3[r], C);
      S = mlp_sub(S, mlp_mul(g, c));
    }
    out[p] = S;
  }
}

// The trainers' memory rule, in one place (mlp_train.hip): device memory of `bytes` beyond 85 % of what is free is
// GLIA_HMT_ERR_UNSUPPORTED with "<who> needs .. MiB of device memory<detail>, more than 85 % of the .. MiB free".
int train_memory_fits(uint64_t bytes, const std::string& who, const std::string& detail);

// The device state of one evaluator for the lifetime of a training call: the prepared rows X [n][D], the weights, the chunk partials
// part_S [n_chunks][d] and part_L [n_L], out = the gradient [d] then L, every further array its term wants, and the events around
// the stages of an evaluation.  One stream; nothing is allocated per evaluation.  The caller sets the shape, names its term's own
// arrays (want), then open().
struct TrainCall {
  int D = 0, n1 = 0, n2 = 0, exp_variant = 0;
  long long n = 0, n_L = 0;            // rows; entries of part_L
  hipStream_t stream = nullptr;
  long long d = 0, n_chunks = 0;
  double *X = nullptr, *w = nullptr, *part_S = nullptr, *part_L = nullptr, *out = nullptr;
  struct Array { void** p; uint64_t bytes; };
  std::vector<Array> arrays;           // the term's own, then (open) every array of the call: the memory plan, the hipMallocs, the hipFrees
  hipEvent_t ev[8] = {};
  std::vector<double> h_out;

  TrainCall() = default;
  TrainCall(const TrainCall&) = delete;
  TrainCall& operator=(const TrainCall&) = delete;
  ~TrainCall();
  template <class T> void want(T** p, uint64_t count) { arrays.push_back({(void**)p, sizeof(T) * count}); }
  // The memory plan -- all arrays -- against 85 % of the free device memory: "<term>: <what> needs .. MiB of device memory (rows .. MiB,
  // chunk partials .. MiB<more>), more than 85 % of the .. MiB free".  Then the allocations (X, the term's, the rest) and the events.
  int open(const std::string& term, const std::string& what, const std::string& more, uint64_t* plan_bytes);
  hipError_t mark(int i) { return hipEventRecord(ev[i], stream); }
  hipError_t to_device(void* dst, const void* src, uint64_t bytes) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream); }
  // waits for the stream; ms[i] = the time from mark i to mark i + 1, i + 1 < n_marks
  int wait(int n_marks, float* ms);
  // An evaluation: begin_eval (mark 0, the weights up, mark 1), the term's kernels and marks 2 .. marks - 1, finish_eval (the fold,
  // mark `marks`, L and -- h_grad != NULL -- the gradient down, mark marks + 1, wait: ms [marks + 1]).
  int begin_eval(const double* h_w);
  // rows, wp (batches): the kernel's row count when it is not n, the weights when they are not this call's copy
  template <class Term> int chunk(const Term& term, int want_grad, long long rows = -1, const double* wp = nullptr) {
    if (rows < 0) rows = n;
    if (!wp) wp = w;
    if (rows < 1 || rows > n) { set_error("mlp_train: a batch outside its term's rows"); return GLIA_HMT_ERR_INTERNAL; }
    const dim3 grid((unsigned)((rows + kMlpTrainChunk - 1) / kMlpTrainChunk)), block(kTrainThreads);
    if (n1 <= 16 && n2 <= 16)
      hipLaunchKernelGGL((k_train_chunk<16, Term>), grid, block, 0, stream, X, rows, D, n1, n2, wp, d, exp_variant, want_grad, term, part_S);
    else
      hipLaunchKernelGGL((k_train_chunk<kMlpTrainMaxHidden, Term>), grid, block, 0, stream, X, rows, D, n1, n2, wp, d, exp_variant, want_grad, term,
                         part_S);
    GLIA_HIP_TRY(hipGetLastError());
    return GLIA_HMT_OK;
  }
  // chunks (batches): the chunk partials to fold when they are not all n_chunks; a batch has no energy value, so none of part_L is
  // folded and *L is +0.0
  int finish_eval(int marks, double* L, double* h_grad, float* ms, long long chunks = -1);
};

}  // namespace glia
