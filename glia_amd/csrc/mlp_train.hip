// glia_amd/csrc/mlp_train.hip -- the device evaluator of the MLP / logsig trainer (the definition: mlp_backward.hpp): the
// supervised term over the chunk kernel of mlp_train_device.hpp, and what that header's TrainCall declares -- the fold kernel, the
// memory plan, the upload of the weights and the read-back.  An evaluation reads back L and, when asked, the gradient -- the update
// itself is the header's, on the host.
#include "mlp.hpp"
#include "mlp_train_device.hpp"

namespace glia {

// grad[p] = the chunk sums of weight p, chunks ascending from +0.0 (threads [0, d)); L the same over the n_L entries of part_L (thread d).
// (n_L comes last: with it next to n_chunks the kernel measured 0.005 to 0.010 ms slower at 512 chunks, profiles/train_refactor_pairs.txt)
__global__ __launch_bounds__(kTrainThreads) void k_train_fold(const double* __restrict__ part_S, const double* __restrict__ part_L, long long n_chunks,
                                                             long long d, int want_grad, double* __restrict__ grad, double* __restrict__ L,
                                                             long long n_L) {
  const long long p = (long long)blockIdx.x * kTrainThreads + threadIdx.x;
  if (p == d) {
    double acc = 0.0;
    for (long long c = 0; c < n_L; ++c) acc = mlp_add(acc, part_L[c]);
    *L = acc;
  } else if (p < d && want_grad) {
    double acc = 0.0;
    for (long long c = 0; c < n_chunks; ++c) acc = mlp_add(acc, part_S[(size_t)c * (size_t)d + (size_t)p]);
    grad[p] = acc;
  }
}

int train_memory_fits(uint64_t bytes, const std::string& who, const std::string& detail) {
  size_t free_b = 0, total_b = 0;
  GLIA_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if (bytes > (uint64_t)(0.85 * (double)free_b)) {
    set_error(who + " needs " + std::to_string(bytes >> 20) + " MiB of device memory" + detail + ", more than 85 % of the " + std::to_string(free_b >> 20) +
              " MiB free");
    return GLIA_HMT_ERR_UNSUPPORTED;
  }
  return GLIA_HMT_OK;
}

TrainCall::~TrainCall() {
  for (const Array& a : arrays) if (*a.p) (void)hipFree(*a.p);      // (the pointers start out NULL: a call that failed half-way frees what it got)
  for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
}

int TrainCall::open(const std::string& term, const std::string& what, const std::string& more, uint64_t* plan_bytes) {
  d = mlp_train_n_weights(D, n1, n2);
  n_chunks = (n + kMlpTrainChunk - 1) / kMlpTrainChunk;
  if (n_chunks > 0x7fffffffll) { set_error(term + ": more than 2^31 chunks of rows"); return GLIA_HMT_ERR_UNSUPPORTED; }
  const uint64_t rows = 8 * (uint64_t)n * (uint64_t)D, partials = 8 * (uint64_t)n_chunks * (uint64_t)d;
  arrays.insert(arrays.begin(), Array{(void**)&X, rows});
  want(&w, (uint64_t)d);
  want(&part_S, (uint64_t)n_chunks * (uint64_t)d);
  want(&part_L, (uint64_t)n_L);
  want(&out, (uint64_t)d + 1);
  uint64_t bytes = 0;
  for (const Array& a : arrays) bytes += a.bytes;
  if (int rc = train_memory_fits(bytes, term + ": " + what, " (rows " + std::to_string(rows >> 20) + " MiB, chunk partials " + std::to_string(partials >> 20) +
                                                             " MiB" + more + ")"))
    return rc;
  *plan_bytes = bytes;
  for (const Array& a : arrays) GLIA_HIP_TRY(hipMalloc(a.p, a.bytes));
  for (hipEvent_t& e : ev) GLIA_HIP_TRY(hipEventCreate(&e));
  h_out.resize((size_t)d + 1);
  return GLIA_HMT_OK;
}

int TrainCall::wait(int n_marks, float* ms) {
  GLIA_HIP_TRY(hipStreamSynchronize(stream));
  for (int i = 0; i + 1 < n_marks; ++i) GLIA_HIP_TRY(hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]));
  return GLIA_HMT_OK;
}

int TrainCall::begin_eval(const double* h_w) {
  GLIA_HIP_TRY(mark(0));
  GLIA_HIP_TRY(to_device(w, h_w, 8 * (uint64_t)d));
  GLIA_HIP_TRY(mark(1));
  return GLIA_HMT_OK;
}

int TrainCall::finish_eval(int marks, double* L, double* h_grad, float* ms, long long chunks) {
  const size_t nd = (size_t)d;
  hipLaunchKernelGGL(k_train_fold, dim3((unsigned)((nd + 1 + kTrainThreads - 1) / kTrainThreads)), dim3(kTrainThreads), 0, stream, part_S, part_L,
                     chunks < 0 ? n_chunks : chunks, d, h_grad ? 1 : 0, out, out + nd, chunks < 0 ? n_L : 0);
  GLIA_HIP_TRY(hipGetLastError());
  GLIA_HIP_TRY(mark(marks));
  if (h_grad) GLIA_HIP_TRY(hipMemcpyAsync(h_out.data(), out, 8 * (nd + 1), hipMemcpyDeviceToHost, stream));
  else GLIA_HIP_TRY(hipMemcpyAsync(h_out.data() + nd, out + nd, 8, hipMemcpyDeviceToHost, stream));
  GLIA_HIP_TRY(mark(marks + 1));
  if (int rc = wait(marks + 2, ms)) return rc;
  *L = h_out[nd];
  if (h_grad) std::copy(h_out.begin(), h_out.begin() + nd, h_grad);
  return GLIA_HMT_OK;
}

namespace {

struct MlpTrainDevice : MlpTrainEval {
  TrainCall call;
  double* t = nullptr;
  glia_hmt_mlp_train_timing* tm = nullptr;

  int eval(const double* h_w, double* L, double* h_grad) override {
    float ms[4] = {0, 0, 0, 0};
    if (int rc = call.begin_eval(h_w)) return rc;
    if (int rc = call.chunk(TermSupervised{t, call.part_L}, h_grad ? 1 : 0)) return rc;
    GLIA_HIP_TRY(call.mark(2));
    if (int rc = call.finish_eval(3, L, h_grad, ms)) return rc;
    tm->ms_weights += ms[0]; tm->ms_chunk += ms[1]; tm->ms_fold += ms[2]; tm->ms_readback += ms[3];
    tm->evals += 1; tm->grad_evals += h_grad ? 1 : 0;
    return GLIA_HMT_OK;
  }
  // the gathered instance over the batch's rows (all rows without a sampler); the times of batches are the batch timing's
  int enqueue_batch(const double* d_w, const MlpBatchView& b, const double** part_S, long long* n_chunks) override {
    const long long rows = b.rows ? b.n : call.n;
    if (int rc = b.rows ? call.chunk(TermSupervisedBatch{b.rows, t}, 1, rows, d_w) : call.chunk(TermSupervised{t, call.part_L}, 1, rows, d_w)) return rc;
    *part_S = call.part_S;
    *n_chunks = (rows + kMlpTrainChunk - 1) / kMlpTrainChunk;
    return GLIA_HMT_OK;
  }
  int batch_grad(const double* h_w, const MlpBatchView& b, double* h_grad) override {
    float ms[4] = {0, 0, 0, 0};
    const double* part = nullptr;
    long long chunks = 0;
    double L;
    if (int rc = call.begin_eval(h_w)) return rc;
    if (int rc = enqueue_batch(call.w, b, &part, &chunks)) return rc;
    GLIA_HIP_TRY(call.mark(2));
    return call.finish_eval(3, &L, h_grad, ms, chunks);
  }
};

}  // namespace

int mlp_train_device_create(const double* h_X, const double* h_t, long long n, int D, int n1, int n2, int exp_variant, hipStream_t stream,
                            glia_hmt_mlp_train_timing* tm, std::unique_ptr<MlpTrainEval>* out) {
  if (n < 1 || D < 2 || D - 1 > kMlpTrainMaxDim || n1 < 0 || n2 < 0 || n1 > kMlpTrainMaxHidden || n2 > kMlpTrainMaxHidden || (n1 == 0) != (n2 == 0)) {
    set_error("mlp_train: shape outside the device trainer's limits");
    return GLIA_HMT_ERR_INTERNAL;
  }
  std::unique_ptr<MlpTrainDevice> st(new MlpTrainDevice);
  TrainCall& c = st->call;
  c.D = D; c.n1 = n1; c.n2 = n2; c.exp_variant = exp_variant; c.n = n; c.stream = stream;
  c.n_L = (n + kMlpTrainChunk - 1) / kMlpTrainChunk;
  st->tm = tm;
  const uint64_t nn = (uint64_t)n;
  c.want(&st->t, nn);
  if (int rc = c.open("mlp_train", "the call", "", &tm->device_bytes)) return rc;
  float ms = 0;
  GLIA_HIP_TRY(c.mark(0));
  GLIA_HIP_TRY(c.to_device(c.X, h_X, 8 * nn * (uint64_t)D));
  GLIA_HIP_TRY(c.to_device(st->t, h_t, 8 * nn));
  GLIA_HIP_TRY(c.mark(1));
  if (int rc = c.wait(2, &ms)) return rc;
  tm->ms_upload = ms;
  *out = std::move(st);
  return GLIA_HMT_OK;
}

}  // namespace glia
