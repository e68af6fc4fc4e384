// glia_amd/csrc/mlp_batch.hip -- the mini-batch step of the MLP / logsig trainers on the device (the definition and the
// plan: mlp_batch.hpp).  The host runs the samplers ahead -- they do not depend on the weights -- and builds the plan of a whole step;
// ONE copy takes it to the device.  Then, per batch and with no wait in between: each term's evaluator enqueues its kernels over the
// batch's lists (mlp_train.hip: the gathered chunk kernel; sshmt_train.hip: the gathered forward pass, k_sshmt_paths, k_sshmt_gather,
// the gathered chunk kernel) and k_batch_step folds both terms' chunk partials in chunk order, forms g and applies the optimiser to
// w, om and ov, which stay in device memory for the step.  One wait and one read-back end the step.  No atomics; nothing is allocated
// per batch (the plan's block grows only when a step's plan outgrows it).
// GLIA_HMT_BATCH = step: the same plan, one batch per evaluation, the gradient read back and the update on the host (MlpBatchHostStep).
#include "mlp.hpp"
#include "mlp_train_device.hpp"
#include "mlp_batch.hpp"

namespace glia {

// one thread per weight: gu, gs = the chunk partials from +0.0 in ascending chunk order (k_train_fold's order), then the rule
__global__ __launch_bounds__(kTrainThreads) void k_batch_step(const double* __restrict__ part_u, long long chunks_u, const double* __restrict__ part_s,
                                                             long long chunks_s, long long d, MlpStepRule k, double step, double* __restrict__ w,
                                                             double* __restrict__ om, double* __restrict__ ov) {
  const long long p = (long long)blockIdx.x * kTrainThreads + threadIdx.x;
  if (p >= d) return;
  double gu = 0.0, gs = 0.0;
  if (k.use_u) for (long long c = 0; c < chunks_u; ++c) gu = mlp_add(gu, part_u[(size_t)c * (size_t)d + (size_t)p]);
  if (k.use_s) for (long long c = 0; c < chunks_s; ++c) gs = mlp_add(gs, part_s[(size_t)c * (size_t)d + (size_t)p]);
  double wp = w[p], m = om[p], v = ov[p];
  const double g = mlp_energy_grad_elem(k, wp, gu, gs);
  mlp_update_elem(k.optimizer, step, g, &wp, &m, &v);
  w[p] = wp; om[p] = m; ov[p] = v;
}

namespace {

struct MlpBatchDeviceStep : MlpBatchHostStep {
  hipStream_t stream = nullptr;
  int route = GLIA_HMT_BATCH_STREAM;
  long long d = 0;
  void* d_plan = nullptr;
  size_t cap = 0;
  double* d_state = nullptr;      // w [d], om [d], ov [d]
  std::vector<double> h_state;
  hipEvent_t evt[3] = {};

  ~MlpBatchDeviceStep() override {
    if (d_plan) (void)hipFree(d_plan);
    if (d_state) (void)hipFree(d_state);
    for (hipEvent_t e : evt) if (e) (void)hipEventDestroy(e);
  }
  int open() {
    for (hipEvent_t& e : evt) GLIA_HIP_TRY(hipEventCreate(&e));
    h_state.resize(3 * (size_t)d);
    return GLIA_HMT_OK;
  }
  // the plan's copy on the device: mark 0, the copy (one), enqueued on the stream that runs the kernels
  int place(const void** base) override {
    if (plan.bytes() > cap) {
      if (d_plan) { GLIA_HIP_TRY(hipStreamSynchronize(stream)); tm.syncs += 1; GLIA_HIP_TRY(hipFree(d_plan)); d_plan = nullptr; cap = 0; }
      const size_t want = 2 * plan.bytes();      // (a later step's plan differs by the rows its paths name)
      // the trainers' memory rule (train_memory_fits): the plan's block and, the first time, w, om and ov
      const size_t state = d_state ? 0 : 8 * 3 * (size_t)d;
      if (int rc = train_memory_fits((uint64_t)(want + state), "train_batches: the plan of a mini-batch step",
                                     " (plan " + std::to_string(want >> 20) + " MiB, weights and optimiser state " + std::to_string((8 * 3 * (size_t)d) >> 10) + " KiB)"))
        return rc;
      if (!d_state) GLIA_HIP_TRY(hipMalloc((void**)&d_state, state));
      GLIA_HIP_TRY(hipMalloc(&d_plan, want));
      cap = want;
    }
    GLIA_HIP_TRY(hipEventRecord(evt[0], stream));
    GLIA_HIP_TRY(hipMemcpyAsync(d_plan, plan.words.data(), plan.bytes(), hipMemcpyHostToDevice, stream));
    *base = d_plan;
    return GLIA_HMT_OK;
  }
  int run_step(const MlpStepRule& k, double step, std::vector<double>& w, std::vector<double>& om, std::vector<double>& ov) override {
    const void* base = nullptr;
    if (int rc = place(&base)) return rc;
    float ms = 0;
    if (route == GLIA_HMT_BATCH_STEP) {
      GLIA_HIP_TRY(hipEventRecord(evt[1], stream));
      const auto t0 = std::chrono::steady_clock::now();
      if (int rc = run_on_host(base, k, step, w, om, ov)) return rc;
      tm.ms_steps += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();      // (wall clock: the waits are the route)
      tm.syncs += (int64_t)plan.draws.size() * ((k.use_u ? 1 : 0) + (k.use_s ? 1 : 0));
      GLIA_HIP_TRY(hipEventElapsedTime(&ms, evt[0], evt[1]));
      tm.ms_upload += ms;
      return GLIA_HMT_OK;
    }
    const size_t nd = (size_t)d;
    std::copy(w.begin(), w.end(), h_state.begin());
    std::copy(om.begin(), om.end(), h_state.begin() + nd);
    std::copy(ov.begin(), ov.end(), h_state.begin() + 2 * nd);
    GLIA_HIP_TRY(hipMemcpyAsync(d_state, h_state.data(), 8 * 3 * nd, hipMemcpyHostToDevice, stream));
    GLIA_HIP_TRY(hipEventRecord(evt[1], stream));
    for (size_t i = 0; i < plan.draws.size(); ++i) {
      const double *part_u = nullptr, *part_s = nullptr;
      long long chunks_u = 0, chunks_s = 0;
      if (k.use_u) { if (int rc = eu->enqueue_batch(d_state, plan.uns(base, i), &part_u, &chunks_u)) return rc; }
      if (k.use_s) { if (int rc = ev->enqueue_batch(d_state, plan.sup(base, i), &part_s, &chunks_s)) return rc; }
      hipLaunchKernelGGL(k_batch_step, dim3((unsigned)((nd + kTrainThreads - 1) / kTrainThreads)), dim3(kTrainThreads), 0, stream, part_u, chunks_u, part_s,
                         chunks_s, d, k, step, d_state, d_state + nd, d_state + 2 * nd);
      GLIA_HIP_TRY(hipGetLastError());
    }
    GLIA_HIP_TRY(hipEventRecord(evt[2], stream));
    GLIA_HIP_TRY(hipMemcpyAsync(h_state.data(), d_state, 8 * 3 * nd, hipMemcpyDeviceToHost, stream));
    GLIA_HIP_TRY(hipStreamSynchronize(stream));
    tm.syncs += 1;
    std::copy(h_state.begin(), h_state.begin() + nd, w.begin());
    std::copy(h_state.begin() + nd, h_state.begin() + 2 * nd, om.begin());
    std::copy(h_state.begin() + 2 * nd, h_state.end(), ov.begin());
    GLIA_HIP_TRY(hipEventElapsedTime(&ms, evt[0], evt[1]));
    tm.ms_upload += ms;
    GLIA_HIP_TRY(hipEventElapsedTime(&ms, evt[1], evt[2]));
    tm.ms_steps += ms;
    return GLIA_HMT_OK;
  }
};

}  // namespace

int mlp_batch_device_create(hipStream_t stream, int route, long long d, std::unique_ptr<MlpBatchHostStep>* out) {
  std::unique_ptr<MlpBatchDeviceStep> st(new MlpBatchDeviceStep);
  st->stream = stream; st->route = route; st->d = d;
  st->tm.route = route;
  if (int rc = st->open()) return rc;
  *out = std::move(st);
  return GLIA_HMT_OK;
}

}  // namespace glia
