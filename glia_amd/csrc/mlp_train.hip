// glia_amd/csrc/mlp_train.hip -- the device evaluator of the MLP / logsig trainer (the definition: mlp_backward.hpp).
//
// k_mlp_train_chunk: one workgroup per chunk of kMlpTrainChunk = 64 consecutive rows.  Phase A runs the forward and backward pass of
// the chunk's rows: the pre-activations, dh1 / dh2, dh3 and e of every row lie in LDS, unit-major ([unit][row]: the lanes of a wave are
// rows, so a wave reads and writes 64 consecutive doubles), one thread per (row, unit) for the layers and for dh1, one thread per row
// for the logit, the sigmoid and dh2.  Phase B: every thread owns weights p, p + 256, ... and walks the chunk's rows in ascending
// order, S = S - (g_i[p] * e_i); with the model's column-major layout consecutive threads read consecutive columns of a row.  The chunk
// sums go to partials [chunk][weight]; k_mlp_train_fold adds them per weight in ascending chunk order.  No atomics: the order is the
// result.  Nothing is allocated per evaluation; an evaluation reads back L and, when asked, the gradient -- the update itself is the
// header's, on the host.
#include "hmt_internal.hpp"
#include "glibc_math.hpp"
#include "mlp.hpp"
#include "mlp_backward.hpp"

namespace glia {

static_assert(kMlpTrainChunk == 64, "the chunk kernel maps one row to one lane of a wave");
constexpr int kTrainThreads = 256;

template <int NMAX>
__global__ __launch_bounds__(kTrainThreads) void k_mlp_train_chunk(const double* __restrict__ X, const double* __restrict__ tgt, long long n,
                                                                  int D, int n1, int n2, const double* __restrict__ w, long long d,
                                                                  int exp_variant, int want_grad, double* __restrict__ part_L,
                                                                  double* __restrict__ part_S) {
  constexpr int C = kMlpTrainChunk;
  __shared__ double s_h1[NMAX * C], s_h2[NMAX * C], s_dh1[NMAX * C], s_dh2[NMAX * C], s_dh3[C], s_e[C];
  const long long chunk = blockIdx.x, r0 = chunk * C;
  const int nr = (int)(n - r0 < C ? n - r0 : C);
  const int tid = threadIdx.x;
  const MlpWeights m = mlp_train_weights(w, D, n1, n2);
  const double* Xc = X + (size_t)r0 * (size_t)D;

  // ---- phase A: forward ----
  if (n1 > 0) {
    for (int q = tid; q < C * n1; q += kTrainThreads) {
      const int r = q & (C - 1), k = q >> 6;
      if (r < nr) s_h1[k * C + r] = mlp_unit(m.w0, D, 1, k, MlpRow{Xc + (size_t)r * (size_t)D});
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
    const double h3 = n1 > 0 ? mlp_unit(m.w2, n2 + 1, 1, 0, MlpActs{s_h2 + r, n2, C}) : mlp_unit(m.w2, D, 1, 0, MlpRow{Xc + (size_t)r * (size_t)D});
    const double f = glibc::sigmoid(h3, exp_variant);
    s_e[r] = mlp_sub(tgt[r0 + r], f);
    if (want_grad) {
      const double dh3 = mlp_dh3(f);
      s_dh3[r] = dh3;
      for (int k = 0; k < n2; ++k) s_dh2[k * C + r] = mlp_dh2(m, k, s_h2[k * C + r], dh3);
    }
  }
  __syncthreads();
  if (tid == 0) {
    double Lc = 0.0;
    for (int r = 0; r < nr; ++r) Lc = mlp_add(Lc, mlp_mul(s_e[r], s_e[r]));
    part_L[chunk] = Lc;
  }
  if (!want_grad) return;                  // (the same in every thread)
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
      const double e = s_e[r];
      if (mlp_feq0(e)) continue;
      const double g = mlp_grad_elem(m, p, MlpRow{Xc + (size_t)r * (size_t)D}, s_h1 + r, s_h2 + r, s_dh1 + r, s_dh2 + r, s_dh3[r], C);
      S = mlp_sub(S, mlp_mul(g, e));
    }
    out[p] = S;
  }
}

// grad[p] = the chunk sums of weight p, chunks ascending from +0.0 (threads [0, d)); L the same over part_L (thread d)
__global__ __launch_bounds__(kTrainThreads) void k_mlp_train_fold(const double* __restrict__ part_S, const double* __restrict__ part_L,
                                                                 long long n_chunks, long long d, int want_grad, double* __restrict__ grad,
                                                                 double* __restrict__ L) {
  const long long p = (long long)blockIdx.x * kTrainThreads + threadIdx.x;
  if (p == d) {
    double acc = 0.0;
    for (long long c = 0; c < n_chunks; ++c) acc = mlp_add(acc, part_L[c]);
    *L = acc;
  } else if (p < d && want_grad) {
    double acc = 0.0;
    for (long long c = 0; c < n_chunks; ++c) acc = mlp_add(acc, part_S[(size_t)c * (size_t)d + (size_t)p]);
    grad[p] = acc;
  }
}

struct MlpTrainDevice {
  int D = 0, n1 = 0, n2 = 0, exp_variant = 0;
  long long n = 0, d = 0, n_chunks = 0;
  hipStream_t stream = nullptr;
  double *X = nullptr, *t = nullptr, *w = nullptr, *part_S = nullptr, *part_L = nullptr, *out = nullptr;   // out: [d] gradient, then L
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  std::vector<double> h_out;
  glia_hmt_mlp_train_timing tm = {};
};

void mlp_train_device_free(MlpTrainDevice* st) {
  if (!st) return;
  for (double* p : {st->X, st->t, st->w, st->part_S, st->part_L, st->out}) if (p) (void)hipFree(p);
  for (hipEvent_t e : st->ev) if (e) (void)hipEventDestroy(e);
  delete st;
}

static int train_device_init(MlpTrainDevice* st, const double* h_X, const double* h_t) {
  const uint64_t n = (uint64_t)st->n, D = (uint64_t)st->D, d = (uint64_t)st->d, nc = (uint64_t)st->n_chunks;
  const uint64_t bytes = 8 * (n * D + n + d + nc * d + nc + d + 1);
  size_t free_b = 0, total_b = 0;
  GLIA_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if (bytes > (uint64_t)(0.85 * (double)free_b)) {
    set_error("mlp_train: the call needs " + std::to_string(bytes >> 20) + " MiB of device memory (rows " + std::to_string((8 * n * D) >> 20) +
              " MiB, chunk partials " + std::to_string((8 * nc * d) >> 20) + " MiB), more than 85 % of the " + std::to_string(free_b >> 20) + " MiB free");
    return GLIA_HMT_ERR_UNSUPPORTED;
  }
  st->tm.device_bytes = bytes;
  GLIA_HIP_TRY(hipMalloc(&st->X, 8 * n * D));
  GLIA_HIP_TRY(hipMalloc(&st->t, 8 * n));
  GLIA_HIP_TRY(hipMalloc(&st->w, 8 * d));
  GLIA_HIP_TRY(hipMalloc(&st->part_S, 8 * nc * d));
  GLIA_HIP_TRY(hipMalloc(&st->part_L, 8 * nc));
  GLIA_HIP_TRY(hipMalloc(&st->out, 8 * (d + 1)));
  for (hipEvent_t& e : st->ev) GLIA_HIP_TRY(hipEventCreate(&e));
  st->h_out.resize((size_t)d + 1);
  GLIA_HIP_TRY(hipEventRecord(st->ev[0], st->stream));
  GLIA_HIP_TRY(hipMemcpyAsync(st->X, h_X, 8 * n * D, hipMemcpyHostToDevice, st->stream));
  GLIA_HIP_TRY(hipMemcpyAsync(st->t, h_t, 8 * n, hipMemcpyHostToDevice, st->stream));
  GLIA_HIP_TRY(hipEventRecord(st->ev[1], st->stream));
  GLIA_HIP_TRY(hipStreamSynchronize(st->stream));
  float ms = 0;
  GLIA_HIP_TRY(hipEventElapsedTime(&ms, st->ev[0], st->ev[1]));
  st->tm.ms_upload = ms;
  return GLIA_HMT_OK;
}

int mlp_train_device_create(const double* h_X, const double* h_t, long long n, int D, int n1, int n2, int exp_variant, hipStream_t stream,
                            MlpTrainDevice** out) {
  *out = nullptr;
  if (n < 1 || D < 2 || D - 1 > kMlpTrainMaxDim || n1 < 0 || n2 < 0 || n1 > kMlpTrainMaxHidden || n2 > kMlpTrainMaxHidden || (n1 == 0) != (n2 == 0)) {
    set_error("mlp_train: shape outside the device trainer's limits");
    return GLIA_HMT_ERR_INTERNAL;
  }
  MlpTrainDevice* st = new MlpTrainDevice;
  st->D = D; st->n1 = n1; st->n2 = n2; st->exp_variant = exp_variant; st->n = n; st->stream = stream;
  st->d = mlp_train_n_weights(D, n1, n2);
  st->n_chunks = (n + kMlpTrainChunk - 1) / kMlpTrainChunk;
  if (st->n_chunks > 0x7fffffffll) { delete st; set_error("mlp_train: more than 2^31 chunks of rows"); return GLIA_HMT_ERR_UNSUPPORTED; }
  if (int rc = train_device_init(st, h_X, h_t)) { mlp_train_device_free(st); return rc; }
  *out = st;
  return GLIA_HMT_OK;
}

int mlp_train_device_eval(MlpTrainDevice* st, const double* h_w, double* L, double* h_grad) {
  const int want_grad = h_grad ? 1 : 0;
  const size_t d = (size_t)st->d;
  GLIA_HIP_TRY(hipEventRecord(st->ev[0], st->stream));
  GLIA_HIP_TRY(hipMemcpyAsync(st->w, h_w, 8 * d, hipMemcpyHostToDevice, st->stream));
  GLIA_HIP_TRY(hipEventRecord(st->ev[1], st->stream));
  const dim3 grid((unsigned)st->n_chunks), block(kTrainThreads);
  if (st->n1 <= 16 && st->n2 <= 16)
    hipLaunchKernelGGL(k_mlp_train_chunk<16>, grid, block, 0, st->stream, st->X, st->t, st->n, st->D, st->n1, st->n2, st->w, st->d, st->exp_variant,
                       want_grad, st->part_L, st->part_S);
  else
    hipLaunchKernelGGL(k_mlp_train_chunk<kMlpTrainMaxHidden>, grid, block, 0, st->stream, st->X, st->t, st->n, st->D, st->n1, st->n2, st->w, st->d,
                       st->exp_variant, want_grad, st->part_L, st->part_S);
  GLIA_HIP_TRY(hipGetLastError());
  GLIA_HIP_TRY(hipEventRecord(st->ev[2], st->stream));
  hipLaunchKernelGGL(k_mlp_train_fold, dim3((unsigned)((d + 1 + kTrainThreads - 1) / kTrainThreads)), block, 0, st->stream, st->part_S, st->part_L,
                     st->n_chunks, st->d, want_grad, st->out, st->out + d);
  GLIA_HIP_TRY(hipGetLastError());
  GLIA_HIP_TRY(hipEventRecord(st->ev[3], st->stream));
  if (want_grad) GLIA_HIP_TRY(hipMemcpyAsync(st->h_out.data(), st->out, 8 * (d + 1), hipMemcpyDeviceToHost, st->stream));
  else GLIA_HIP_TRY(hipMemcpyAsync(st->h_out.data() + d, st->out + d, 8, hipMemcpyDeviceToHost, st->stream));
  GLIA_HIP_TRY(hipEventRecord(st->ev[4], st->stream));
  GLIA_HIP_TRY(hipStreamSynchronize(st->stream));
  float ms[4] = {0, 0, 0, 0};
  for (int i = 0; i < 4; ++i) GLIA_HIP_TRY(hipEventElapsedTime(&ms[i], st->ev[i], st->ev[i + 1]));
  st->tm.ms_weights += ms[0]; st->tm.ms_chunk += ms[1]; st->tm.ms_fold += ms[2]; st->tm.ms_readback += ms[3];
  st->tm.evals += 1; st->tm.grad_evals += want_grad;
  *L = st->h_out[d];
  if (want_grad) std::copy(st->h_out.begin(), st->h_out.begin() + d, h_grad);
  return GLIA_HMT_OK;
}

void mlp_train_device_timing(const MlpTrainDevice* st, glia_hmt_mlp_train_timing* out) {
  const double total = out->ms_total;
  const int64_t it = out->iterations;
  *out = st->tm;
  out->ms_total = total; out->iterations = it;
}

}  // namespace glia
