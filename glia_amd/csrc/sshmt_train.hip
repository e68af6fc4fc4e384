// glia_amd/csrc/sshmt_train.hip -- the device evaluator of the merge-path (unsupervised) term (the definition:
// sshmt_paths.hpp).  Resident for the call: the prepared unlabelled rows, the path CSR, the row -> (path, slot) incidence CSR, f [N],
// e [P], q [P][8], c [N] with its named flags, the chunk partials.  Per evaluation:
//   1. k_sshmt_chunk without partials: the forward pass of every row, f to global memory (mlp_train.hip's phase A, a row per lane);
//   2. k_sshmt_paths: one thread per path, one workgroup = one wave per chunk of kSshmtPathChunk paths: e, q and the chunk's sum of e^2;
//   3. (gradient only) k_sshmt_gather: one thread per row folds q over the row's incidence list in ascending path order -> c_r;
//   4. (gradient only) k_sshmt_chunk with partials: forward and backward recomputed in LDS, then phase B with c_r as the coefficient;
//   5. k_sshmt_fold: the chunk sums per weight in chunk order, L_U over the path chunks in chunk order.
// An L-only evaluation runs 1, 2, 5.  No atomics, no allocation per evaluation, one stream, events around every stage.
#include "hmt_internal.hpp"
#include "glibc_math.hpp"
#include "mlp.hpp"
#include "sshmt_paths.hpp"

namespace glia {

static_assert(kMlpTrainChunk == 64 && kSshmtPathChunk == 64, "a row / a path of a chunk is a lane of one wave");
constexpr int kSshmtThreads = 256;

// part_S == NULL: the forward pass alone, f_out [n].  Otherwise the chunk sums S[p] = S - (g_r[p] * c_r) over the chunk's named rows.
template <int NMAX>
__global__ __launch_bounds__(kSshmtThreads) void k_sshmt_chunk(const double* __restrict__ X, long long n, int D, int n1, int n2,
                                                              const double* __restrict__ w, long long d, int exp_variant,
                                                              const double* __restrict__ coef, const uint32_t* __restrict__ named,
                                                              double* __restrict__ f_out, double* __restrict__ part_S) {
  constexpr int C = kMlpTrainChunk;
  __shared__ double s_h1[NMAX * C], s_h2[NMAX * C], s_dh1[NMAX * C], s_dh2[NMAX * C], s_dh3[C], s_c[C];
  __shared__ uint32_t s_named[C];
  const long long chunk = blockIdx.x, r0 = chunk * C;
  const int nr = (int)(n - r0 < C ? n - r0 : C);
  const int tid = threadIdx.x;
  const MlpWeights m = mlp_train_weights(w, D, n1, n2);
  const double* Xc = X + (size_t)r0 * (size_t)D;
  const bool want_grad = part_S != nullptr;

  if (n1 > 0) {
    for (int q = tid; q < C * n1; q += kSshmtThreads) {
      const int r = q & (C - 1), k = q >> 6;
      if (r < nr) s_h1[k * C + r] = mlp_unit(m.w0, D, 1, k, MlpRow{Xc + (size_t)r * (size_t)D});
    }
    __syncthreads();
    for (int q = tid; q < C * n2; q += kSshmtThreads) {
      const int r = q & (C - 1), k = q >> 6;
      if (r < nr) s_h2[k * C + r] = mlp_unit(m.w1, n1 + 1, 1, k, MlpActs{s_h1 + r, n1, C});
    }
    __syncthreads();
  }
  if (tid < nr) {
    const int r = tid;
    const double h3 = n1 > 0 ? mlp_unit(m.w2, n2 + 1, 1, 0, MlpActs{s_h2 + r, n2, C}) : mlp_unit(m.w2, D, 1, 0, MlpRow{Xc + (size_t)r * (size_t)D});
    const double f = glibc::sigmoid(h3, exp_variant);
    if (!want_grad) f_out[r0 + r] = f;
    else {
      const double dh3 = mlp_dh3(f);
      s_dh3[r] = dh3;
      s_c[r] = coef[r0 + r];
      s_named[r] = named[r0 + r];
      for (int k = 0; k < n2; ++k) s_dh2[k * C + r] = mlp_dh2(m, k, s_h2[k * C + r], dh3);
    }
  }
  if (!want_grad) return;                  // (the same in every thread)
  __syncthreads();
  if (n1 > 0) {
    for (int q = tid; q < C * n1; q += kSshmtThreads) {
      const int r = q & (C - 1), j = q >> 6;
      if (r < nr) s_dh1[j * C + r] = mlp_dh1(m, j, s_h1[j * C + r], s_dh2 + r, C);
    }
    __syncthreads();
  }
  double* out = part_S + (size_t)chunk * (size_t)d;
  for (long long p = tid; p < d; p += kSshmtThreads) {
    double S = 0.0;
    for (int r = 0; r < nr; ++r) {
      if (!s_named[r]) continue;
      const double g = mlp_grad_elem(m, p, MlpRow{Xc + (size_t)r * (size_t)D}, s_h1 + r, s_h2 + r, s_dh1 + r, s_dh2 + r, s_dh3[r], C);
      S = mlp_sub(S, mlp_mul(g, s_c[r]));
    }
    out[p] = S;
  }
}

// one thread per path; the workgroup is the chunk.  q == NULL: e and the chunk sums alone.
__global__ __launch_bounds__(kSshmtPathChunk) void k_sshmt_paths(const double* __restrict__ f, const long long* __restrict__ offsets,
                                                                const long long* __restrict__ members, long long P, SshmtTables tb,
                                                                double* __restrict__ e, double* __restrict__ q, double* __restrict__ part_L) {
  __shared__ double s_ee[kSshmtPathChunk];
  const long long p0 = (long long)blockIdx.x * kSshmtPathChunk, p = p0 + threadIdx.x;
  if (p < P) {
    const long long o = offsets[p];
    int n = (int)(offsets[p + 1] - o);
    if (n > kSshmtMaxPath) n = kSshmtMaxPath;      // (the host never builds one)
    double fp[kSshmtMaxPath], qp[kSshmtMaxPath];
    for (int i = 0; i < kSshmtMaxPath; ++i) fp[i] = i < n ? f[members[o + i]] : 0.0;
    const double ep = sshmt_path(fp, n, tb.T[n], tb.t[n], q ? qp : nullptr);
    e[p] = ep;
    if (q) for (int i = 0; i < kSshmtMaxPath; ++i) if (i < n) q[(size_t)p * kSshmtMaxPath + i] = qp[i];
    s_ee[threadIdx.x] = mlp_mul(ep, ep);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int np = (int)(P - p0 < kSshmtPathChunk ? P - p0 : kSshmtPathChunk);
    double Lc = 0.0;
    for (int i = 0; i < np; ++i) Lc = mlp_add(Lc, s_ee[i]);
    part_L[blockIdx.x] = Lc;
  }
}

// c_r: the chain from +0.0 of q over the row's (path, slot) pairs, paths with |e| < FEPS left out; named_r: whether any is left
__global__ __launch_bounds__(kSshmtThreads) void k_sshmt_gather(const long long* __restrict__ inc_off, const uint32_t* __restrict__ inc,
                                                               const double* __restrict__ e, const double* __restrict__ q, long long n,
                                                               double* __restrict__ c, uint32_t* __restrict__ named) {
  const long long r = (long long)blockIdx.x * kSshmtThreads + threadIdx.x;
  if (r >= n) return;
  double acc = 0.0;
  uint32_t any = 0;
  for (long long k = inc_off[r]; k < inc_off[r + 1]; ++k) {
    const uint32_t i = inc[k];
    if (mlp_feq0(e[i / kSshmtMaxPath])) continue;
    acc = mlp_add(acc, q[i]);
    any = 1;
  }
  c[r] = acc;
  named[r] = any;
}

// grad[p] = the chunk sums of weight p, chunks ascending from +0.0 (threads [0, d)); L the same over the path chunks (thread d)
__global__ __launch_bounds__(kSshmtThreads) void k_sshmt_fold(const double* __restrict__ part_S, long long n_chunks, const double* __restrict__ part_L,
                                                             long long n_path_chunks, long long d, int want_grad, double* __restrict__ grad,
                                                             double* __restrict__ L) {
  const long long p = (long long)blockIdx.x * kSshmtThreads + threadIdx.x;
  if (p == d) {
    double acc = 0.0;
    for (long long c = 0; c < n_path_chunks; ++c) acc = mlp_add(acc, part_L[c]);
    *L = acc;
  } else if (p < d && want_grad) {
    double acc = 0.0;
    for (long long c = 0; c < n_chunks; ++c) acc = mlp_add(acc, part_S[(size_t)c * (size_t)d + (size_t)p]);
    grad[p] = acc;
  }
}

struct SshmtTrainDevice {
  int D = 0, n1 = 0, n2 = 0, exp_variant = 0;
  long long n = 0, P = 0, d = 0, n_chunks = 0, n_path_chunks = 0;
  SshmtTables tb;
  hipStream_t stream = nullptr;
  double *X = nullptr, *w = nullptr, *f = nullptr, *e = nullptr, *q = nullptr, *c = nullptr, *part_S = nullptr, *part_L = nullptr, *out = nullptr;
  long long *offsets = nullptr, *members = nullptr, *inc_off = nullptr;
  uint32_t *inc = nullptr, *named = nullptr;
  hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  std::vector<double> h_out;
  glia_hmt_sshmt_train_timing tm = {};
};

void sshmt_train_device_free(SshmtTrainDevice* st) {
  if (!st) return;
  for (void* p : {(void*)st->X, (void*)st->w, (void*)st->f, (void*)st->e, (void*)st->q, (void*)st->c, (void*)st->part_S, (void*)st->part_L,
                  (void*)st->out, (void*)st->offsets, (void*)st->members, (void*)st->inc_off, (void*)st->inc, (void*)st->named})
    if (p) (void)hipFree(p);
  for (hipEvent_t e : st->ev) if (e) (void)hipEventDestroy(e);
  delete st;
}

static int sshmt_device_init(SshmtTrainDevice* st, const SshmtInput& in) {
  const uint64_t n = (uint64_t)st->n, D = (uint64_t)st->D, d = (uint64_t)st->d, nc = (uint64_t)st->n_chunks, P = (uint64_t)st->P,
                 npc = (uint64_t)st->n_path_chunks, M = (uint64_t)in.members.size();
  const uint64_t bytes = 8 * (n * D + d + n + P + P * kSshmtMaxPath + n + nc * d + npc + d + 1 + (P + 1) + M + (n + 1)) + 4 * (M + n);
  size_t free_b = 0, total_b = 0;
  GLIA_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if (bytes > (uint64_t)(0.85 * (double)free_b)) {
    set_error("sshmt_train: the unsupervised term needs " + std::to_string(bytes >> 20) + " MiB of device memory (rows " + std::to_string((8 * n * D) >> 20) +
              " MiB, chunk partials " + std::to_string((8 * nc * d) >> 20) + " MiB, paths " + std::to_string((8 * (P * (kSshmtMaxPath + 2) + 2 * M)) >> 20) +
              " MiB), more than 85 % of the " + std::to_string(free_b >> 20) + " MiB free");
    return GLIA_HMT_ERR_UNSUPPORTED;
  }
  st->tm.u_device_bytes = bytes;
  GLIA_HIP_TRY(hipMalloc(&st->X, 8 * n * D));
  GLIA_HIP_TRY(hipMalloc(&st->w, 8 * d));
  GLIA_HIP_TRY(hipMalloc(&st->f, 8 * n));
  GLIA_HIP_TRY(hipMalloc(&st->e, 8 * P));
  GLIA_HIP_TRY(hipMalloc(&st->q, 8 * P * kSshmtMaxPath));
  GLIA_HIP_TRY(hipMalloc(&st->c, 8 * n));
  GLIA_HIP_TRY(hipMalloc(&st->part_S, 8 * nc * d));
  GLIA_HIP_TRY(hipMalloc(&st->part_L, 8 * npc));
  GLIA_HIP_TRY(hipMalloc(&st->out, 8 * (d + 1)));
  GLIA_HIP_TRY(hipMalloc(&st->offsets, 8 * (P + 1)));
  GLIA_HIP_TRY(hipMalloc(&st->members, 8 * M));
  GLIA_HIP_TRY(hipMalloc(&st->inc_off, 8 * (n + 1)));
  GLIA_HIP_TRY(hipMalloc(&st->inc, 4 * M));
  GLIA_HIP_TRY(hipMalloc(&st->named, 4 * n));
  for (hipEvent_t& e : st->ev) GLIA_HIP_TRY(hipEventCreate(&e));
  st->h_out.resize((size_t)d + 1);
  static_assert(sizeof(long long) == sizeof(int64_t), "the CSR arrays are copied as they are");
  GLIA_HIP_TRY(hipEventRecord(st->ev[0], st->stream));
  GLIA_HIP_TRY(hipMemcpyAsync(st->X, in.X.data(), 8 * n * D, hipMemcpyHostToDevice, st->stream));
  GLIA_HIP_TRY(hipMemcpyAsync(st->offsets, in.offsets.data(), 8 * (P + 1), hipMemcpyHostToDevice, st->stream));
  GLIA_HIP_TRY(hipMemcpyAsync(st->members, in.members.data(), 8 * M, hipMemcpyHostToDevice, st->stream));
  GLIA_HIP_TRY(hipMemcpyAsync(st->inc_off, in.inc_off.data(), 8 * (n + 1), hipMemcpyHostToDevice, st->stream));
  GLIA_HIP_TRY(hipMemcpyAsync(st->inc, in.inc.data(), 4 * M, hipMemcpyHostToDevice, st->stream));
  GLIA_HIP_TRY(hipEventRecord(st->ev[1], st->stream));
  GLIA_HIP_TRY(hipStreamSynchronize(st->stream));
  float ms = 0;
  GLIA_HIP_TRY(hipEventElapsedTime(&ms, st->ev[0], st->ev[1]));
  st->tm.ms_u_upload = ms;
  return GLIA_HMT_OK;
}

// in: at least one path, every member a row of in.X, the incidence lists built (sshmt_incidence)
int sshmt_train_device_create(const SshmtInput& in, int n1, int n2, int exp_variant, hipStream_t stream, SshmtTrainDevice** out) {
  *out = nullptr;
  const long long n = in.n_rows, P = in.n_paths();
  const int D = in.D;
  bool ok = n >= 1 && P >= 1 && D >= 2 && D - 1 <= kMlpTrainMaxDim && n1 >= 0 && n2 >= 0 && n1 <= kMlpTrainMaxHidden && n2 <= kMlpTrainMaxHidden &&
            (n1 == 0) == (n2 == 0) && (long long)in.X.size() == n * D && (long long)in.inc_off.size() == n + 1 && in.inc.size() == in.members.size() &&
            in.offsets[0] == 0 && in.offsets[(size_t)P] == (long long)in.members.size() && in.inc_off[(size_t)n] == (long long)in.members.size();
  for (long long p = 0; ok && p < P; ++p) ok = in.offsets[p + 1] - in.offsets[p] >= 1 && in.offsets[p + 1] - in.offsets[p] <= kSshmtMaxPath;
  for (size_t k = 0; ok && k < in.members.size(); ++k) ok = in.members[k] >= 0 && in.members[k] < n && (long long)(in.inc[k] / kSshmtMaxPath) < P;
  if (!ok) { set_error("sshmt_train: input outside the device evaluator's limits"); return GLIA_HMT_ERR_INTERNAL; }
  if (P > (1ll << 28)) { set_error("sshmt_train: more than 2^28 merge paths"); return GLIA_HMT_ERR_UNSUPPORTED; }
  SshmtTrainDevice* st = new SshmtTrainDevice;
  st->D = D; st->n1 = n1; st->n2 = n2; st->exp_variant = exp_variant; st->n = n; st->P = P; st->stream = stream; st->tb = in.tb;
  st->d = mlp_train_n_weights(D, n1, n2);
  st->n_chunks = (n + kMlpTrainChunk - 1) / kMlpTrainChunk;
  st->n_path_chunks = (P + kSshmtPathChunk - 1) / kSshmtPathChunk;
  st->tm.n_paths = P; st->tm.n_uns_rows = n;
  if (st->n_chunks > 0x7fffffffll) { delete st; set_error("sshmt_train: more than 2^31 chunks of rows"); return GLIA_HMT_ERR_UNSUPPORTED; }
  if (int rc = sshmt_device_init(st, in)) { sshmt_train_device_free(st); return rc; }
  *out = st;
  return GLIA_HMT_OK;
}

template <int NMAX> static void launch_chunk(SshmtTrainDevice* st, bool want_grad) {
  hipLaunchKernelGGL(k_sshmt_chunk<NMAX>, dim3((unsigned)st->n_chunks), dim3(kSshmtThreads), 0, st->stream, st->X, st->n, st->D, st->n1, st->n2, st->w,
                     st->d, st->exp_variant, st->c, st->named, st->f, want_grad ? st->part_S : nullptr);
}

int sshmt_train_device_eval(SshmtTrainDevice* st, const double* h_w, double* L, double* h_grad) {
  const int want_grad = h_grad ? 1 : 0;
  const size_t d = (size_t)st->d;
  const bool small = st->n1 <= 16 && st->n2 <= 16;
  GLIA_HIP_TRY(hipEventRecord(st->ev[0], st->stream));
  GLIA_HIP_TRY(hipMemcpyAsync(st->w, h_w, 8 * d, hipMemcpyHostToDevice, st->stream));
  GLIA_HIP_TRY(hipEventRecord(st->ev[1], st->stream));
  if (small) launch_chunk<16>(st, false); else launch_chunk<kMlpTrainMaxHidden>(st, false);
  GLIA_HIP_TRY(hipGetLastError());
  GLIA_HIP_TRY(hipEventRecord(st->ev[2], st->stream));
  hipLaunchKernelGGL(k_sshmt_paths, dim3((unsigned)st->n_path_chunks), dim3(kSshmtPathChunk), 0, st->stream, st->f, st->offsets, st->members, st->P,
                     st->tb, st->e, want_grad ? st->q : nullptr, st->part_L);
  GLIA_HIP_TRY(hipGetLastError());
  GLIA_HIP_TRY(hipEventRecord(st->ev[3], st->stream));
  if (want_grad) {
    hipLaunchKernelGGL(k_sshmt_gather, dim3((unsigned)((st->n + kSshmtThreads - 1) / kSshmtThreads)), dim3(kSshmtThreads), 0, st->stream, st->inc_off,
                       st->inc, st->e, st->q, st->n, st->c, st->named);
    GLIA_HIP_TRY(hipGetLastError());
  }
  GLIA_HIP_TRY(hipEventRecord(st->ev[4], st->stream));
  if (want_grad) {
    if (small) launch_chunk<16>(st, true); else launch_chunk<kMlpTrainMaxHidden>(st, true);
    GLIA_HIP_TRY(hipGetLastError());
  }
  GLIA_HIP_TRY(hipEventRecord(st->ev[5], st->stream));
  hipLaunchKernelGGL(k_sshmt_fold, dim3((unsigned)((d + 1 + kSshmtThreads - 1) / kSshmtThreads)), dim3(kSshmtThreads), 0, st->stream, st->part_S,
                     st->n_chunks, st->part_L, st->n_path_chunks, st->d, want_grad, st->out, st->out + d);
  GLIA_HIP_TRY(hipGetLastError());
  GLIA_HIP_TRY(hipEventRecord(st->ev[6], st->stream));
  if (want_grad) GLIA_HIP_TRY(hipMemcpyAsync(st->h_out.data(), st->out, 8 * (d + 1), hipMemcpyDeviceToHost, st->stream));
  else GLIA_HIP_TRY(hipMemcpyAsync(st->h_out.data() + d, st->out + d, 8, hipMemcpyDeviceToHost, st->stream));
  GLIA_HIP_TRY(hipEventRecord(st->ev[7], st->stream));
  GLIA_HIP_TRY(hipStreamSynchronize(st->stream));
  float ms[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 7; ++i) GLIA_HIP_TRY(hipEventElapsedTime(&ms[i], st->ev[i], st->ev[i + 1]));
  st->tm.ms_u_weights += ms[0]; st->tm.ms_u_forward += ms[1]; st->tm.ms_u_paths += ms[2]; st->tm.ms_u_gather += ms[3]; st->tm.ms_u_chunk += ms[4];
  st->tm.ms_u_fold += ms[5]; st->tm.ms_u_readback += ms[6];
  st->tm.u_evals += 1; st->tm.u_grad_evals += want_grad;
  *L = st->h_out[d];
  if (want_grad) std::copy(st->h_out.begin(), st->h_out.begin() + d, h_grad);
  return GLIA_HMT_OK;
}

// the unsupervised evaluator's fields of *out; out->sup is the caller's
void sshmt_train_device_timing(const SshmtTrainDevice* st, glia_hmt_sshmt_train_timing* out) {
  const glia_hmt_mlp_train_timing sup = out->sup;
  *out = st->tm;
  out->sup = sup;
}

}  // namespace glia
