// glia_amd/csrc/sshmt_train.hip -- the device evaluator of the merge-path (unsupervised) term (the definition:
// sshmt_paths.hpp).  Resident for the call: the prepared unlabelled rows, the path CSR, the row -> (path, slot) incidence CSR, f [N],
// e [P], q [P][8], c [N] with its named flags, the chunk partials.  Per evaluation:
//   1. k_train_chunk (mlp_train_device.hpp) without the gradient: the forward pass of every row, f to global memory;
//   2. k_sshmt_paths: one thread per path, one workgroup = one wave per chunk of kSshmtPathChunk paths: e, q and the chunk's sum of e^2;
//   3. (gradient only) k_sshmt_gather: one thread per row folds q over the row's incidence list in ascending path order -> c_r;
//   4. (gradient only) k_train_chunk with the gradient: forward and backward recomputed in LDS, then phase B with c_r as the coefficient;
//   5. k_train_fold: the chunk sums per weight in chunk order, L_U over the path chunks in chunk order.
// An L-only evaluation runs 1, 2, 5.  No atomics, no allocation per evaluation, one stream, events around every stage.
#include "mlp.hpp"
#include "mlp_train_device.hpp"
#include "sshmt_paths.hpp"

namespace glia {

static_assert(kSshmtPathChunk == 64, "a path of a chunk is a lane of one wave");
constexpr int kSshmtThreads = 256;

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

namespace {

struct SshmtTrainDevice : MlpTrainEval {
  TrainCall call;
  long long P = 0, n_path_chunks = 0;
  SshmtTables tb;
  double *f = nullptr, *e = nullptr, *q = nullptr, *c = nullptr;
  long long *offsets = nullptr, *members = nullptr, *inc_off = nullptr;
  uint32_t *inc = nullptr, *named = nullptr;
  glia_hmt_sshmt_train_timing* tm = nullptr;

  int eval(const double* h_w, double* L, double* h_grad) override {
    const int want_grad = h_grad ? 1 : 0;
    const TermPaths term{c, named, f};
    float ms[7] = {0, 0, 0, 0, 0, 0, 0};
    if (int rc = call.begin_eval(h_w)) return rc;
    if (int rc = call.chunk(term, 0)) return rc;
    GLIA_HIP_TRY(call.mark(2));
    hipLaunchKernelGGL(k_sshmt_paths, dim3((unsigned)n_path_chunks), dim3(kSshmtPathChunk), 0, call.stream, f, offsets, members, P, tb, e,
                       want_grad ? q : nullptr, call.part_L);
    GLIA_HIP_TRY(hipGetLastError());
    GLIA_HIP_TRY(call.mark(3));
    if (want_grad) {
      hipLaunchKernelGGL(k_sshmt_gather, dim3((unsigned)((call.n + kSshmtThreads - 1) / kSshmtThreads)), dim3(kSshmtThreads), 0, call.stream, inc_off,
                         inc, e, q, call.n, c, named);
      GLIA_HIP_TRY(hipGetLastError());
    }
    GLIA_HIP_TRY(call.mark(4));
    if (want_grad)
      if (int rc = call.chunk(term, 1)) return rc;
    GLIA_HIP_TRY(call.mark(5));
    if (int rc = call.finish_eval(6, L, h_grad, ms)) return rc;
    tm->ms_u_weights += ms[0]; tm->ms_u_forward += ms[1]; tm->ms_u_paths += ms[2]; tm->ms_u_gather += ms[3]; tm->ms_u_chunk += ms[4];
    tm->ms_u_fold += ms[5]; tm->ms_u_readback += ms[6];
    tm->u_evals += 1; tm->u_grad_evals += want_grad;
    return GLIA_HMT_OK;
  }
  // stages 1 to 4 over the batch's lists -- the gathered chunk kernel over the named rows, k_sshmt_paths and
  // k_sshmt_gather over the batch's own CSRs (positions in the named rows, positions in the batch); f, e, q, c and named by position
  int enqueue_batch(const double* d_w, const MlpBatchView& b, const double** part_S, long long* n_chunks) override {
    const long long rows = b.rows ? b.n : call.n, paths = b.rows ? b.P : P;
    if (paths < 1 || paths > P) { set_error("sshmt_train: a batch outside the paths"); return GLIA_HMT_ERR_INTERNAL; }
    const TermPaths term{c, named, f};
    const TermPathsBatch bterm{b.rows, term};
    if (int rc = b.rows ? call.chunk(bterm, 0, rows, d_w) : call.chunk(term, 0, rows, d_w)) return rc;
    hipLaunchKernelGGL(k_sshmt_paths, dim3((unsigned)((paths + kSshmtPathChunk - 1) / kSshmtPathChunk)), dim3(kSshmtPathChunk), 0, call.stream, f,
                       b.rows ? b.offsets : offsets, b.rows ? b.members : members, paths, tb, e, q, call.part_L);
    GLIA_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_sshmt_gather, dim3((unsigned)((rows + kSshmtThreads - 1) / kSshmtThreads)), dim3(kSshmtThreads), 0, call.stream,
                       b.rows ? b.inc_off : inc_off, b.rows ? b.inc : inc, e, q, rows, c, named);
    GLIA_HIP_TRY(hipGetLastError());
    if (int rc = b.rows ? call.chunk(bterm, 1, rows, d_w) : call.chunk(term, 1, rows, d_w)) return rc;
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

// in: at least one path, every member a row of in.X, the incidence lists built (sshmt_incidence)
int sshmt_train_device_create(const SshmtInput& in, int n1, int n2, int exp_variant, hipStream_t stream, glia_hmt_sshmt_train_timing* tm,
                              std::unique_ptr<MlpTrainEval>* out) {
  const long long n = in.n_rows, P = in.n_paths();
  const int D = in.D;
  bool ok = n >= 1 && P >= 1 && D >= 2 && D - 1 <= kMlpTrainMaxDim && n1 >= 0 && n2 >= 0 && n1 <= kMlpTrainMaxHidden && n2 <= kMlpTrainMaxHidden &&
            (n1 == 0) == (n2 == 0) && (long long)in.X.size() == n * D && (long long)in.inc_off.size() == n + 1 && in.inc.size() == in.members.size() &&
            in.offsets[0] == 0 && in.offsets[(size_t)P] == (long long)in.members.size() && in.inc_off[(size_t)n] == (long long)in.members.size();
  for (long long p = 0; ok && p < P; ++p) ok = in.offsets[p + 1] - in.offsets[p] >= 1 && in.offsets[p + 1] - in.offsets[p] <= kSshmtMaxPath;
  for (size_t k = 0; ok && k < in.members.size(); ++k) ok = in.members[k] >= 0 && in.members[k] < n && (long long)(in.inc[k] / kSshmtMaxPath) < P;
  if (!ok) { set_error("sshmt_train: input outside the device evaluator's limits"); return GLIA_HMT_ERR_INTERNAL; }
  if (P > (1ll << 28)) { set_error("sshmt_train: more than 2^28 merge paths"); return GLIA_HMT_ERR_UNSUPPORTED; }
  std::unique_ptr<SshmtTrainDevice> st(new SshmtTrainDevice);
  TrainCall& c = st->call;
  c.D = D; c.n1 = n1; c.n2 = n2; c.exp_variant = exp_variant; c.n = n; c.stream = stream;
  c.n_L = st->n_path_chunks = (P + kSshmtPathChunk - 1) / kSshmtPathChunk;
  st->P = P; st->tb = in.tb; st->tm = tm;
  tm->n_paths = P; tm->n_uns_rows = n;
  static_assert(sizeof(long long) == sizeof(int64_t), "the CSR arrays are copied as they are");
  const uint64_t N = (uint64_t)n, NP = (uint64_t)P, M = (uint64_t)in.members.size();
  c.want(&st->f, N);
  c.want(&st->e, NP);
  c.want(&st->q, NP * kSshmtMaxPath);
  c.want(&st->c, N);
  c.want(&st->offsets, NP + 1);
  c.want(&st->members, M);
  c.want(&st->inc_off, N + 1);
  c.want(&st->inc, M);
  c.want(&st->named, N);
  if (int rc = c.open("sshmt_train", "the unsupervised term", ", paths " + std::to_string((8 * (NP * (kSshmtMaxPath + 2) + 2 * M)) >> 20) + " MiB",
                      &tm->u_device_bytes))
    return rc;
  float ms = 0;
  GLIA_HIP_TRY(c.mark(0));
  GLIA_HIP_TRY(c.to_device(c.X, in.X.data(), 8 * N * (uint64_t)D));
  GLIA_HIP_TRY(c.to_device(st->offsets, in.offsets.data(), 8 * (NP + 1)));
  GLIA_HIP_TRY(c.to_device(st->members, in.members.data(), 8 * M));
  GLIA_HIP_TRY(c.to_device(st->inc_off, in.inc_off.data(), 8 * (N + 1)));
  GLIA_HIP_TRY(c.to_device(st->inc, in.inc.data(), 4 * M));
  GLIA_HIP_TRY(c.mark(1));
  if (int rc = c.wait(2, &ms)) return rc;
  tm->ms_u_upload = ms;
  *out = std::move(st);
  return GLIA_HMT_OK;
}

}  // namespace glia
