// glia_amd/csrc/median_init.hip -- GLIA_USE_MEDIAN_AS_FEATS for the INITIAL edges (TBoundaryTable::init).
//
// Both regions of an initial edge are leaves, so every value multiset its row looks at (median_feats.hip has the list) is fixed by
// the region map.  Instead of gathering and sorting every set afresh, each listed image is sorted ONCE, O(volume):
//   * region image: voxel values grouped by leaf (mf_scatter_regions), one segmented radix sort with one segment per leaf;
//   * boundary image: boundary-voxel values grouped by directed pair (mf_scatter_pairs), one segment per pair; the pairs ascend by
//     (a, b), so the runs leaving one leaf are adjacent: entries le_start[u] .. le_start[u + 1];
//   * per run: n (from the offsets), the f64 sum and the f64 sum of squared deviations from the run's own mean (M2).
// The sets of a table edge (u, v) -- mutual: u -> v and v -> u both exist -- are then lists of runs:
//   P(u), P(v) one run each; P(u + v) two runs; B(u), B(v) every run leaving the leaf (non-mutual ones included, TRegion::merge,
//   type/region.hxx:66-75); Sh(u, v) = (u -> v) + (v -> u); B(u + v) = B(u) + B(v) - (u -> v) - (v -> u), a multiset difference.
// median = stats::amedian = the element at rank n / 2 (util/stats.hxx:83-91), selected over the runs (median_select.hpp): the same
// f32 as sorted[n / 2] of the materialised set, the radix sort's order being the ordering rule (-0.0 below +0.0, as in bc_feat).
// mean = sum of the run sums / n; stddev from  sum (x - m)^2 = sum over runs of M2_r + n_r (mean_r - m)^2  -- non-negative terms
// only: the two runs B(u + v) leaves out are skipped there, not subtracted.  An empty set gives 0 (feat.hxx:708-709).
//
// Kernels: one thread per record for the region sets (at most two runs), one wave per boundary set with one lane per run (a loop
// when a leaf has more than 64 neighbours).  No wave hands data to another: no workgroup barrier anywhere.
// Memory per image in flight: 4 B per voxel (boundary image: per boundary voxel) for the grouped values + the same again for the
// sort's second buffer + rocPRIM's scratch; 16 B per run; 8 B per leaf and per pair for the offsets.  Sizes stay below 2^32 values
// per image (rocPRIM's segmented sort counts in 32 bits).
#include <cmath>

#include "median_runs.hpp"

namespace glia {

namespace {

constexpr int kWave = 64;

__global__ void mi_counts(const uint32_t* rec, long long n, int words, int word, uint32_t* out) {   // out[n] = 0: the scan's last offset
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= n) out[i] = i < n ? rec[(size_t)i * words + word] : 0u;
}

__device__ __forceinline__ double wave_sum(double x) {
  for (int d = kWave / 2; d >= 1; d >>= 1) x += __shfl_xor(x, d, kWave);
  return x;
}
__device__ __forceinline__ long long wave_sum(long long x) {
  for (int d = kWave / 2; d >= 1; d >>= 1) x += __shfl_xor(x, d, kWave);
  return x;
}
struct SelectWave { __device__ long long operator()(long long c) const { return wave_sum(c); } };

// (sum, M2) of every sorted run, one wave per run (the order of the additions is fixed: the result does not depend on the launch)
__global__ __launch_bounds__(256) void mi_run_stats(const float* sorted, const unsigned long long* off, long long n_runs, double2* out) {
  const long long r = (long long)blockIdx.x * (256 / kWave) + threadIdx.x / kWave;
  if (r >= n_runs) return;                                       // (whole waves leave together)
  const int lane = threadIdx.x % kWave;
  const unsigned long long b = off[r], e = off[r + 1];
  double acc = 0.0;
  for (unsigned long long i = b + lane; i < e; i += kWave) acc += (double)sorted[i];
  const double sum = wave_sum(acc);
  const double mean = e > b ? sum / (double)(e - b) : 0.0;
  acc = 0.0;
  for (unsigned long long i = b + lane; i < e; i += kWave) { const double dx = (double)sorted[i] - mean; acc += dx * dx; }
  const double m2 = wave_sum(acc);
  if (lane == 0) out[r] = make_double2(sum, m2);
}

__device__ __forceinline__ void put3(double* out, double med, double mean, double m2, unsigned long long n) {
  const double var = n ? m2 / (double)n : 0.0;                   // stats::var (util/stats.hxx:60-69)
  out[0] = med; out[1] = mean; out[2] = var >= 0.0 ? sqrt(var) : 0.0;
}
__device__ __forceinline__ bool mi_wanted(const MedianInitRecords& rec, uint32_t e) { return rec.e_table[e] && e % rec.n_shards == rec.shard; }

// P(u), P(v), P(u + v) of image c for the records [e0, e1): one thread per record
__global__ void mi_region_sets(MedianInitRecords rec, uint32_t e0, uint32_t e1, const float* sorted, const unsigned long long* off, const double2* rs,
                               int n_r, int c, double* reg) {
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= e1 - e0) return;
  const uint32_t e = e0 + slot;
  if (!mi_wanted(rec, e)) return;
  const uint32_t leaf[2] = {rec.e_u[e], rec.e_v[e]};
  SignedRun run[2];
  double sum[2], m2[2], mean[2];
  for (int k = 0; k < 2; ++k) {
    const unsigned long long b = off[leaf[k]], n = off[leaf[k] + 1] - b;
    run[k] = SignedRun{sorted + b, n, 1};
    sum[k] = rs[leaf[k]].x; m2[k] = rs[leaf[k]].y;
    mean[k] = n ? sum[k] / (double)n : 0.0;
    put3(&reg[(((size_t)slot * 3 + k) * n_r + c) * 3], n ? (double)sorted[b + n / 2] : 0.0, mean[k], m2[k], n);
  }
  const unsigned long long n = run[0].n + run[1].n;
  const double m = n ? (sum[0] + sum[1]) / (double)n : 0.0;
  const double d0 = mean[0] - m, d1 = mean[1] - m;
  const double M2 = (m2[0] + (double)run[0].n * (d0 * d0)) + (m2[1] + (double)run[1].n * (d1 * d1));
  const double med = n ? (double)median_select(RunList{run, 2}, (long long)(n / 2), SelectAlone()) : 0.0;
  put3(&reg[(((size_t)slot * 3 + 2) * n_r + c) * 3], med, m, M2, n);
}

// The runs of one boundary set dealt out to the lanes of a wave: lane l looks at the runs l, l + 64, ... of the list
//   [b0, b0 + n0) (+)  |  [b1, b1 + n1) (+)  |  neg0 (-)  |  neg1 (-)          (entry indices; kNone = no such run)
struct BoundaryRuns {
  const float* sorted; const unsigned long long* off;
  uint32_t b0, n0, b1, n1, neg0, neg1, lane;
  __device__ uint32_t total() const { return n0 + n1 + (neg0 != kNone ? 1u : 0u) + (neg1 != kNone ? 1u : 0u); }
  __device__ int count() const { const uint32_t t = total(); return t > lane ? (int)((t - lane + kWave - 1) / kWave) : 0; }
  __device__ uint32_t entry(int i, int* sign) const {
    const uint32_t j = lane + (uint32_t)i * kWave;
    *sign = j < n0 + n1 ? 1 : -1;
    return j < n0 ? b0 + j : j < n0 + n1 ? b1 + (j - n0) : (j == n0 + n1 && neg0 != kNone) ? neg0 : neg1;
  }
  __device__ SignedRun get(int i) const {
    int sign;
    const uint32_t en = entry(i, &sign);
    return SignedRun{sorted + off[en], off[en + 1] - off[en], sign};
  }
};

// the entry (u -> v) among u's entries (ascending by target), kNone when absent
__device__ __forceinline__ uint32_t mi_find_entry(const MedianInitRecords& rec, uint32_t u, uint32_t v) {
  uint32_t lo = rec.le_start[u], hi = rec.le_start[u + 1];
  const uint32_t end = hi;
  while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (rec.le_dst[mid] < v) lo = mid + 1; else hi = mid; }
  return (lo < end && rec.le_dst[lo] == v) ? lo : kNone;
}

// B(u), B(v), B(u + v), Sh(u, v) of image c for the records [e0, e1): one wave per set, four waves (one workgroup) per record
__global__ __launch_bounds__(4 * kWave) void mi_boundary_sets(MedianInitRecords rec, uint32_t e0, const float* sorted, const unsigned long long* off, const double2* rs,
                                                              int n_b, int c, double* bnd) {
  const uint32_t slot = blockIdx.x, e = e0 + slot;
  if (!mi_wanted(rec, e)) return;
  const int k = threadIdx.x / kWave;                             // which set (wave-uniform)
  const uint32_t u = rec.e_u[e], v = rec.e_v[e];
  const uint32_t bu = rec.le_start[u], nu = rec.le_start[u + 1] - bu, bv = rec.le_start[v], nv = rec.le_start[v + 1] - bv;
  BoundaryRuns runs{sorted, off, 0, 0, 0, 0, kNone, kNone, threadIdx.x % kWave};
  if (k == 0) { runs.b0 = bu; runs.n0 = nu; }
  else if (k == 1) { runs.b0 = bv; runs.n0 = nv; }
  else {
    const uint32_t uv = mi_find_entry(rec, u, v), vu = mi_find_entry(rec, v, u);    // (a table edge has both)
    if (k == 2) { runs.b0 = bu; runs.n0 = nu; runs.b1 = bv; runs.n1 = nv; runs.neg0 = uv; runs.neg1 = vu; }
    else { if (uv != kNone) { runs.b0 = uv; runs.n0 = 1; } if (vu != kNone) { runs.b1 = vu; runs.n1 = 1; } }
  }
  // n and sum, then M2 about the set's mean; a run the difference takes out again contributes to neither (on both of its appearances)
  const int mine = runs.count();
  auto counted = [&](uint32_t en, int sign) { return sign > 0 && en != runs.neg0 && en != runs.neg1; };
  long long n_part = 0;
  double s_part = 0.0;
  for (int i = 0; i < mine; ++i) {
    int sign;
    const uint32_t en = runs.entry(i, &sign);
    if (counted(en, sign)) { n_part += (long long)(off[en + 1] - off[en]); s_part += rs[en].x; }
  }
  const long long n = wave_sum(n_part);
  const double sum = wave_sum(s_part);
  const double m = n ? sum / (double)n : 0.0;
  double q_part = 0.0;
  for (int i = 0; i < mine; ++i) {
    int sign;
    const uint32_t en = runs.entry(i, &sign);
    const unsigned long long nr = off[en + 1] - off[en];
    if (counted(en, sign) && nr) { const double d = rs[en].x / (double)nr - m; q_part += rs[en].y + (double)nr * (d * d); }
  }
  const double M2 = wave_sum(q_part);
  const double med = n ? (double)median_select(runs, n / 2, SelectWave()) : 0.0;    // (n is wave-uniform: all lanes or none)
  if (threadIdx.x % kWave == 0) put3(&bnd[(((size_t)slot * 4 + k) * n_b + c) * 3], med, m, M2, (unsigned long long)n);
}

struct StageTimer {                 // device time of a stage, added up over the images
  hipEvent_t a = nullptr, b = nullptr;
  ~StageTimer() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
  int create() { GLIA_HIP_TRY(hipEventCreate(&a)); GLIA_HIP_TRY(hipEventCreate(&b)); return GLIA_HMT_OK; }
};

}  // namespace

int median_init_stats(const MedianFeatIn& in, const MedianInitRecords& rec, uint32_t e0, uint32_t e1, hipStream_t stream, double* d_reg, double* d_bnd,
                      MedianInitTiming* timing) {
  const RagArrays& rag = *in.rag;
  const long long R = rag.R, P = rag.P;
  const long long N = in.vol.nx * in.vol.ny * in.vol.nz;
  if (!in.vol.lab) { set_error("score_initial_edges (median features): needs the volumes the region map was built from (whole-volume build)"); return GLIA_HMT_ERR_UNSUPPORTED; }
  if (e1 <= e0 || R == 0) return GLIA_HMT_OK;
  const uint32_t n_rec = e1 - e0;
  DeviceBuffers buf;
  StageTimer ts, tq;
  int rc;
  if ((rc = ts.create()) || (rc = tq.create())) return rc;
  float ms;
  // the runs of one kind of image: kind 0 = leaves (region images), 1 = directed pairs (boundary images)
  for (int kind = 0; kind < 2; ++kind) {
    const int n_img = kind == 0 ? in.n_r : in.n_b;
    const long long n_runs = kind == 0 ? R : P;
    if (n_img <= 0 || n_runs == 0) continue;
    uint32_t* d_cnt; unsigned long long* d_off; uint32_t* d_cursor; double2* d_rs;
    if ((rc = buf.get(&d_cnt, (size_t)n_runs + 1, false, stream)) || (rc = buf.get(&d_off, (size_t)n_runs + 1, false, stream)) ||
        (rc = buf.get(&d_cursor, (size_t)n_runs, false, stream)) || (rc = buf.get(&d_rs, (size_t)n_runs, false, stream))) return rc;
    const unsigned g_runs = (unsigned)((n_runs + 256) / 256);
    if (kind == 0) hipLaunchKernelGGL(mi_counts, dim3(g_runs), dim3(256), 0, stream, rag.d_rrec, R, kRegionWords, R_CNT, d_cnt);
    else hipLaunchKernelGGL(mi_counts, dim3(g_runs), dim3(256), 0, stream, rag.d_prec, P, kPairWords, P_CNT, d_cnt);
    if ((rc = rocprim_run(buf, stream, [&](void* t, size_t& b) {
          return rocprim::exclusive_scan(t, b, d_cnt, d_off, 0ull, (size_t)n_runs + 1, rocprim::plus<unsigned long long>(), stream); }))) return rc;
    unsigned long long total = 0;
    GLIA_HIP_TRY(hipMemcpyAsync(&total, d_off + n_runs, sizeof(total), hipMemcpyDeviceToHost, stream));
    GLIA_HIP_TRY(hipStreamSynchronize(stream));
    if (total >= (1ull << 32)) {
      set_error("score_initial_edges (median features): " + std::to_string(total) + (kind == 0 ? " voxel" : " boundary-voxel") + " values in one image, the sort is bounded by 2^32");
      return GLIA_HMT_ERR_UNSUPPORTED;
    }
    float *d_a, *d_b;
    if ((rc = buf.get(&d_a, (size_t)total, false, stream)) || (rc = buf.get(&d_b, (size_t)total, false, stream))) return rc;
    size_t sort_bytes = 0;                              // rocPRIM's scratch: sized once, the same for every image of this kind
    char* d_tmp = nullptr;
    if (total) GLIA_HIP_TRY(rocprim::segmented_radix_sort_keys(nullptr, sort_bytes, d_a, d_b, (unsigned)total, (unsigned)n_runs, d_off, d_off + 1, 0, 32, stream));
    if ((rc = buf.get(&d_tmp, sort_bytes ? sort_bytes : 16, false, stream))) return rc;
    for (int c = 0; c < n_img; ++c) {
      GLIA_HIP_TRY(hipEventRecord(ts.a, stream));
      GLIA_HIP_TRY(hipMemsetAsync(d_cursor, 0, sizeof(uint32_t) * (size_t)n_runs, stream));
      if (kind == 0) hipLaunchKernelGGL(mf_scatter_regions, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, in.vol, in.r_img[c], rag.d_rlabel, (uint32_t)R, d_off, d_cursor, d_a);
      else hipLaunchKernelGGL(mf_scatter_pairs, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, in.vol, in.b_img[c], rag.d_pa, rag.d_pb, P, d_off, d_cursor, d_a);
      GLIA_HIP_TRY(hipGetLastError());
      if (total) GLIA_HIP_TRY(rocprim::segmented_radix_sort_keys((void*)d_tmp, sort_bytes, d_a, d_b, (unsigned)total, (unsigned)n_runs, d_off, d_off + 1, 0, 32, stream));
      hipLaunchKernelGGL(mi_run_stats, dim3((unsigned)((n_runs + 3) / 4)), dim3(256), 0, stream, d_b, d_off, n_runs, d_rs);
      GLIA_HIP_TRY(hipEventRecord(ts.b, stream));
      GLIA_HIP_TRY(hipEventRecord(tq.a, stream));
      if (kind == 0) hipLaunchKernelGGL(mi_region_sets, dim3((n_rec + 127) / 128), dim3(128), 0, stream, rec, e0, e1, d_b, d_off, d_rs, in.n_r, c, d_reg);
      else hipLaunchKernelGGL(mi_boundary_sets, dim3(n_rec), dim3(4 * kWave), 0, stream, rec, e0, d_b, d_off, d_rs, in.n_b, c, d_bnd);
      GLIA_HIP_TRY(hipGetLastError());
      GLIA_HIP_TRY(hipEventRecord(tq.b, stream));
      GLIA_HIP_TRY(hipEventSynchronize(tq.b));
      if (timing) {
        GLIA_HIP_TRY(hipEventElapsedTime(&ms, ts.a, ts.b)); timing->ms_sort += ms;
        GLIA_HIP_TRY(hipEventElapsedTime(&ms, tq.a, tq.b)); timing->ms_select += ms;
      }
    }
  }
  if (timing) { unsigned long long b = 0; for (size_t s : buf.sizes) b += s; if (b > timing->bytes) timing->bytes = b; }
  return GLIA_HMT_OK;
}

}  // namespace glia
