// glia_amd/csrc/forest_predict.hip -- the classifier over a batch of feature rows (ml/rf/main_pred_rf.cxx:13-40: alg::RandomForest /
// alg::EnsembleRandomForest::operator() per row, alg/rf.hxx; opt::ThresholdModelDistributor, type/function.hxx:71-85).
//
// A THROUGHPUT kernel, unlike the walks of the classifier loop (greedy_bc.hip), which wait for one vector at a time.  A workgroup of
// 256 threads takes a tile of TR rows (TR = 64, 32, 16 or 8: the largest whose rows fit the staging budget) and stages it in LDS with a
// row stride that is an ODD number of doubles, so the 32 lanes of a ds_read_b64 group that read one column of 32 rows hit 32 different
// bank pairs.  thread = (row, slot): row = tid % TR, slot = tid / TR; the 256 / TR slots split the trees (slot, slot + slots, ...), so a
// tile of 64 rows is walked by four waves, one of 8 rows by 32 row groups -- also when the whole input is one tile.  The lanes of one
// slot walk the same tree: near its root they read the same 16-byte node (PackedNode is breadth-first, a level's nodes are contiguous).
// A lane that finishes a tree goes on with its next one (no waiting for the deepest walk of the wave) and keeps two walks in flight.
// Every thread counts its votes in an integer; the slots' counts meet in LDS and the thread of slot 0 adds them and writes
// votes / ntree -- no float atomics, no global atomics, and integers add in any order: the result is bit-exact.
// A row too long to stage (dim > GLIA_HMT_PREDICT_STAGE_MAX_DIM) is walked from global memory, as is the one-column read of the stub.
#include <cstddef>

#include "forest.hpp"

namespace glia {

namespace {

static_assert(sizeof(PackedNode) == 16 && offsetof(PackedNode, var) == 8 && offsetof(PackedNode, left) == 12, "lane_votes reads a node as one uint4");
constexpr int kThreads = 256;
constexpr int kStageBytes = 48 * 1024;                 // row tile in LDS: three workgroups per compute unit
constexpr int kMinTile = 8;
constexpr long long kMaxBlocks = 1ll << 23;           // workgroups per launch: 2^31 threads
static_assert(((GLIA_HMT_PREDICT_STAGE_MAX_DIM | 1) * kMinTile * 8) <= kStageBytes, "the longest staged row fits the smallest tile");
static_assert((((GLIA_HMT_PREDICT_STAGE_MAX_DIM + 1) | 1) * kMinTile * 8) > kStageBytes, "GLIA_HMT_PREDICT_STAGE_MAX_DIM is the limit");

// One lane's walks over its trees t0, t0 + stride, ...: the project's rule -- left iff x[var] <= split, so a NaN goes
// right; a walk that has read nrnodes nodes without meeting a terminal one votes 0, as forest_vote does.  A lane that reaches a leaf
// starts its next tree at once instead of waiting for the deepest walk of its wave, and it keeps TWO walks in flight (trees t0 and
// t0 + stride, then every second one each), so that two node loads of a lane are outstanding at a time.
struct Walk { int t, k, steps; };
template <typename X> __device__ __forceinline__ int lane_votes(const DeviceForest& f, int t0, int stride, const X x) {
  const uint4* const nodes = reinterpret_cast<const uint4*>(f.nodes);       // one 16-byte load per level (PackedNode: split, var, left)
  const int ntree = f.ntree, nrnodes = f.nrnodes;
  int votes = 0;
  auto start = [&](Walk& w, int t) { w.t = t; w.steps = 0; w.k = t < ntree ? f.root[t] : 0; };
  auto advance = [&](Walk& w, const uint4 q) {
    const int var = (int)q.z;
    ++w.steps;
    if (var < 0) { votes += -1 - var; start(w, w.t + 2 * stride); }
    else if (w.steps >= nrnodes) start(w, w.t + 2 * stride);
    else w.k = (int)q.w + ((x[var] <= __hiloint2double((int)q.y, (int)q.x)) ? 0 : 1);
  };
  Walk a, b;
  start(a, t0);
  start(b, t0 + stride);
  for (;;) {
    const bool la = a.t < ntree, lb = b.t < ntree;
    if (!la && !lb) break;
    const uint4 qa = nodes[la ? a.k : 0], qb = nodes[lb ? b.k : 0];       // node 0 exists in every forest
    if (la) advance(a, qa);
    if (lb) advance(b, qb);
  }
  return votes;
}

template <bool STAGED>
__global__ __launch_bounds__(kThreads) void forest_predict_kernel(const DeviceClassifier clf, const double* __restrict__ rows, long long n_rows,
                                                                  int dim, long long row_stride, int TR, int S, double* __restrict__ pred) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x;
  const long long row0 = (long long)blockIdx.x * TR;
  const int have = (int)(n_rows - row0 < TR ? n_rows - row0 : TR);          // rows of this tile, >= 1
  int* const counts = reinterpret_cast<int*>(lds + (STAGED ? (size_t)TR * S : 0));   // [kThreads]
  if (STAGED) {
    // wave w copies rows w, w + 4, ...: 64 consecutive doubles per load
    for (int r = tid >> 6; r < have; r += kThreads / 64) {
      const double* src = rows + (row0 + r) * row_stride;
      for (int c = tid & 63; c < dim; c += 64) lds[(size_t)r * S + c] = src[c];
    }
    __syncthreads();
  }
  const int row = tid % TR, slot = tid / TR, slots = kThreads / TR;
  int votes = 0, ntree = 1;
  if (row < have) {
    const double* x = STAGED ? lds + (size_t)row * S : rows + (row0 + row) * row_stride;
    int m = 0;
    if (clf.n_models != 1) m = x[clf.dim1] < clf.threshold ? 0 : (x[clf.dim0] < clf.threshold ? 1 : 2);   // type/function.hxx:80-84
    const DeviceForest& f = clf.f[m];
    ntree = f.ntree;
    votes = lane_votes(f, slot, slots, x);
  }
  counts[tid] = votes;
  __syncthreads();
  if (slot == 0 && row < have) {
    int sum = 0;
    for (int s = 0; s < slots; ++s) sum += counts[s * TR + row];
    pred[row0 + row] = (double)sum / (double)ntree;                          // ml/rf/rf.hxx:366-369
  }
}

__global__ void stub_predict_kernel(int index, const double* __restrict__ rows, long long n_rows, long long row_stride, double* __restrict__ pred) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_rows) pred[i] = 1.0 - rows[i * row_stride + index];
}

}  // namespace

// rows of a tile: the largest power of two <= 64 whose rows fit the staging budget; a small input takes smaller tiles (down to 16 rows)
// so that its walks spread over more compute units.  0: the row is too long to stage.
int forest_predict_tile_rows(long long n_rows, int dim) {
  const int S = dim | 1;
  if ((long long)S * kMinTile * 8 > kStageBytes) return 0;
  int tr = 64;
  while (tr > kMinTile && (long long)S * tr * 8 > kStageBytes) tr >>= 1;
  while (tr > 16 && (n_rows + tr - 1) / tr < 512) tr >>= 1;
  return tr;
}

int launch_forest_predict(const DeviceClassifier& clf, const double* d_rows, long long n_rows, int dim, long long row_stride, double* d_pred,
                          hipStream_t stream) {
  if (n_rows <= 0) return GLIA_HMT_OK;
  if (clf.kind == 1) {
    for (long long r0 = 0; r0 < n_rows; r0 += kMaxBlocks * 256) {
      const long long n = n_rows - r0 < kMaxBlocks * 256 ? n_rows - r0 : kMaxBlocks * 256;
      stub_predict_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(clf.stub_index, d_rows + r0 * row_stride, n, row_stride, d_pred + r0);
      GLIA_HIP_TRY(hipGetLastError());
    }
    return GLIA_HMT_OK;
  }
  const int S = dim | 1;
  int TR = forest_predict_tile_rows(n_rows, dim);
  const bool staged = TR > 0;
  if (!staged) TR = 64;
  const size_t shmem = (staged ? (size_t)TR * S * sizeof(double) : 0) + kThreads * sizeof(int);
  // at most kMaxBlocks workgroups (2^31 threads) per launch: more rows take further launches
  for (long long r0 = 0; r0 < n_rows; r0 += kMaxBlocks * TR) {
    const long long n = n_rows - r0 < kMaxBlocks * TR ? n_rows - r0 : kMaxBlocks * TR;
    const dim3 grid((unsigned)((n + TR - 1) / TR));
    const double* rows = d_rows + r0 * row_stride;
    if (staged) forest_predict_kernel<true><<<grid, dim3(kThreads), shmem, stream>>>(clf, rows, n, dim, row_stride, TR, S, d_pred + r0);
    else forest_predict_kernel<false><<<grid, dim3(kThreads), shmem, stream>>>(clf, rows, n, dim, row_stride, TR, S, d_pred + r0);
    GLIA_HIP_TRY(hipGetLastError());
  }
  return GLIA_HMT_OK;
}

}  // namespace glia
