// glia_amd/csrc/mlp_predict.hip -- the MLP / logsig classifier over a batch of feature rows (sshmt/main_pred_mlp.cxx:18-48: stats::rescale,
// the appended 1, alg::MLP2v / alg::EnsembleMLP2v::operator(), alg/nn.hxx:52-71,227-230; sshmt/main_pred_logsig.cxx:12-32).
//
// A THROUGHPUT kernel in the manner of forest_predict.hip.  The arithmetic is mlp_model.hpp's: every dot product is one
// chain, j ascending, multiply and add rounded separately -- so no v_mfma_f64 (its summation order is not specified) and no split of a
// dot product over lanes.  Parallelism is over rows and over hidden units:
//   * a workgroup of kMlpSlots = 4 waves takes a tile of TR rows; lane = row, wave = slot.  Each row of the tile has `stride` doubles of LDS, an
//     ODD number, so the 32 lanes of a ds_read_b64 group that read one column of 32 rows hit 32 different bank pairs.
//   * staging rescales the row, appends the 1.0 and writes it to region A of its LDS row (a row too long for that is rescaled again by
//     every wave as it reads it from global memory); every thread picks its row's model from the rescaled vector.
//   * a layer's units are cut into blocks of UB <= 16 (mlp_unit_block: the layer split evenly over the 4 slots); slot s takes blocks
//     s, s + 4, ...  A thread keeps the UB sums of its row in registers and walks j once per block: one LDS read and UB multiply-add
//     pairs per j.  The weights of a block lie as [j][UB] (mlp_block_weights), the slot is wave-uniform, so they arrive through scalar
//     loads and are VALU operands from SGPRs.
//   * layer 1 reads region A (the row) and writes region B; a barrier; layer 2 reads B and writes A (the row is dead by then); a
//     barrier; the threads of slot 0 sum the logit from A and write the outputs.
//   * the compact tile (both layers of at most 4 * 16 units: one block per slot): a slot keeps its block's activations in registers
//     until every wave is done reading the layer's input, then they overwrite it -- one region of max(row, layer) doubles per row
//     instead of two, so 64 rows of 104 columns fit three workgroups into a compute unit's LDS.
//   * an ensemble: a wave runs a block once per model that one of its rows picked (a wave-uniform branch, weights stay uniform);
//     a thread keeps the sums of its own model only.
// TR < 64 (layers too wide for 64 LDS rows) leaves the upper lanes of every wave idle: correct, not fast.
#include <cstddef>

#include "mlp.hpp"

namespace glia {

namespace {

constexpr int kThreads = 64 * kMlpSlots;
constexpr long long kMaxBlocks = 1ll << 23;           // workgroups per launch
constexpr int kStageBatch = 8;

struct LdsRow {
  const double* p;
  __device__ __forceinline__ double operator()(int j) const { return p[j]; }
};
// stats::rescale with the denominator (max - min) + FEPS taken from the table the host computed: the same operations, each rounded once
__device__ __forceinline__ double rescaled(double v, double mn, double den) { return __dadd_rn(__ddiv_rn(__dmul_rn(2.0, __dsub_rn(v, mn)), den), -1.0); }
// a row in global memory: rescaled on the way, the bias appended
struct GlobalRow {
  const double* p;
  const double* mn;
  const double* den;
  int dim, rescale;
  __device__ __forceinline__ double operator()(int j) const {
    if (j >= dim) return 1.0;
    const double v = p[j];
    return rescale ? rescaled(v, mn[j], den[j]) : v;
  }
};

// The blocks slot, slot + kMlpSlots, ... of a layer with din inputs and n_out units: relu(sum_j in(j) * w[k][j]) of a thread's own model
// (`mine`).  DEFER = false: stored to out[k].  DEFER = true (the compact tile: at most one block per slot, and `out` overlays the
// layer's input): kept in keep[0 .. UB), for the caller to store once every wave is done reading.
template <int UB, bool DEFER, typename In>
__device__ __forceinline__ void layer_blocks(const double* __restrict__ w, int nb, int din, int n_out, int slot, const In in, double* out, bool mine,
                                             double (&keep)[kMlpUnitBlock]) {
  constexpr int kUnroll = UB <= 4 ? 8 : (UB <= 8 ? 4 : 2);                  // j's whose weights are fetched together: <= 64 SGPRs
  for (int b = slot; b < nb; b += kMlpSlots) {
    double acc[UB];
#pragma unroll
    for (int u = 0; u < UB; ++u) acc[u] = 0.0;
    const double* __restrict__ wb = w + (size_t)b * din * UB;
#pragma unroll kUnroll
    for (int j = 0; j < din; ++j) {
      const double x = in(j);
#pragma unroll
      for (int u = 0; u < UB; ++u) acc[u] = __dadd_rn(acc[u], __dmul_rn(x, wb[(size_t)j * UB + u]));
    }
    if (mine) {
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const int k = b * UB + u;
        const double a = acc[u] > 0.0 ? acc[u] : 0.0;                        // a NaN becomes 0
        if (DEFER) keep[u] = a;
        else if (k < n_out) out[k] = a;
      }
    }
  }
}
template <bool DEFER, typename In>
__device__ __forceinline__ void layer(int ub, const double* w, int nb, int din, int n_out, int slot, const In in, double* out, bool mine,
                                      double (&keep)[kMlpUnitBlock]) {
  switch (ub) {
    case 1: layer_blocks<1, DEFER>(w, nb, din, n_out, slot, in, out, mine, keep); break;
    case 2: layer_blocks<2, DEFER>(w, nb, din, n_out, slot, in, out, mine, keep); break;
    case 3: layer_blocks<3, DEFER>(w, nb, din, n_out, slot, in, out, mine, keep); break;
    case 4: layer_blocks<4, DEFER>(w, nb, din, n_out, slot, in, out, mine, keep); break;
    case 6: layer_blocks<6, DEFER>(w, nb, din, n_out, slot, in, out, mine, keep); break;
    case 8: layer_blocks<8, DEFER>(w, nb, din, n_out, slot, in, out, mine, keep); break;
    case 12: layer_blocks<12, DEFER>(w, nb, din, n_out, slot, in, out, mine, keep); break;
    default: layer_blocks<16, DEFER>(w, nb, din, n_out, slot, in, out, mine, keep); break;
  }
}
// the compact tile: what a slot kept of its one block goes to the row's LDS, with the 1.0 behind the layer
__device__ __forceinline__ void store_kept(const double (&keep)[kMlpUnitBlock], int ub, int slot, int n_out, double* out, bool active) {
  if (!active) return;
#pragma unroll
  for (int u = 0; u < kMlpUnitBlock; ++u) {
    const int k = slot * ub + u;
    if (u < ub && k < n_out) out[k] = keep[u];
  }
  if (slot == 0) out[n_out] = 1.0;
}

template <typename In> __device__ __forceinline__ double chain(const In in, const double* __restrict__ w, int n) {
  double h = 0.0;
  for (int j = 0; j < n; ++j) h = __dadd_rn(h, __dmul_rn(in(j), w[j]));
  return h;
}

template <bool STAGED, bool COMPACT>
__global__ __launch_bounds__(kThreads) void mlp_predict_kernel(const DeviceMlp mlp, const double* __restrict__ rows, long long n_rows, long long row_stride,
                                                               int TR, int S, int region_a, double* __restrict__ pred, double* __restrict__ logit) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int slot = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int D = mlp.D, dim = D - 1, N1 = mlp.n1, N2 = mlp.n2;
  const long long row0 = (long long)blockIdx.x * TR;
  const int have = (int)(n_rows - row0 < TR ? n_rows - row0 : TR);          // rows of this tile, >= 1
  const bool active = lane < have;
  const int row = active ? lane : 0;                                         // idle lanes read row 0 and store nothing
  double* const ra = lds + (size_t)row * S;                                  // region A: the row, later a2
  double* const rb = ra + (COMPACT ? 0 : region_a);                          // region B: a1 (the compact tile: over region A)
  const GlobalRow grow = {rows + (row0 + row) * row_stride, mlp.mn, mlp.den, dim, mlp.rescale};
  if (STAGED) {
    // the tile's have * dim values in the order they lie in memory, consecutive threads consecutive values; a thread has kStageBatch
    // loads in flight before it rescales and stores the first
    const int total = have * dim;
    for (int i0 = tid; i0 < total; i0 += kThreads * kStageBatch) {
      double v[kStageBatch];
      int at[kStageBatch], col[kStageBatch];
#pragma unroll
      for (int k = 0; k < kStageBatch; ++k) {
        const int i = i0 + k * kThreads;
        const int r = i < total ? i / dim : 0, c = i < total ? i - r * dim : 0;     // beyond the tile: its first value again, not stored
        at[k] = r * S + c; col[k] = c;
        v[k] = rows[(row0 + r) * row_stride + c];
      }
      if (mlp.rescale) {
#pragma unroll
        for (int k = 0; k < kStageBatch; ++k) v[k] = rescaled(v[k], mlp.mn[col[k]], mlp.den[col[k]]);
      }
#pragma unroll
      for (int k = 0; k < kStageBatch; ++k)
        if (i0 + k * kThreads < total) lds[at[k]] = v[k];
    }
    for (int r = tid; r < have; r += kThreads) lds[(size_t)r * S + dim] = 1.0;
  }
  if (!COMPACT && slot == 0 && active && N1 > 0) rb[N1] = 1.0;
  __syncthreads();
  int model = -1;
  if (active) {
    model = 0;
    if (mlp.n_models != 1) {                                                 // type/function.hxx:80-84 on the rescaled, bias-appended row
      const double x1 = STAGED ? ra[mlp.dim1] : grow(mlp.dim1), x0 = STAGED ? ra[mlp.dim0] : grow(mlp.dim0);
      model = x1 < mlp.threshold ? 0 : (x0 < mlp.threshold ? 1 : 2);
    }
  }
  const LdsRow xa = {ra}, xb = {rb};
  double keep[kMlpUnitBlock];
#pragma unroll
  for (int u = 0; u < kMlpUnitBlock; ++u) keep[u] = 0.0;
  if (N1 > 0) {
    for (int m = 0; m < mlp.n_models; ++m) {
      const bool mine = model == m;
      if (!__any(mine)) continue;
      const double* w0 = m == 0 ? mlp.w0[0] : (m == 1 ? mlp.w0[1] : mlp.w0[2]);
      if (STAGED) layer<COMPACT>(mlp.ub1, w0, mlp.nb1, D, N1, slot, xa, rb, mine, keep);
      else layer<COMPACT>(mlp.ub1, w0, mlp.nb1, D, N1, slot, grow, rb, mine, keep);
    }
    __syncthreads();                                                         // a1 complete; nobody reads the row any more
    if (COMPACT) {
      store_kept(keep, mlp.ub1, slot, N1, rb, active);                       // rb == ra: over the row
      __syncthreads();
    } else if (slot == 0 && active) ra[N2] = 1.0;
    for (int m = 0; m < mlp.n_models; ++m) {
      const bool mine = model == m;
      if (!__any(mine)) continue;
      const double* w1 = m == 0 ? mlp.w1[0] : (m == 1 ? mlp.w1[1] : mlp.w1[2]);
      layer<COMPACT>(mlp.ub2, w1, mlp.nb2, N1 + 1, N2, slot, xb, ra, mine, keep);
    }
    __syncthreads();                                                         // a2 complete (compact: kept, and nobody reads a1 any more)
    if (COMPACT) {
      store_kept(keep, mlp.ub2, slot, N2, ra, active);
      __syncthreads();
    }
  }
  if (slot == 0) {
    // the output chain, once per model a row of this wave picked: the weights stay wave-uniform
    const int nin = N1 > 0 ? N2 + 1 : D;
    double h3 = 0.0;
    for (int m = 0; m < mlp.n_models; ++m) {
      const bool mine = model == m;
      if (!__any(mine)) continue;
      const double* w2 = m == 0 ? mlp.w2[0] : (m == 1 ? mlp.w2[1] : mlp.w2[2]);
      const double h = (N1 > 0 || STAGED) ? chain(xa, w2, nin) : chain(grow, w2, nin);
      if (mine) h3 = h;
    }
    if (active) {
      if (logit) logit[row0 + row] = h3;
      if (pred) pred[row0 + row] = __ddiv_rn(1.0, __dadd_rn(1.0, exp(-h3)));
    }
  }
}

}  // namespace

int launch_mlp_predict(const DeviceMlp& mlp, const double* d_rows, long long n_rows, long long row_stride, double* d_pred, double* d_logit,
                       hipStream_t stream) {
  if (n_rows <= 0) return GLIA_HMT_OK;
  const MlpPlan p = mlp_plan(mlp.D - 1, mlp.n1, mlp.n2);
  const int TR = p.tile_rows;
  const size_t shmem = (size_t)TR * p.stride * sizeof(double);
  if (TR < 8 || TR > 64 || shmem > (size_t)kMlpLdsBytes) { set_error("mlp_predict: no tile for this model (internal error)"); return GLIA_HMT_ERR_INTERNAL; }
  // at most kMaxBlocks workgroups per launch: more rows take further launches (GLIA_HMT_MINCAP: 3 workgroups, so that tests of a
  // few hundred rows cross launch boundaries)
  const long long max_blocks = option("GLIA_HMT_MINCAP") ? 3 : kMaxBlocks;
  for (long long r0 = 0; r0 < n_rows; r0 += max_blocks * TR) {
    const long long n = n_rows - r0 < max_blocks * TR ? n_rows - r0 : max_blocks * TR;
    const dim3 grid((unsigned)((n + TR - 1) / TR));
    const double* rows = d_rows + r0 * row_stride;
    double* const pr = d_pred ? d_pred + r0 : nullptr;
    double* const lg = d_logit ? d_logit + r0 : nullptr;
    if (p.staged && p.compact) mlp_predict_kernel<true, true><<<grid, dim3(kThreads), shmem, stream>>>(mlp, rows, n, row_stride, TR, p.stride, p.region_a, pr, lg);
    else if (p.staged) mlp_predict_kernel<true, false><<<grid, dim3(kThreads), shmem, stream>>>(mlp, rows, n, row_stride, TR, p.stride, p.region_a, pr, lg);
    else if (p.compact) mlp_predict_kernel<false, true><<<grid, dim3(kThreads), shmem, stream>>>(mlp, rows, n, row_stride, TR, p.stride, p.region_a, pr, lg);
    else mlp_predict_kernel<false, false><<<grid, dim3(kThreads), shmem, stream>>>(mlp, rows, n, row_stride, TR, p.stride, p.region_a, pr, lg);
    GLIA_HIP_TRY(hipGetLastError());
  }
  return GLIA_HMT_OK;
}

}  // namespace glia
