// glia_amd/csrc/hmt_internal.hpp -- shared definitions of the HIP implementation (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/glia_hmt.h"
#include "median_select.hpp"   // float_ord / ord_float, the order-preserving 32-bit image of an f32

namespace glia {

void set_error(const std::string& msg);
// process-wide tuning / test switches (api.cpp; glia_hmt_set_option): true when `key` is set, its text in *value
bool option(const char* key, std::string* value = nullptr);
// merge loops: calls that ended with GLIA_HMT_ERR_INTERNAL (a kernel's own consistency stop, or an order that fails the replay)
unsigned long long internal_errors();
void count_internal_error();
// dense ids: every merge k joins two regions that still exist and creates region R + k (util/struct_merge.hxx:19-31)
bool merge_order_is_consistent(const uint32_t* dense_order, int64_t n, uint32_t R, int64_t* first_bad);
// the end of every merge loop call: an order that fails the replay becomes GLIA_HMT_ERR_INTERNAL, and every internal error is counted
int finish_merge_order(int rc, const uint32_t* dense_order, int64_t n, uint32_t R, hipStream_t stream);
#define GLIA_HIP_TRY(expr)                                                                       \
  do {                                                                                           \
    hipError_t _e = (expr);                                                                      \
    if (_e != hipSuccess) {                                                                      \
      ::glia::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                      \
      return GLIA_HMT_ERR_HIP;                                                                   \
    }                                                                                            \
  } while (0)

// ---- accumulation tile geometry -------------------------------------------------------------
constexpr int kTileX = 64;         // one wave = one row of 64 voxels, one voxel per lane
#ifndef GLIA_ACC_TILEY
#define GLIA_ACC_TILEY 24
#endif
constexpr int kTileY = GLIA_ACC_TILEY;   // rows of a tile = marching waves x rows per wave (rag_accumulate.hip, Geo)
constexpr int kTZ = 32;            // planes a workgroup marches through (a run of a lane has at most kTZ voxels: 8-bit counters)

// ---- record layouts (32-bit words).  All zero == "empty": minima / lower bounds are stored
// complemented so that every reduction is an add or an unsigned max and tables initialise by memset.
// region record
constexpr int R_CNT = 0, R_BORDER = 1, R_LO = 2 /*3: 0x7fffffff-lo*/, R_HI = 5 /*3: hi+1*/, R_SUM = 8 /*f64*/,
              R_SQ = 10 /*f64*/, R_MIN = 12 /*~ord*/, R_MAX = 13 /*ord*/, R_FIRST = 14 /*u64 ~idx*/, R_HIST = 16;
constexpr int kRegionWords = 32;
// directed pair record
constexpr int P_CNT = 0, P_MIN = 1, P_MAX = 2, P_THR = 4 /*4*/, P_SUM = 8, P_SQ = 10, P_HIST = 12;
constexpr int kPairWords = 32;      // global stride (128-byte lines)


struct HistSpec {
  int bins;
  float fb[GLIA_HMT_MAX_BINS];  // smallest float >= bounds[i] (util/image_stats.hxx:17-22), +inf padded
  float lo_f;                   // largest float <= range.first   (val >  lo  <=> val >  lo_f ; val <= lo <=> val <= lo_f)
  float hi_f;                   // smallest float >= range.second (val <  hi  <=> val <  hi_f)
};

struct AccParams {
  const uint32_t* lab;               // labels; with a mask: the folded copy (masked-out voxels hold kMaskedLabel)
  const uint32_t* lab_c;             // labels of the centre voxels (differs from lab only for contour-only mode + mask)
  int masked;                        // a mask was given
  const float* img;
  int64_t nx, ny, nz;                // extent of the arrays handed in (nz includes halo planes of a slab)
  int64_t gz0, gnz;                  // slab mode: global z of local plane 0 and global depth (gz0 = 0, gnz = nz otherwise)
  int64_t zb, ze;                    // local planes [zb, ze) are accumulated (the halo planes only feed the neighbour rule)
  int dim;
  int nbx, nby, nbz;
  int tz;                            // planes a workgroup marches through: kTZ, or fewer when supervoxels are small
  HistSpec hist;
  int nthr;
  float thr_f[GLIA_HMT_MAX_THRESH];  // smallest float >= threshold (val >= thr <=> val >= thr_f)
  uint32_t* rkeys;                   // label + 1, 0 = empty
  uint32_t* rrec;
  uint32_t rmask;
  unsigned long long* pkeys;         // ((a+1) << 32) | (b+1), 0 = empty
  uint32_t* prec;
  uint32_t pmask;
  uint32_t* flags;                   // [0] region table full, [1] pair table full
  uint32_t debug;                    // ablation switches for profiling builds (GLIA_HMT_DEBUG), 0 in production
};

constexpr int kMaxChannels = 4;     // distinct (image volume, histogram) pairs over all feature lists
constexpr int kMaxListed = GLIA_HMT_MAX_IMAGES;   // images per feature list (region / label / boundary); the vector they give must still fit kMaxFeat columns

// compact, sorted RAG as produced by the edge-table step.  INVARIANT, established by every producer and relied on by every consumer:
// c_rrec[0] == d_rrec and c_prec[0] == d_prec -- a channel's records are read as c_rrec[ch] / c_prec[ch], never with a fallback.
// It owns its blocks (released by free_rag_arrays only) unless it is a view (slab_dist.cpp, Block::view), which is never released.
struct RagArrays {
  int64_t R = 0, P = 0;       // regions, directed pairs
  uint32_t* d_rlabel = nullptr;   // [R] ascending
  uint32_t* d_rrec = nullptr;     // [R][kRegionWords]
  uint32_t* d_pa = nullptr;       // [P] label a (ascending (a,b))
  uint32_t* d_pb = nullptr;       // [P]
  uint32_t* d_prec = nullptr;     // [P][kPairWords]
  // Feature lists with several image volumes: one accumulation pass per distinct (volume, histogram) CHANNEL.  Channel
  // 0 is the boundary-probability volume; the keys are common.
  int K = 1;
  uint32_t* c_rrec[kMaxChannels] = {nullptr, nullptr, nullptr, nullptr};
  uint32_t* c_prec[kMaxChannels] = {nullptr, nullptr, nullptr, nullptr};
  int c_bins[kMaxChannels] = {0, 0, 0, 0};
  // Optional (slab route, median linkage): the image value of every boundary voxel, grouped by directed pair -- values of pair i
  // are d_pv[d_pv_off[i] .. d_pv_off[i + 1]) in no particular order (the median loop sorts its runs itself).  The reference keeps
  // these lists per edge (util/struct_merge.hxx:97-111); a whole-volume map re-reads them from the volume instead.
  unsigned long long* d_pv_off = nullptr;   // [P + 1]
  float* d_pv = nullptr;                    // [nV]
  unsigned long long nV = 0;
};

void free_rag_arrays(RagArrays* a);      // the one place that knows which pointers are owned: every block once, then *a = RagArrays()
int launch_accumulate(const AccParams& p, hipStream_t stream);
int launch_synth(int dim, const int64_t dims[3], int S, int G, uint64_t seed, int variant, uint32_t* d_labels,
                 uint32_t* d_truth_tmp, float* d_pb, hipStream_t stream);
// Masks (type/neighbor.hxx:80-86, util/struct.hxx:86-91,133-143): a masked-out NEIGHBOUR is invalid like an out-of-bounds one;
// a masked-out CENTRE voxel is skipped in point-map mode and processed in contour-only mode.  The mask is folded into a
// copy of the label volume once (sentinel label), so the streaming pass keeps its label loads.
constexpr uint32_t kMaskedLabel = 0xFFFFFFFFu;
int launch_mask_fold(const uint32_t* lab, const uint32_t* mask, uint32_t* out, int64_t n, hipStream_t stream);

// the volume a RAG was built from: median linkage re-reads the boundary voxels' values (util/struct_merge.hxx:97-103)
struct VolumeRef {
  const uint32_t* lab = nullptr;      // centre labels
  const uint32_t* lab_nb = nullptr;   // neighbour labels (the folded copy when a mask was given, else = lab)
  const float* pb = nullptr;
  int dim = 3;
  long long nx = 1, ny = 1, nz = 1;
  long long zb = 0, ze = -1;           // planes whose voxels count (a slab's owned planes; ze < 0: all)
};
// GLIA_USE_MEDIAN_AS_FEATS for a given merge order (median_feats.hip): median, mean and standard deviation of the value multiset of
// every voxel set a bc_feat row looks at.  forced = dense region pairs of the merges; list entry c of the region / boundary lists
// reads r_img[c] / b_img[c] (device).  reg[((i * 3 + k) * n_r + c) * 3 + q]: merge i, k = first region | second region | region
// created, q = median | mean | stddev; bnd[((i * 4 + k) * n_b + c) * 3 + q]: k = B(first) | B(second) | B(created) | shared boundary.
struct MedianFeatIn {
  const RagArrays* rag; VolumeRef vol;
  int n_r; const float* r_img[GLIA_HMT_MAX_IMAGES]; int n_b; const float* b_img[GLIA_HMT_MAX_IMAGES];
  const uint32_t* forced; int64_t n_merges;
};
int median_feature_stats(const MedianFeatIn& in, hipStream_t stream, std::vector<double>* reg, std::vector<double>* bnd, std::vector<unsigned long long>* area);
// GLIA_USE_MEDIAN_AS_FEATS for the INITIAL edges (median_init.hip): every leaf's values and every directed pair's boundary values are
// sorted once per listed image, and the sets of a record (u, v) -- both leaves -- are selections over those runs.  The records are the
// ones of the classifier loop's state (greedy_bc_state.hpp); records [e0, e1) that are table edges of the shard get, at slot e - e0,
//   reg[((slot * 3 + k) * n_r + c) * 3 + q]   k = P(u) | P(v) | P(u + v),               q = median | mean | stddev
//   bnd[((slot * 4 + k) * n_b + c) * 3 + q]   k = B(u) | B(v) | B(u + v) | shared boundary
// (device arrays; u < v are the record's dense leaf ids, NOT the x1 / x2 of the row).  forced / n_merges of `in` are not read.
struct MedianInitRecords {
  const uint32_t *e_u, *e_v; const uint8_t* e_table; uint32_t shard, n_shards;
  const uint32_t* le_start;      // [R + 1] first directed entry of each leaf (entries ascend by (source, target))
  const uint32_t* le_dst;        // [P] target leaf of each entry
};
struct MedianInitTiming { double ms_sort = 0, ms_select = 0; unsigned long long bytes = 0; };   // sort stage (grouping + sort + run sums) | selection kernels | device memory taken
int median_init_stats(const MedianFeatIn& in, const MedianInitRecords& rec, uint32_t e0, uint32_t e1, hipStream_t stream, double* d_reg, double* d_bnd,
                      MedianInitTiming* timing);
// bc_label (bc_label.cpp): the voxels of dense leaf `leaf` with truth label `truth` (0 included), sorted by (leaf, truth) -- the
// table of label_overlap, below, with its labels mapped to leaves (leaf_truth_counts, dense_order.hpp)
struct TruthCount { uint32_t leaf, truth; unsigned long long count; };
// per tree node (leaves 0 .. R-1, merge k = R + k) and one truth volume: n = voxels with truth != 0, size = all voxels,
// Q = sum_t c_t^2, E = sum_t c_t log2 c_t (t != 0); *moves = map entries moved by the small-to-large merging, *node_pairs = the
// (node, truth) pairs of the tree (what a walk that visits each of them once would do)
struct NodeTruthStats { std::vector<unsigned long long> n, size, Q; std::vector<long double> E; };
void node_truth_stats(const std::vector<TruthCount>& cnt, uint32_t R, const uint32_t* forced, int64_t M, NodeTruthStats* out, int64_t* moves,
                      int64_t* node_pairs);
// the labels of main_bc_label_ri / _vi from the per-node values of every truth volume (options already validated)
int bc_label_rules(const std::vector<NodeTruthStats>& st, uint32_t R, const uint32_t* forced, int64_t M, const glia_hmt_bc_label_opts& o,
                   int32_t* labels);
// What a merge loop returns: the order in dense ids (leaf i = i-th label ascending, merged region R + k) -- [n][3] -- with the
// saliencies, optionally the feature row of every merge, the edges scored, and the times of the table, the initial scores and
// the loop.
struct MergeResult {
  std::vector<uint32_t> order;
  std::vector<double> sal, rows;
  int64_t n = 0, n_scored = 0;
  double ms_table = 0.0, ms_init = 0.0, ms_loop = 0.0;
};
// the pb-mean, median and pre_merge loops
struct PbRequest {
  int cond_n = 0;                               // pre_merge condition (gadget/main_pre_merge.cxx:27-76): 0 = none, else 1 or 2 thresholds
  long long cond_sizes[2] = {0, 0};
  double cond_rpb = 0.0;
  const VolumeRef* median_of = nullptr;         // median linkage: the volume the RAG was built from
  bool size_weight = false;                     // ...AndMinSize linkage
};
int greedy_mean(const RagArrays& rag, hipStream_t stream, const PbRequest& req, MergeResult* out);
struct BcCfg;
struct DeviceClassifier;
struct DeviceMlp;
// the classifier loop
struct BcRequest {
  const uint32_t* forced = nullptr;             // a given order (bc_feat): dense region pairs [n_forced][2]; the classifier is not run
  int64_t n_forced = 0;
  bool rows = false;                            // MergeResult::rows wanted
  bool init_only = false;                       // features + scores of the initial records only (TBoundaryTable::init): n = records
  bool scores = false;                          // init_only: MergeResult::sal = the records' scores
  const MedianFeatIn* median = nullptr;         // init_only: score the median layout (GLIA_USE_MEDIAN_AS_FEATS) -- the images and the volume of the map
  int shard = 0, n_shards = 1;
  const DeviceMlp* mlp = nullptr;               // DeviceClassifier::kind == 2: the model (its weights on the device) ...
  int exp_variant = 0;                          // ... and the restatement of the host's exp its sigmoid uses (glibc_math.hpp; 0 = the device's exp)
};
// The loop's set-up kernels and its host driver, greedy_bc_run, are compiled once (greedy_bc_setup.hip).  The three kernels whose
// feature code is specialised -- the initial scores in both layouts and the loop itself (greedy_bc.hip) -- are compiled SIX times,
// and each instance is what the driver is given to launch them (BcInstance, greedy_bc_state.hpp):
//   1      generic: the libm restatements of the feature code (glibc_math.hpp) selected at run time (any combination, incl. "unpinned");
//   2, 3   fma, sse2: the two combinations real hosts have -- glibc's FMA build and its non-FMA build -- fixed at compile time
//          (GLIA_LIBM_FIXED; a run-time choice between three logarithms at every call site costs the loop 5 %);
//   4, 5   fma_common, sse2_common: the same with GLIA_BC_COMMON (bc_features.hpp): one image on the region and boundary lists, no
//          --logs / --simpf / histogram columns;
//   6      mlp (GLIA_BC_MLP, libm at run time): the only one that holds the MLP scorer (DeviceClassifier::kind == 2) -- compiled into
//          the other five it cost the forest's loop a third of its rate (more spilled registers, a larger kernel argument), so they
//          are built without it and the driver refuses kind 2 for them.
// greedy_bc() picks the instance from cfg.libm_*, the feature lists and clf.kind (api_loops.cpp).
struct BcInstance;
const BcInstance& greedy_bc_generic();
const BcInstance& greedy_bc_fma();
const BcInstance& greedy_bc_sse2();
const BcInstance& greedy_bc_fma_common();
const BcInstance& greedy_bc_sse2_common();
const BcInstance& greedy_bc_mlp();
int greedy_bc_run(const BcInstance& inst, const RagArrays& rag, const BcCfg& cfg, const DeviceClassifier& clf, hipStream_t stream,
                  const BcRequest& req, MergeResult* out);
int greedy_bc(const RagArrays& rag, const BcCfg& cfg, const DeviceClassifier& clf, hipStream_t stream, const BcRequest& req, MergeResult* out);
// bc_feat for a given order as a batch computation over the known merge tree (bc_feat_batch.hip): rows [M][cfg.fdim] in the layout
// greedy_bc writes them.  forced: dense region pairs of the merges, validated by the caller.
struct BcFeatBatchInfo {
  double ms_plan = 0, ms_sets = 0, ms_rows = 0;      // host plan (tree tables, uploads) | device: the sets | device: row assembly
  int64_t height = 0, launches = 0, path_updates = 0;
};
int bc_feat_batch_rows(const RagArrays& rag, const BcCfg& cfg, const uint32_t* forced, int64_t M, hipStream_t stream, std::vector<double>* rows,
                       BcFeatBatchInfo* info);
int compact_tables(const AccParams& p, uint32_t rcap, uint32_t pcap, RagArrays* out, hipStream_t stream);
int transform_keys(const uint32_t* order, int64_t n, std::vector<uint32_t>* src, std::vector<uint32_t>* dst);
int64_t gen_tree(const uint32_t* order, int64_t n, uint32_t* node_label, int32_t* parent, int32_t* child0, int32_t* child1, int64_t capacity);
int transform_image(uint32_t* d_lab, int64_t n, const uint32_t* h_src, const uint32_t* h_dst, int64_t m, const uint32_t* d_mask,
                    int fill_missing, hipStream_t stream, double* ms);
int relabel_image(uint32_t* d_lab, int64_t n, int64_t min_size, uint32_t* n_labels, hipStream_t stream);
int paint_pair_values(const VolumeRef& vol, const uint32_t* d_pa, const uint32_t* d_pb, int64_t P, const float* h_val, float* d_out,
                      hipStream_t stream);
int boundary_confidence_values(int n_trees, const int64_t* n_nodes, const uint32_t* const* node_label, const int32_t* const* parent,
                               const int32_t* const* child0, const double* const* potential, const uint32_t* pa, const uint32_t* pb,
                               int64_t P, std::vector<float>* out);
int watershed_labels(int dim, const int64_t dims[3], const float* d_img, double level, uint32_t* d_out, uint32_t* n_labels, int* sweeps,
                     hipStream_t stream);
// face-connected components of a label volume (components.hip); arguments validated by the caller (api.cpp), route = GLIA_HMT_CC
enum { GLIA_HMT_CC_ROUTE_TILED = 0, GLIA_HMT_CC_ROUTE_GLOBAL = 1 };
int label_components(int dim, const int64_t dims[3], const uint32_t* d_in, const uint32_t* d_mask, int mode, int route, uint32_t* d_out,
                     uint32_t* n_components, hipStream_t stream);
// blur_image on the device (blur.hip); arguments validated by the caller (api_blur.cpp).  taps[a] = NULL: axis a is left alone;
// route = GLIA_HMT_BLUR; *route_used: the route that ran (march falls back to passes above kBlurMarchRadius), *ms: its device time
constexpr int kBlurTileX = 64, kBlurTileY = 16;   // the x-y tile of a marching workgroup
constexpr int kBlurMarchRadius = 5;               // largest radius of the march route: tile + halo, the x pass and a ring of 2 r + 1 planes in 64 KiB of static LDS
struct GaussianKernel;
int blur_image_device(int dim, const int64_t dims[3], int pixel_type, const void* d_in, const GaussianKernel* const taps[3], int route, void* d_out,
                      hipStream_t stream, double* ms, int* route_used);
// the contingency table of two label streams under a mask (label_overlap.hip): entries with count > 0 ascending by (a, b); arguments
// validated by the caller (api.cpp).  info: device time of the counting passes (all of them, a repeated pass included) and how many were repeated
struct OverlapPass { double ms = 0; int repeats = 0; };
int label_overlap(const uint32_t* d_a, const uint32_t* d_b, const uint32_t* d_mask, unsigned long long n_voxels, int flags,
                  hipStream_t stream, std::vector<glia_hmt_overlap_entry>* out, OverlapPass* info);
// the scores of eval_ri / eval_vi from such tables (eval.cpp, host-only); arguments validated by the caller
int overlap_scores(const glia_hmt_overlap_entry* const* tables, const int64_t* n_entries, int n_tables, int vi_mode, glia_hmt_eval_result* out);
int launch_libm_eval(int function, int variant, const double* d_in, double* d_out, int64_t n, hipStream_t stream);
int merge_rag_arrays(const RagArrays* parts, int n_parts, RagArrays* out, hipStream_t stream);
// boundary-voxel values per directed pair of a map built from `vol` (its owned planes): fills rag->d_pv_off / d_pv / nV (owned)
int collect_pair_values(RagArrays* rag, const VolumeRef& vol, hipStream_t stream);
// value runs in a new pair order: out run j = source run order[j] (counts from the source offsets); `own` allocates *out_off [n + 1], *out_vals
struct OwnedArrays;
int gather_value_runs(const unsigned long long* src_off, const float* src_vals, const uint32_t* order, uint32_t n, OwnedArrays& own,
                      unsigned long long** out_off, float** out_vals, unsigned long long* nV, hipStream_t stream);
int rag_cut_flags(const RagArrays& rag, const uint32_t* d_lab, int64_t nx, int64_t ny, int64_t nzl, int64_t zb, int64_t ze,
                  uint8_t* d_rflag, uint8_t* d_pflag, hipStream_t stream);

}  // namespace glia
