/* include/glia_hmt.h -- C ABI of the MI355X-native HMT hot path (libglia_hmt.so).
 *
 * Drop-in boundary for GLIA's hierarchical-merge-tree path (code/hmt + the L1/L2 types it
 * drives).  GLIA has no FFI/plugin registry: its operator API is header templates whose
 * behaviour is injected through lambdas, plus CLIs and file formats.  Each
 * entry point below therefore replaces one reference operator together with the fixed set
 * of lambdas the reference's own callers pass to it; the citation names file:line under
 * /root/reference/code/.
 *
 * Conventions: plain C, opaque handles, int status (0 = ok, <0 = error, message via
 * glia_hmt_last_error()); never exits the process (the reference's perr() does,
 * glia_base.hxx:66-69).  Pointers prefixed d_ are DEVICE (HBM) pointers on the context's
 * GPU, h_ are host pointers.  Volumes are dense, x fastest: index = x + nx*(y + ny*z),
 * labels uint32 (glia_base.hxx:43), images float (:44), features double (:45).
 * A handle is not thread-safe; all work of a context is ordered on its HIP stream.
 */
#ifndef GLIA_HMT_H
#define GLIA_HMT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLIA_HMT_OK 0
#define GLIA_HMT_ERR_ARG (-1)          /* invalid argument */
#define GLIA_HMT_ERR_HIP (-2)          /* HIP runtime error */
#define GLIA_HMT_ERR_UNSUPPORTED (-3)  /* valid in the reference, not implemented here yet */
#define GLIA_HMT_ERR_CAPACITY (-4)     /* caller-provided output buffer too small */
#define GLIA_HMT_ERR_SALIENCY (-5)     /* "Error: invalid boundary saliency..." (util/struct_merge.hxx:58-59) */
#define GLIA_HMT_ERR_IO (-6)           /* file could not be read / malformed */
#define GLIA_HMT_ERR_INTERNAL (-7)     /* a merge loop stopped on its own consistency check (see glia_hmt_internal_errors) */

#define GLIA_HMT_MAX_IMAGES 8
#define GLIA_HMT_MAX_BINS 16
#define GLIA_HMT_MAX_THRESH 4

typedef struct glia_hmt_ctx glia_hmt_ctx;
typedef struct glia_hmt_rag glia_hmt_rag;
typedef struct glia_hmt_forest glia_hmt_forest;

const char* glia_hmt_last_error(void);
const char* glia_hmt_version(void);

/* Context: device + stream + reusable workspaces.  hip_stream may be NULL (own stream) or a
 * hipStream_t the caller owns (e.g. torch.cuda.current_stream().cuda_stream). */
int glia_hmt_ctx_create(int device, void* hip_stream, glia_hmt_ctx** out);
void glia_hmt_ctx_destroy(glia_hmt_ctx* ctx);
/* The library parks scratch blocks of finished calls for reuse (at most 12 GiB per process; a hipMalloc / hipFree pair is a
 * device-wide synchronisation).  This returns them to the driver -- for callers that share the device with another allocator
 * (torch, a second library).  Returns the number of bytes released.  Destroying the last context of a process does the same. */
unsigned long long glia_hmt_release_cached_memory(void);
/* The invariant of genMergeOrderGreedy's output (util/struct_merge.hxx:19-31: the loop appends (r0, r1, key++) and erases the two
 * regions' items): merge k joins two regions that still exist and creates region n_regions + k.  h_order holds DENSE ids (leaf i =
 * i-th label ascending, merged region n_regions + k).  Returns GLIA_HMT_OK, or GLIA_HMT_ERR_ARG with *first_bad = the first merge
 * that breaks the rule.  The pb / pre_merge loops run this O(R) replay on every order before they return it; a violation ends the
 * call with GLIA_HMT_ERR_INTERNAL -- it is never repaired by running the loop again. */
int glia_hmt_check_merge_order(const uint32_t* h_order, int64_t n_merges, int64_t n_regions, int64_t* first_bad);
/* Calls of this process that ended with GLIA_HMT_ERR_INTERNAL.  0 is the only healthy answer: bench.py prints it, the GPU test
 * session and __graft_entry__.smoke() assert it. */
unsigned long long glia_hmt_internal_errors(void);
/* Tuning and test switches of the loops, process-wide: which queue the pb-mean loop runs on (GLIA_HMT_PB_WINDOW, GLIA_HMT_PB_BATCH,
 * GLIA_HMT_FORCE_TREE), its window size / baseline interval / horizon (GLIA_HMT_WINCAP, GLIA_HMT_REBASE, GLIA_HMT_REBASE_END, GLIA_HMT_HORIZON), the
 * classifier loop's helper workgroups and instance tier (GLIA_HMT_HELPERS, GLIA_HMT_BC_NOCOMMON, GLIA_HMT_BC_GENERIC), the libm
 * variant (GLIA_HMT_LIBM, read when a context is created), GLIA_HMT_TRACE, GLIA_HMT_DEBUG (profiling build).  No setting changes a
 * result.  value = NULL unsets.  The table starts from the environment variables of the same names, read once; nothing in the
 * library calls getenv() per call.  Unknown key: GLIA_HMT_ERR_ARG. */
int glia_hmt_set_option(const char* key, const char* value);
int glia_hmt_ctx_sync(glia_hmt_ctx* ctx);
/* Logarithms of the feature vector.  The reference computes histogram entropies with std::log2 (util/stats.hxx:145-152)
 * and the --logs features with std::log (glia_base.hxx:80-81), the compactness with std::pow (type/feat.hxx:78-79), i.e.
 * with the host's glibc, which is not correctly
 * rounded; the kernels carry restatements of glibc's algorithms (glia_amd/csrc/glibc_math.hpp) and the context selects,
 * by probing the host's libm when it is created, the one that reproduces it bit for bit: 1 = non-FMA build ("sse2"),
 * 2 = FMA build, 0 = no restatement matches this host (device libm, within 1 ulp: entropy features then UNPINNED).
 * glia_hmt_host_libm_probe runs the same probe without a GPU; glia_hmt_libm_eval evaluates function (0 = log2, 1 = log,
 * 2 = the pow(perim, 1.5) of type/feat.hxx:78-79, 3 = exp, 4 = the sigmoid 1 / (1 + exp(-h)) built on it) in the given variant over
 * a device array (parity tests).
 * std::exp is probed too (glia_hmt_ctx_libm_exp): the MLP of the classifier loop (glia_hmt_merge_order_bc_mlp) turns its logit into
 * the queue key with it, as alg/nn.hxx does on the host.  0 there: the loop uses the device's exp and its saliencies are within a
 * few ulps of the host's, unpinned.  It is not part of glia_hmt_ctx_libm_status, which speaks of the feature columns. */
int glia_hmt_ctx_libm(const glia_hmt_ctx* ctx, int* log2_variant, int* log_variant);
int glia_hmt_ctx_libm_pow(const glia_hmt_ctx* ctx, int* pow_variant);        /* same, for std::pow(perim, 1.5) (type/feat.hxx:78-79) */
int glia_hmt_ctx_libm_exp(const glia_hmt_ctx* ctx, int* exp_variant);        /* same, for std::exp (the MLP's sigmoid) */
/* 1 = all three host functions are reproduced bit for bit, 0 = at least one is not (glia_hmt_ctx_create then also leaves a
 * "warning: ..." text in glia_hmt_last_error(); the tools print it to stderr), < 0 = error */
int glia_hmt_ctx_libm_status(const glia_hmt_ctx* ctx);
int glia_hmt_host_libm_probe(int* log2_variant, int* log_variant);
int glia_hmt_host_libm_probe_pow(int* pow_variant);
int glia_hmt_host_libm_probe_exp(int* exp_variant);
int glia_hmt_host_libm_eval(int function, int variant, const double* h_in, double* h_out, int64_t n);  /* host code of the same restatement, no GPU */
int glia_hmt_libm_eval(glia_hmt_ctx* ctx, int function, int variant, const double* d_in, double* d_out, int64_t n);
/* Which region is "region 0" of an initial edge, everything else being equal, follows the iteration order of the reference's
 * std::unordered_map region map (type/region_map.hxx:79-95 filled from genPointMap, util/struct.hxx:77-92).  The library
 * reproduces it by replaying the insertions under libstdc++'s hashtable rules (glia_amd/csrc/rmap_order.cpp).  This host-only
 * entry evaluates the replay for n leaves (labels ascending, first_voxel = raster index of a label's first voxel): rank[i] =
 * position of leaf i in that order.  mode 0 = as the library does, 1 = through the real container, 2 = the array emulation
 * (tests compare them). */
int glia_hmt_host_rmap_ranks(const uint32_t* labels, const int64_t* first_voxel, int64_t n, int mode, uint32_t* rank);
/* Optional sizing hint for the accumulation hash tables (0 = derive from the volume size; they grow and
 * the pass is redone if they fill up). */
int glia_hmt_ctx_set_table_hint(glia_hmt_ctx* ctx, int64_t expected_regions, int64_t expected_pairs);

/* Image + histogram spec: one ImageHistPair of hmt/bc_feat.hxx:29-43. */
typedef struct {
  const float* d_image;
  int bins;            /* --rbb/--rlb/--rb/--bb, <= GLIA_HMT_MAX_BINS */
  double lo, hi;       /* histogram range (--rbl/--rbu ...) */
} glia_hmt_image;

/* Feature configuration = the image lists prepareImages builds (hmt/hmt_util.hxx:17-56: an --rbi
 * image is appended to BOTH the region and the boundary list) plus the scalar flags of
 * hmt/main_merge_order_bc.cxx:172-242.  At most 4 entries per list; every distinct (d_image, bins, lo, hi) over
 * all lists is one accumulation pass over the volume (at most 4 distinct ones). */
typedef struct {
  int n_region;  glia_hmt_image region[GLIA_HMT_MAX_IMAGES];         /* rImages  */
  int n_rlabel;  glia_hmt_image rlabel[GLIA_HMT_MAX_IMAGES];         /* rlImages */
  int n_boundary; glia_hmt_image boundary[GLIA_HMT_MAX_IMAGES];      /* bImages  */
  const float* d_pb;                 /* --pb */
  int n_thresholds;                  /* --bt, <= GLIA_HMT_MAX_THRESH */
  double thresholds[GLIA_HMT_MAX_THRESH];
  double normalizing_area;           /* 1.0 unless --ns (main_merge_order_bc.cxx:36-39) */
  double normalizing_length;
  int use_log_shape;                 /* --logs */
  int use_simple_features;           /* --simpf */
  /* Build options of the reference that change the vector layout (CMakeLists.txt:54-64, type/feat.hxx:608-621, 677-722):
   * GLIA_HMT_HIST_FEAT -> GLIA_USE_HISTOGRAM_AS_FEATS: every image-feature block carries its normalised histogram ahead of
   * the entropy (bins more columns per block).  GLIA_HMT_MEDIAN_FEAT -> GLIA_USE_MEDIAN_AS_FEATS: every real-feature block carries
   * the MEDIAN of its voxel set ahead of the mean, mean / standard deviation come from the value vector (stats::mean, stats::var),
   * the diff blocks gain |median0 - median1|, --simpf carries the shared boundary's median beside its mean (hmt/bc_feat.hxx:252-268).
   * Implemented for a GIVEN merge order (glia_hmt_bc_feat / _saliency: glia_amd/csrc/median_feats.hip; the value multisets of one
   * order are processed in batches of 2^27 values, one set may hold at most 2^30) and for the scores of the INITIAL edges
   * (glia_hmt_score_initial_edges / _shard with a forest, an ensemble or the stub: glia_amd/csrc/median_init.hip sorts every leaf's
   * and every directed pair's values once per listed image and selects each median over those runs; < 2^32 values per image).  Both
   * need the volumes the map was built from (glia_hmt_rag_build; a slab / distributed map gives GLIA_HMT_ERR_UNSUPPORTED).  The
   * greedy loop (glia_hmt_merge_order_bc) returns GLIA_HMT_ERR_UNSUPPORTED with this layout.  Median columns are bit-exact (the
   * radix sort's order is the ordering rule: -0.0 sorts below +0.0), the mean / stddev columns comparable to 1e-12 (the reference
   * sums in an order that depends on rand(), util/stats.hxx:87). */
  int use_histogram_features;
  int use_median_features;
} glia_hmt_feat_config;

/* ---- region adjacency structure -------------------------------------------------------
 * Replaces TRegionMap(image, mask, onlyContour) (type/region_map.hxx:38-40,52-65), i.e.
 * genPointMap/genContourMap (util/struct.hxx:77-144) with getContourTraits
 * (type/neighbor.hxx:109-126).  Instead of voxel lists it accumulates, in ONE pass over the
 * label volume and `cfg->d_pb`/image volumes, the sufficient statistics every downstream
 * operator needs: per label (count, border count, bbox, image moments, histogram) and per
 * DIRECTED label pair (a->b) (boundary voxel count, image moments, histogram, threshold counts).
 * cfg may be NULL when only merge_order_pb will be called (then d_pb must be given).
 * d_mask (optional, u32 volume, MASK_OUT_VAL = 0 masks a voxel out): masked-out neighbours are invalid like
 * out-of-bounds ones (type/neighbor.hxx:80-86); a masked-out centre voxel belongs to no region when only_contour = 0
 * (util/struct.hxx:86-91) and is still processed when only_contour = 1 (:133-143 has no mask test).
 * The label / mask / image volumes must stay alive while the handle lives: median linkage re-reads them. */
int glia_hmt_rag_build(glia_hmt_ctx* ctx, int dim, const int64_t dims[3], const uint32_t* d_labels,
                       const uint32_t* d_mask, int only_contour, const float* d_pb,
                       const glia_hmt_feat_config* cfg, glia_hmt_rag** out);
/* ---- z-slab partition for volumes split across GPUs (no reference counterpart: GLIA is single-node) ----------
 * A rank owns global planes [z_global_of_plane0 + z_begin, z_global_of_plane0 + z_end) and hands in its planes plus
 * one halo plane on each side that is not a face of the volume (dims_local[2] = planes handed in).  The result is a
 * PARTIAL region map: every statistic is a commutative monoid, so partial maps of all slabs are combined with
 * glia_hmt_rag_merge into exactly the map glia_hmt_rag_build gives for the whole volume.  Between ranks the partial
 * records travel as the plain device arrays glia_hmt_rag_device_arrays exposes -- only the records glia_hmt_rag_cut_flags marks
 * take the keyed owner exchange (unpadded point-to-point messages over RCCL), everything goes once to the rank that runs the
 * merge loop (glia_amd/slab.py) -- and are wrapped again with glia_hmt_rag_from_arrays (`like` supplies configuration and
 * dimensions). */
int glia_hmt_rag_build_slab(glia_hmt_ctx* ctx, const int64_t dims_local[3], int64_t z_global_of_plane0,
                            int64_t nz_global, int64_t z_begin, int64_t z_end, const uint32_t* d_labels,
                            int only_contour, const float* d_pb, const glia_hmt_feat_config* cfg, glia_hmt_rag** out);
int glia_hmt_rag_merge(glia_hmt_ctx* ctx, glia_hmt_rag* const* parts, int n_parts, glia_hmt_rag** out);
/* ---- the slab route end to end (glia_amd/csrc/slab_dist.cpp): build, keyed owner exchange of the cut records, hand-over ----
 * A communicator holds the ranks of ONE process.  glia_hmt_comm_create_rccl: one rank per process and GPU, transfers between
 * processes are ncclSend / ncclRecv over RCCL (xGMI inside a node); the 128-byte id comes from glia_hmt_comm_unique_id on one rank
 * and reaches the others through the launcher (a file, an environment variable).  glia_hmt_comm_create_local: all `world` ranks
 * in this process on this context's GPU, transfers are device copies -- the same code path otherwise (single-GPU runs of volumes
 * processed slab by slab, tests).  librccl.so is loaded when the first RCCL communicator is made, not linked. */
typedef struct glia_hmt_comm glia_hmt_comm;
int glia_hmt_comm_unique_id(void* id128);
int glia_hmt_comm_create_rccl(glia_hmt_ctx* ctx, int world, int rank, const void* id128, glia_hmt_comm** out);
int glia_hmt_comm_create_local(glia_hmt_ctx* ctx, int world, glia_hmt_comm** out);
void glia_hmt_comm_destroy(glia_hmt_comm* comm);
int glia_hmt_comm_world(const glia_hmt_comm* comm);
int glia_hmt_comm_local_ranks(const glia_hmt_comm* comm, int* ranks, int capacity);      /* returns their number */
/* the z range of rank `rank` of `world`: planes [first_plane, first_plane + n_planes) are handed in (owned planes + one halo
 * plane per cut), of which the local planes [z_begin, z_end) are owned (the arguments of glia_hmt_rag_build_slab) */
int glia_hmt_slab_range(int64_t nz, int world, int rank, int64_t* first_plane, int64_t* n_planes, int64_t* z_begin, int64_t* z_end);
typedef struct {
  int64_t dims_local[3];             /* x, y, planes handed in */
  int64_t z_global_of_plane0;        /* global z of local plane 0 */
  int64_t z_begin, z_end;            /* owned local planes */
  const uint32_t* d_labels;          /* device, dims_local */
  const float* d_pb;                 /* device, dims_local (or NULL when cfg lists the images) */
  const glia_hmt_feat_config* cfg;   /* image lists of THIS slab's sub-volumes, or NULL */
} glia_hmt_slab;
typedef struct {
  uint64_t records, cut_records;                     /* of the local ranks: all records / records that took the owner exchange */
  uint64_t bytes_cut_exchange, bytes_to_loop_owner;  /* bytes the local ranks sent to OTHER ranks in step 2 / step 3 */
} glia_hmt_dist_stats;
/* slabs[i] belongs to the i-th local rank of the communicator (rank order).  *out = the whole volume's map when loop_owner is a
 * local rank, NULL otherwise.  Collective: every process of the communicator calls it.
 * with_values != 0: the image value (d_pb) of every boundary voxel travels with its directed pair, so that the merged map can run
 * the MEDIAN linkage (glia_hmt_merge_order_pb type 1, the reference tool's default, hmt/main_merge_order_pb.cxx:10; the reference
 * keeps these value lists per edge, util/struct_merge.hxx:97-111) -- 4 bytes per boundary voxel on top of the records. */
int glia_hmt_rag_build_distributed(glia_hmt_ctx* ctx, glia_hmt_comm* comm, const glia_hmt_slab* slabs, int64_t nz_global, int only_contour,
                                   int with_values, int loop_owner, glia_hmt_rag** out, glia_hmt_dist_stats* stats);
/* Which records of a slab's partial map may have a counterpart in another slab ("exchanging only the cross-slab boundary
 * regions"): d_region_cut[i] / d_pair_cut[i] (device, one byte per record, in the order of glia_hmt_rag_device_arrays) = 1 iff
 * the region's label / one of the pair's labels occurs on a plane next to a cut (first / last owned plane, halo plane).  Only
 * flagged records take the keyed owner exchange (glia_amd/slab.py); the others go once to the rank that runs the merge loop.
 * dims_local / z_begin / z_end / d_labels: as handed to glia_hmt_rag_build_slab. */
int glia_hmt_rag_cut_flags(glia_hmt_ctx* ctx, const glia_hmt_rag* rag, const int64_t dims_local[3], int64_t z_begin, int64_t z_end,
                           const uint32_t* d_labels, uint8_t* d_region_cut, uint8_t* d_pair_cut);
int glia_hmt_rag_device_arrays(const glia_hmt_rag* rag, const uint32_t** d_region_label, const uint32_t** d_region_rec,
                               const uint32_t** d_pair_a, const uint32_t** d_pair_b, const uint32_t** d_pair_rec,
                               int* region_words, int* pair_words);
/* copies the compact arrays into caller-owned device buffers ([R], [R][region_words], [P], [P], [P][pair_words]) */
int glia_hmt_rag_copy_arrays(const glia_hmt_rag* rag, uint32_t* d_region_label, uint32_t* d_region_rec,
                             uint32_t* d_pair_a, uint32_t* d_pair_b, uint32_t* d_pair_rec);
int glia_hmt_rag_from_arrays(glia_hmt_ctx* ctx, const glia_hmt_rag* like, int64_t n_regions,
                             const uint32_t* d_region_label, const uint32_t* d_region_rec, int64_t n_pairs,
                             const uint32_t* d_pair_a, const uint32_t* d_pair_b, const uint32_t* d_pair_rec,
                             glia_hmt_rag** out);
/* Feature lists with several image volumes give a map one record set per CHANNEL (distinct volume + histogram); the keys are
 * common.  glia_hmt_rag_device_arrays / _copy_arrays / _from_arrays handle channel 0; the further channels of a partial map
 * are copied out with glia_hmt_rag_copy_channel and attached, in order, to a map made by glia_hmt_rag_from_arrays with
 * glia_hmt_rag_add_channel (`like` supplied the histogram layout of every channel). */
int glia_hmt_rag_num_channels(const glia_hmt_rag* rag);
int glia_hmt_rag_copy_channel(const glia_hmt_rag* rag, int channel, uint32_t* d_region_rec, uint32_t* d_pair_rec);
int glia_hmt_rag_add_channel(glia_hmt_ctx* ctx, glia_hmt_rag* rag, const uint32_t* d_region_rec, const uint32_t* d_pair_rec);
void glia_hmt_rag_free(glia_hmt_rag* rag);
int64_t glia_hmt_rag_num_regions(const glia_hmt_rag* rag);
int64_t glia_hmt_rag_num_pairs(const glia_hmt_rag* rag);     /* directed label pairs */
/* Export for inspection / parity tests (host arrays sized by the counts above; any may be NULL).
 * Regions ascend by label; pairs ascend by (a,b). */
int glia_hmt_rag_export_regions(const glia_hmt_rag* rag, uint32_t* h_label, int64_t* h_count,
                                int64_t* h_border, int64_t* h_bbox_lo /*[n][3]*/, int64_t* h_bbox_hi,
                                double* h_sum, double* h_sumsq, double* h_min, double* h_max,
                                int64_t* h_hist /*[n][bins]*/, int64_t* h_first_voxel);
int glia_hmt_rag_export_pairs(const glia_hmt_rag* rag, uint32_t* h_a, uint32_t* h_b, int64_t* h_count,
                              double* h_sum, double* h_sumsq, double* h_min, double* h_max,
                              int64_t* h_hist /*[n][bins]*/, int64_t* h_thr /*[n][n_thresholds]*/);
/* Kernel time of the accumulation pass of the last build on this handle, measured with HIP events
 * on the context stream (milliseconds), and the algorithmic bytes it covers. */
int glia_hmt_rag_last_pass(const glia_hmt_rag* rag, double* ms, double* algorithmic_bytes);

/* ---- greedy merge orders -----------------------------------------------------------------
 * glia_hmt_merge_order_pb replaces genMergeOrderGreedyUsingPbApproxMedian (type 1,
 * util/struct_merge.hxx:90-136) and genMergeOrderGreedyUsingPbMean (type 2, :38-85) as called by
 * merge_order_pb (hmt/main_merge_order_pb.cxx:27-36) with fcond = f_true.
 * Output: h_order[3*i..] = (x0, x1, x2) of merge i (TTriple, type/tuple.hxx:8-29),
 * h_saliency[i] = popped queue key.  *n_merges <= capacity.  Type 1 (the tool's default) keeps, per table edge, the
 * SORTED run of its boundary voxels' values; a contraction merges runs (merge path) and reads the order statistic
 * n/2 (stats::amedian, util/stats.hxx:83-91).  It needs a handle built by glia_hmt_rag_build (whole volume).
 * Type 3 (no tool of the reference calls it) = genMergeOrderGreedyUsingPbApproxMedianAndMinSize (:141-185): saliency
 * -median * min(size of the two regions), regions merged as the loop goes; needs only_contour = 0. */
int glia_hmt_merge_order_pb(glia_hmt_ctx* ctx, glia_hmt_rag* rag, int type, uint32_t* h_order,
                            double* h_saliency, int64_t capacity, int64_t* n_merges);

/* ---- boundary classifier -------------------------------------------------------------------------
 * glia_hmt_forest_load replaces alg::RandomForest(predictLabel, modelFile) (alg/rf.hxx:22-33) for n_models == 1
 * and alg::EnsembleRandomForest + opt::ThresholdModelDistributor(dim0, dim1, threshold) (alg/rf.hxx:63-98,
 * type/function.hxx:71-85; --bcmd) for n_models == 3.  Files are GLIA's binary RF models
 * (ml/rf/ml_rf_model.cxx:378-455).  predict_label is BC_LABEL_MERGE = -1 in every reference caller.
 * glia_hmt_forest_stub builds the diagnostic scorer P = 1 - x[feature_index] (tests only). */
int glia_hmt_forest_load(glia_hmt_ctx* ctx, int n_models, const char* const* paths, int predict_label,
                         const double* distributor_args /*[3] or NULL*/, glia_hmt_forest** out);
/* Host-only: parse a GLIA model file (rf_old::readModelFromBinaryFile, ml/rf/ml_rf_model.cxx:459-563) into the node
 * arrays the device walks: h_split[tree][node], h_meta[tree][node][4] = {variable (0-based), left, right (0-based node),
 * vote (-1 = internal node, else 1 iff the leaf's class is predict_label)}.  Needs no GPU. */
int glia_hmt_forest_file_parse(const char* path, int predict_label, int* ntree, int* nrnodes, int* nclass,
                               double* h_split, int* h_meta, int64_t capacity_nodes);
int glia_hmt_forest_stub(glia_hmt_ctx* ctx, int feature_index, glia_hmt_forest** out);
void glia_hmt_forest_free(glia_hmt_forest* forest);

/* Replaces the prediction loop of pred_rf (ml/rf/main_pred_rf.cxx:13-40; alg::RandomForest / EnsembleRandomForest::operator(),
 * alg/rf.hxx; the model pick of opt::ThresholdModelDistributor, type/function.hxx:71-85) for a batch of feature rows -- what bc_feat -b
 * and merge_order_bc -b write.  pred[i] = votes for predict_label / ntree of the model the distributor picks for row i (it tests
 * x[dim1] < threshold first, then x[dim0] < threshold); for a stub classifier 1 - x[index].  The walk goes left iff x[var] <= split, so
 * a NaN goes right; votes are integers, the results bit-exact.  dim = columns of a row: it must exceed every column the classifier
 * reads (tree variables, distributor dimensions, stub index), else GLIA_HMT_ERR_ARG.  n_rows == 0 is GLIA_HMT_OK.  Any number of rows:
 * beyond 2^23 tiles the work takes several launches.
 * glia_hmt_forest_predict streams host rows through device buffers in bounded chunks and returns when h_pred is written.
 * glia_hmt_forest_predict_device reads device rows (row i at d_rows + i * row_stride doubles, row_stride >= dim; the padding is never
 * read) and is ordered on the context's stream like every other call.  Rows of up to GLIA_HMT_PREDICT_STAGE_MAX_DIM columns are staged
 * in LDS, longer ones are walked from global memory (glia_amd/csrc/forest_predict.hip). */
#define GLIA_HMT_PREDICT_STAGE_MAX_DIM 767
int glia_hmt_forest_predict(glia_hmt_ctx* ctx, const glia_hmt_forest* forest, const double* h_rows, int64_t n_rows, int dim,
                            double* h_pred);
int glia_hmt_forest_predict_device(glia_hmt_ctx* ctx, const glia_hmt_forest* forest, const double* d_rows, int64_t n_rows, int dim,
                                   int64_t row_stride /* doubles, >= dim */, double* d_pred);
/* Host-only: the rows of the LDS tile the kernel takes for n_rows rows of dim columns -- 64, 32, 16 or 8 -- or 0 when rows of that
 * length are not staged (dim > GLIA_HMT_PREDICT_STAGE_MAX_DIM).  For tests and tuning; no result depends on it. */
int glia_hmt_forest_predict_tile_rows(int64_t n_rows, int dim);

/* ---- the MLP and logsig batch predictors --------------------------------------------------------------
 * Replace pred_mlp (sshmt/main_pred_mlp.cxx:18-48) and pred_logsig (sshmt/main_pred_logsig.cxx:12-32): alg::MLP2v /
 * alg::EnsembleMLP2v (alg/nn.hxx:14-254; two ReLU hidden layers of n1 and n2 units, a sigmoid output) and alg::Logsig
 * (alg/function.hxx:33-34; n1 = n2 = 0) over feature rows -- what bc_feat -b writes.  Per row: stats::rescale to [-1, 1] when a min/max
 * table is given (util/stats.hxx:265-277), a 1.0 appended, for three models the pick of opt::ThresholdModelDistributor
 * (type/function.hxx:80-84) on that RESCALED, bias-appended vector (indices in [0, dim]), the layers, 1 / (1 + exp(-logit)).
 * The arithmetic is this library's own definition (glia_amd/csrc/mlp_model.hpp): every sum starts at 0.0 and takes
 * its terms in ascending index order, multiply and add rounded separately.  The reference computes the same sums through Eigen, in an
 * order that depends on how Eigen vectorises: parity with its last bits is not claimed.  Host forward pass and kernel agree bit for bit
 * on the logits.
 * A model is the reference's text file of weights (readData(w, file, true)): D * n1 + (n1 + 1) * n2 + n2 + 1 doubles with D = columns
 * of a row + 1 (logsig: D doubles).  A count that gives no whole D, or D < 2: GLIA_HMT_ERR_ARG with a message (the reference
 * truncates).  n1 or n2 above 256, rows of more than 65535 columns: GLIA_HMT_ERR_UNSUPPORTED.  Unlike alg::MLP2v(N1, N2, file)
 * (nn.hxx:150-154), which reads the file and never copies the weights in, a single model is loaded.
 * glia_hmt_mlp_file_parse (host-only): the doubles of a model file; h_w may be NULL to ask for *n_weights alone.
 * glia_hmt_mlp_create / _load: ctx may be NULL for a host-only handle (glia_hmt_mlp_predict_host and glia_hmt_mlp_dim only).
 * h_min / h_max: n_minmax >= dim entries each (extras ignored; fewer: GLIA_HMT_ERR_ARG), NULL = no rescale; the min/max file has two
 * rows, minima then maxima.  distributor_args = {dim0, dim1, threshold}, required for three models.
 * Prediction: any number of rows (beyond 2^23 tiles the work takes several launches); dim != glia_hmt_mlp_dim is GLIA_HMT_ERR_ARG, n_rows == 0 is GLIA_HMT_OK, two calls with the same arguments return
 * identical bytes; h_pred / h_logit (d_pred / d_logit) may each be NULL, not both.
 * glia_hmt_mlp_predict_host: the header's forward pass, no GPU.
 * glia_hmt_mlp_predict_device: device rows (row i at d_rows + i * row_stride doubles, the padding is never read), ordered on the
 * context's stream; the sigmoid is computed on the device (within a few ulps of the host's).
 * glia_hmt_mlp_predict: host rows streamed through bounded device buffers; the kernel returns the logits and the sigmoid is applied on
 * the host with the host's exp, so h_pred is what a host program computes from h_logit. */
typedef struct glia_hmt_mlp glia_hmt_mlp;
int glia_hmt_mlp_file_parse(const char* path, double* h_w, int64_t capacity, int64_t* n_weights);
int glia_hmt_mlp_create(glia_hmt_ctx* ctx, int n_models /*1 or 3*/, const double* const* h_weights, const int64_t* n_weights, int n1, int n2,
                        const double* h_min, const double* h_max /*NULL: no rescale*/, int64_t n_minmax,
                        const double* distributor_args /*[3] or NULL*/, glia_hmt_mlp** out);
int glia_hmt_mlp_load(glia_hmt_ctx* ctx, int n_models, const char* const* paths, int n1, int n2, const char* minmax_path /*or NULL*/,
                      const double* distributor_args /*[3] or NULL*/, glia_hmt_mlp** out);
int glia_hmt_mlp_dim(const glia_hmt_mlp* mlp);   /* the columns a row must have */
void glia_hmt_mlp_free(glia_hmt_mlp* mlp);
int glia_hmt_mlp_predict_host(const glia_hmt_mlp* mlp, const double* h_rows, int64_t n_rows, int dim, double* h_pred, double* h_logit);
int glia_hmt_mlp_predict_device(glia_hmt_ctx* ctx, const glia_hmt_mlp* mlp, const double* d_rows, int64_t n_rows, int dim,
                                int64_t row_stride /* doubles, >= dim */, double* d_pred /*or NULL*/, double* d_logit /*or NULL*/);
int glia_hmt_mlp_predict(glia_hmt_ctx* ctx, const glia_hmt_mlp* mlp, const double* h_rows, int64_t n_rows, int dim, double* h_pred,
                         double* h_logit /*or NULL*/);
/* Host-only, for tests and tuning; no result depends on them.  glia_hmt_mlp_limits: the longest row that is staged in LDS under hidden
 * layers of n1 and n2 units (longer rows are read from global memory), the most hidden units a thread accumulates at a time, the waves
 * that split a layer's units, the largest n1 / n2 and the most columns.  glia_hmt_mlp_predict_tile_rows: the rows of a workgroup's tile
 * (64, 32, 16 or 8; below 64 the upper lanes of every wave idle) and whether rows of dim columns are staged. */
int glia_hmt_mlp_limits(int n1, int n2, int* stage_max_dim, int* unit_block, int* slots, int* max_hidden, int* max_dim);
int glia_hmt_mlp_predict_tile_rows(int dim, int n1, int n2, int* staged);
/* Host-only: the most units per hidden layer a model may have inside the classifier loop (glia_hmt_merge_order_bc_mlp). */
int glia_hmt_mlp_loop_limits(int* max_hidden);

/* ---- training the boundary classifier ---------------------------------------------------------------
 * Replaces train_rf (ml/rf/main_train_rf.cxx:18-70): rf_old::train around classRF (ml/rf/ml_rf_train.cxx:234, whose sources the
 * reference tree does not hold) and rf_old::writeModelToBinaryFile (ml/rf/ml_rf_model.cxx:378-455).  The flags, their defaults, the
 * sample-size and class-weight arithmetic (main_train_rf.cxx:11-15,40-61), the mtry default (ml_rf_train.cxx:362,376) and the file
 * format are the reference's; the growing rule is this library's own, deterministic definition -- no parity with
 * classRF's trees is possible or claimed.
 * glia_hmt_train_opts replaces the tool's options (nTree, mTry, sampleSizeRatio, nodeSize, balance) + max_depth (0 = unlimited) and the
 * seed everything random is hashed from. */
typedef struct {
  int ntree;              /* --nt, 255 */
  int mtry;               /* --mt, 0 = floor(sqrt(dim)) */
  double sample_ratio;    /* --sr, 0.7; <= 1e-6: as many draws as rows */
  int nodesize;           /* --ns, 1 */
  int balance;            /* --bal, 1 */
  int max_depth;          /* 0 = unlimited */
  uint64_t seed;          /* 0x9E3779B97F4A7C15 */
} glia_hmt_train_opts;
void glia_hmt_train_opts_default(glia_hmt_train_opts* opts);
/* A trained model on the host: every array of rf_old::Model the model file holds (ml/rf/ml_rf.h:97-156). */
typedef struct glia_hmt_forest_model glia_hmt_forest_model;
/* h_rows: [n_rows][dim] doubles, h_labels: [n_rows]; opts NULL = the defaults.  GLIA_HMT_ERR_ARG with a message: no rows, no columns,
 * a non-finite value, fewer than 2 or more than 8 distinct labels, a sample size outside [1, n_rows], more than 32767 columns.  A plan
 * whose device memory does not fit: GLIA_HMT_ERR_UNSUPPORTED.  Two calls with the same arguments return identical models. */
int glia_hmt_forest_train(glia_hmt_ctx* ctx, const double* h_rows, int64_t n_rows, int dim, const int32_t* h_labels,
                          const glia_hmt_train_opts* opts, glia_hmt_forest_model** out);
/* Host-only: a model from its arrays (tests, converters): tree arrays [ntree][nrnodes] node fastest, treemap [ntree][nrnodes][2],
 * 1-based daughters / variables / classes as the file holds them. */
int glia_hmt_forest_model_from_arrays(int ntree, int nrnodes, int nclass, int mtry, const double* xbestsplit, const int* treemap,
                                      const int* nodestatus, const int* nodeclass, const int* bestvar, const int* ndbigtree,
                                      const double* classwt, const double* cutoff, const int* orig_labels, const int* new_labels,
                                      glia_hmt_forest_model** out);
int glia_hmt_forest_model_sizes(const glia_hmt_forest_model* model, int* ntree, int* nrnodes, int* nclass, int* mtry);
/* copies the arrays (layout as above; any pointer may be NULL) */
int glia_hmt_forest_model_arrays(const glia_hmt_forest_model* model, double* xbestsplit, int* treemap, int* nodestatus, int* nodeclass,
                                 int* bestvar, int* ndbigtree, double* classwt, double* cutoff, int* orig_labels, int* new_labels);
/* rf_old::writeModelToBinaryFile (ml/rf/ml_rf_model.cxx:378-455), every array dense; host-only */
int glia_hmt_forest_model_write(const glia_hmt_forest_model* model, const char* path);
void glia_hmt_forest_model_free(glia_hmt_forest_model* model);
/* alg::RandomForest(predictLabel, modelFile) (alg/rf.hxx:22-33) without the trip through a file: the classifier
 * glia_hmt_forest_predict and glia_hmt_merge_order_bc take. */
int glia_hmt_forest_from_model(glia_hmt_ctx* ctx, const glia_hmt_forest_model* model, int predict_label, glia_hmt_forest** out);
/* the stages of the last glia_hmt_forest_train call of this context (device times from events, ms_total wall clock) */
typedef struct {
  double ms_total, ms_upload, ms_bootstrap, ms_prepare, ms_gather, ms_sort, ms_scan, ms_split, ms_partition, ms_download;
  int64_t levels;            /* tree levels grown, over all batches */
  int64_t launches;
  int64_t batches;           /* groups of trees grown side by side */
  int64_t trees_in_flight;   /* trees of a full batch */
  int64_t nodes;             /* nodes of all trees */
  uint64_t device_bytes;     /* device memory planned for the call */
} glia_hmt_forest_train_timing;
int glia_hmt_last_forest_train_timing(const glia_hmt_ctx* ctx, glia_hmt_forest_train_timing* out);
/* Out-of-bag error and variable importance: classRF's outputs errtr, outcl, counttr, votes, oob_times, importance and importanceSD
 * (sized at ml/rf/ml_rf_train.cxx:112-159, kept in the model at ml/rf/ml_rf.h:131-156).  As with the trees, the values are this
 * library's own deterministic definition; classRF's sources are not in the reference tree and no parity is claimed.
 * oob: the votes of the trees a row is outside the bag of, and the error per tree; importance: mean decrease in accuracy under a
 * permutation of the out-of-bag rows, per class and overall, its standard error, and the mean decrease in Gini (the doImportance
 * switch of ml/rf/ml_rf_train.cxx:112-130).  Both 0: exactly glia_hmt_forest_train. */
typedef struct {
  int oob;                /* 0 */
  int importance;         /* 0 */
} glia_hmt_oob_opts;
void glia_hmt_oob_opts_default(glia_hmt_oob_opts* opts);
/* glia_hmt_forest_train with the out-of-bag passes after every batch of trees; oob_opts NULL = neither.  The model's trees are those of
 * glia_hmt_forest_train with the same train_opts (rf_old::train, ml/rf/ml_rf_train.cxx:234). */
int glia_hmt_forest_train_oob(glia_hmt_ctx* ctx, const double* h_rows, int64_t n_rows, int dim, const int32_t* h_labels,
                              const glia_hmt_train_opts* train_opts, const glia_hmt_oob_opts* oob_opts, glia_hmt_forest_model** out);
/* The sizes the out-of-bag arrays are shaped by (ml/rf/ml_rf_train.cxx:728-784): rows and columns of the training call, and which of
 * the two groups the model holds.  GLIA_HMT_ERR_ARG when it holds neither.  Any pointer may be NULL. */
int glia_hmt_forest_model_oob_sizes(const glia_hmt_forest_model* model, int64_t* n_rows, int* dim, int* has_oob, int* has_importance);
/* Copies the arrays (ml/rf/ml_rf.h:131-156): outcl [n_rows] (1-based class, 0 = never out of bag), counttr [nclass][n_rows], votes
 * [n_rows][nclass], oob_times [n_rows], errtr [ntree][nclass + 1] with the integers it divides err_wrong, err_seen [ntree][nclass + 1]
 * (not part of rf_old::Model), importance [dim][nclass + 2] (per class, all, Gini), importanceSD [dim][nclass + 1].  Any pointer may be
 * NULL; a group the model does not hold is left untouched.  GLIA_HMT_ERR_ARG when it holds neither. */
int glia_hmt_forest_model_oob_arrays(const glia_hmt_forest_model* model, int* outcl, int* counttr, int* votes, int* oob_times, double* errtr,
                                     int64_t* err_wrong, int64_t* err_seen, double* importance, double* importanceSD);
/* Host-only (tests, converters): gives a model its out-of-bag arrays, shaped as above (the slots of ml/rf/ml_rf.h:131-156).  The group
 * outcl / counttr / votes / oob_times / errtr is set when outcl is not NULL (then all five are needed), importance / importanceSD when
 * importance is not NULL; err_wrong / err_seen are left empty.  Replaces what the model held. */
int glia_hmt_forest_model_set_oob(glia_hmt_forest_model* model, int64_t n_rows, int dim, const int* outcl, const int* counttr, const int* votes,
                                  const int* oob_times, const double* errtr, const double* importance, const double* importanceSD);
/* the out-of-bag passes of the last glia_hmt_forest_train_oob call of this context (device times from events; all zero after a call
 * with neither option): the walk of the out-of-bag rows (with the node table and the leaves' in-bag counts), the tally of votes and
 * errors, the permuted walks of the importance.  walks_nominal = sum over trees of out-of-bag rows x columns, walks_done = the walks
 * made after the rule that a variable a row's path never tests needs none (replaces classRF's own timing, none in the reference). */
typedef struct {
  double ms_walk, ms_tally, ms_importance;
  int64_t oob_rows;          /* out-of-bag rows over all trees */
  int64_t walks_nominal, walks_done;
  uint64_t device_bytes;     /* device memory the passes add to the plan */
} glia_hmt_forest_oob_timing;
int glia_hmt_last_forest_oob_timing(const glia_hmt_ctx* ctx, glia_hmt_forest_oob_timing* out);

/* ---- training the MLP / logsig classifier --------------------------------------------------------------
 * Replaces the supervised part of train_sshmt_mlp / train_sshmt_logsig (sshmt/main_train_sshmt_mlp.cxx:96-168): the energy
 * wr * |w|^2 / 2 + ws * (0.5 * L / sigma^2 + n * log(sigma^2) / 2) with L = sum (t_i - f_i)^2 over the rows labelled +1 / -1
 * (type/energy_function.hxx:164-230, alg/function.hxx:171-267), the vanilla / Adam / momentum updates with a fixed or an adaptive step
 * (alg/gd.hxx) and the sigma rule and outer loop of sshmt_util.hxx:140-207.  The arithmetic is this library's own definition
 * (glia_amd/csrc/mlp_backward.hpp): no parity with Eigen's sums, Boost's Gaussian or the OpenMP partial sums is
 * possible or claimed.  The unsupervised term is glia_hmt_sshmt_train's, below; batch samplers are glia_hmt_mlp_train_batches', further
 * below, and altSU is not built: an opts struct that asks for any of them here is GLIA_HMT_ERR_UNSUPPORTED with a message naming the field.  sigma^2 is updated only when update_sigma_s is set (the reference's tool
 * also updates it whenever it runs with --v 0).
 * glia_hmt_mlp_train_opts: the tool's options and defaults; min_sigma2 is the floor the tool passes (0.0); seed keys the initial
 * weights of an MLP (a logsig model starts at zeros; h_init, when given, takes precedence over both). */
typedef struct {
  int n1, n2;                        /* --nn1 10, --nn2 10; 0 / 0: logsig */
  double wr, ws;                     /* --wr 0, --ws 0 */
  double sigma_s;                    /* --ss 0 */
  int update_sigma_s;                /* --uss 0 */
  int optimizer;                     /* --topt 1: vanilla, 2: Adam, 3: momentum */
  double step, step_decay;           /* --lr 0, --lrd 1 (1: fixed step) */
  int fixed_step_decay_iterations;   /* --lrdi -1 */
  int sigma_update_step_period;      /* --lrds -1 */
  int max_iterations;                /* --tw 0 */
  int n_sigma_updates;               /* --ts 0 */
  double pos_target, neg_target;     /* 0.05, 0.95 */
  double min_sigma2;                 /* 0.0 */
  uint64_t seed;                     /* 0 */
  /* glia_hmt_mlp_train refuses anything but the defaults; glia_hmt_sshmt_train honours wu and update_sigma_u and refuses the rest */
  double wu;                         /* --wu 0 */
  int update_sigma_u;                /* --usu 0 */
  int sup_batch_size, uns_batch_size;/* --bss -1, --bsu -1 */
  int balance_sup_batch;             /* --bb 0 */
  int alt_su;                        /* 0 */
} glia_hmt_mlp_train_opts;
void glia_hmt_mlp_train_opts_default(glia_hmt_mlp_train_opts* opts);
/* One evaluation of the optimiser: kind 0 = an iteration (fx, |x|, |g| before its step; step and, with the adaptive rule, the number of
 * roll-backs after it), 1 = the final statistics of a round (the reference's last "gd:" line), 2 = the evaluation that was not finite. */
typedef struct {
  double fx, xnorm, gnorm, step, sigma2;
  int32_t round, t, kind, rollbacks;
} glia_hmt_mlp_train_record;
typedef struct glia_hmt_mlp_model glia_hmt_mlp_model;
/* h_rows [n_rows][dim], h_labels [n_rows]: rows with a label other than +1 / -1 are dropped.  h_min / h_max [dim] (both or neither):
 * rows are rescaled once, as glia_hmt_mlp_predict rescales them.  h_init: the D * N1 + (N1 + 1) * N2 + N2 + 1 (logsig: D) initial weights
 * or NULL.  GLIA_HMT_ERR_ARG with a message, before any kernel: ws and wr both off, sigma_s == 0 without update_sigma_s, n1 == 0 xor
 * n2 == 0, no labelled row, a row or weight that is not finite.  Hidden layers of more than 32 units, rows of more than 384 columns, a
 * memory plan beyond 85 % of the free device memory: GLIA_HMT_ERR_UNSUPPORTED.  If fx or sum g^2 is not finite after an iteration the
 * call stops, restores the weights from before that step and says so in the model (stopped_nonfinite); that is not an error.
 * glia_hmt_mlp_train_host: the same on one host thread, no GPU -- the definition's executable form. */
int glia_hmt_mlp_train(glia_hmt_ctx* ctx, const double* h_rows, int64_t n_rows, int dim, const int32_t* h_labels,
                       const glia_hmt_mlp_train_opts* opts, const double* h_min, const double* h_max, const double* h_init,
                       glia_hmt_mlp_model** out);
int glia_hmt_mlp_train_host(const double* h_rows, int64_t n_rows, int dim, const int32_t* h_labels, const glia_hmt_mlp_train_opts* opts,
                            const double* h_min, const double* h_max, const double* h_init, glia_hmt_mlp_model** out);
/* rounds: sigma rounds whose weights the model holds; n_sigma: entries of glia_hmt_mlp_model_sigmas (one per sigma update) */
int glia_hmt_mlp_model_info(const glia_hmt_mlp_model* model, int* rounds, int64_t* n_weights, int64_t* n_trace, int* stopped_nonfinite,
                            int64_t* n_used_rows, int* n_sigma);
/* round in [0, rounds), or -1: the last.  A model trained with n_sigma_updates == 0 holds one round: the initial weights. */
int glia_hmt_mlp_model_weights(const glia_hmt_mlp_model* model, int round, double* h_w);
int glia_hmt_mlp_model_trace(const glia_hmt_mlp_model* model, glia_hmt_mlp_train_record* h_records);
int glia_hmt_mlp_model_sigmas(const glia_hmt_mlp_model* model, double* h_sigma2, double* h_sigma2_eval);
/* One %.17g double per line: a file that reads back bit for bit (the reference writes the stream's default precision). */
int glia_hmt_mlp_model_write(const glia_hmt_mlp_model* model, const char* path, int round);
/* The classifier glia_hmt_mlp_predict and glia_hmt_merge_order_bc_mlp take, with the min/max table the training used (ctx NULL: host-only). */
int glia_hmt_mlp_model_create_mlp(glia_hmt_ctx* ctx, const glia_hmt_mlp_model* model, int round, glia_hmt_mlp** out);
void glia_hmt_mlp_model_free(glia_hmt_mlp_model* model);
/* Host-only: rows of a chunk of the reduction (part of the definition), the most units per hidden layer, the most columns. */
int glia_hmt_mlp_train_limits(int* chunk_rows, int* max_hidden, int* max_dim);
/* Host-only: the initial weight p of an MLP under seed. */
double glia_hmt_mlp_init_weight(uint64_t seed, uint64_t p);
/* Host-only: the per-column minima and maxima stats::rescale finds over several row blocks (util/stats.hxx:280-314). */
int glia_hmt_rows_minmax(const double* const* h_blocks, const int64_t* n_rows, int n_blocks, int dim, double* h_min, double* h_max);
/* the last glia_hmt_mlp_train call of this context: device times from events, summed over all evaluations */
typedef struct {
  double ms_total, ms_upload;        /* wall clock of the call; rows and targets to the device */
  double ms_weights, ms_chunk, ms_fold, ms_readback;   /* weights up, chunk kernel, fold kernel, L and gradient down */
  int64_t evals, grad_evals;         /* evaluations of L; those that also computed the gradient */
  int64_t iterations;                /* optimiser iterations (trace records of kind 0) */
  uint64_t device_bytes;
} glia_hmt_mlp_train_timing;
int glia_hmt_last_mlp_train_timing(const glia_hmt_ctx* ctx, glia_hmt_mlp_train_timing* out);

/* ---- training with the merge-path (unsupervised) term: train_sshmt_mlp / train_sshmt_logsig ----------------
 * The energy of glia_hmt_mlp_train plus wu * (0.5 * L_U / sigma_u^2 + P * log(sigma_u^2) / 2) between the regulariser and the supervised
 * term (type/energy_function.hxx:164-230).  Each block is one unlabelled volume: a merge order and its feature rows, row i = merge i
 * (sshmt/sshmt_util.hxx:30-52).  The bounded genMergePaths (hmt/tree_build.hxx:150-180) lists P merge paths over all blocks; a path of
 * n rows with classifier outputs f_0 .. f_{n-1} has the monotonic DNF D = 1 - prod_{j=0..n} (merge_target^n - prod_{i<j} f_i
 * prod_{i>=j} (1 - f_i)) (alg/dnf.hxx:126-326), the residual e = path_target^n - D (sshmt/input.hxx:36-39) and L_U = sum e^2
 * (alg/function.hxx:171-267).  sigma_u^2 = max(min_sigma2, L_U / P) under update_sigma_u, updated after sigma_s^2
 * (sshmt_util.hxx:148-222).  Without a single path the term is off (input.hxx:120-121).  The arithmetic is this library's own
 * definition (glia_amd/csrc/sshmt_paths.hpp).  Batch samplers (glia_hmt_sshmt_train_batches, below) and alt_su stay refused
 * by name. */
typedef struct { const double* rows; const uint32_t* order; int64_t n_merges; } glia_hmt_sshmt_block;  /* rows [n_merges][dim], order [n_merges][3] */
typedef struct {
  glia_hmt_mlp_train_opts base;          /* wu and update_sigma_u are honoured HERE; the batch fields and alt_su stay refused */
  double sigma_u;                        /* --su 0 */
  double merge_target, path_target;      /* 0.95, 1.0 (main_train_sshmt_mlp.cxx:41-53) */
  int max_path_length, min_path_length;  /* 3, 2; 1 <= min <= max <= 8 */
} glia_hmt_sshmt_train_opts;
void glia_hmt_sshmt_train_opts_default(glia_hmt_sshmt_train_opts* opts);
/* As glia_hmt_mlp_train, with the unlabelled blocks.  Labelled rows may be absent (n_rows == 0) when base.ws is off.  The same min/max
 * table rescales labelled and unlabelled rows.  GLIA_HMT_ERR_ARG: a block without rows or order, an invalid order (an operand that was
 * merged before or is created later, a created key seen before), a row that is not finite, no term on, wu on with sigma_u == 0 and no
 * update_sigma_u.  GLIA_HMT_ERR_UNSUPPORTED: max_path_length < 0 (unbounded paths) or > 8, the batch fields, the limits of
 * glia_hmt_mlp_train, a memory plan beyond 85 % of the free device memory.  ctx NULL: glia_hmt_sshmt_train_host. */
int glia_hmt_sshmt_train(glia_hmt_ctx* ctx, const double* h_rows, int64_t n_rows, int dim, const int32_t* h_labels,
                         const glia_hmt_sshmt_block* blocks, int n_blocks, const glia_hmt_sshmt_train_opts* opts, const double* h_min,
                         const double* h_max, const double* h_init, glia_hmt_mlp_model** out);
int glia_hmt_sshmt_train_host(const double* h_rows, int64_t n_rows, int dim, const int32_t* h_labels, const glia_hmt_sshmt_block* blocks,
                              int n_blocks, const glia_hmt_sshmt_train_opts* opts, const double* h_min, const double* h_max,
                              const double* h_init, glia_hmt_mlp_model** out);
/* Host-only: the merge paths of one order (hmt/tree_build.hxx:150-180) as CSR.  Call with offsets == members == NULL for *n_paths and
 * *n_members, then with offsets [n_paths + 1] and members [n_members] (merge indices, bottom-up). */
int glia_hmt_merge_paths(const uint32_t* h_order, int64_t n_merges, int max_len, int min_len, int64_t* n_paths, int64_t* n_members,
                         int64_t* offsets, int64_t* members);
/* sigma_u^2 and its evaluated value after every sigma update (n_sigma entries each; 0.0 while the term is off) */
int glia_hmt_mlp_model_sigmas_u(const glia_hmt_mlp_model* model, double* h_sigma2, double* h_sigma2_eval);
int glia_hmt_mlp_model_paths(const glia_hmt_mlp_model* model, int64_t* n_paths, int64_t* n_uns_rows);
/* the last glia_hmt_sshmt_train call of this context: the supervised evaluator's fields, then the unsupervised evaluator's stages */
typedef struct {
  glia_hmt_mlp_train_timing sup;
  double ms_u_upload;                /* unlabelled rows, paths and incidence lists to the device */
  double ms_u_weights, ms_u_forward, ms_u_paths, ms_u_gather, ms_u_chunk, ms_u_fold, ms_u_readback;
  int64_t u_evals, u_grad_evals;
  int64_t n_paths, n_uns_rows;
  uint64_t u_device_bytes;
} glia_hmt_sshmt_train_timing;
int glia_hmt_last_sshmt_train_timing(const glia_hmt_ctx* ctx, glia_hmt_sshmt_train_timing* out);

/* ---- mini-batch training: --bss, --bsu, --bb, --te, --tb of the four trainers -------------------------------
 * An explicit opt-in: the entry points above keep refusing the batch fields by name, because a caller of these accepts THIS library's
 * sampler.  The reference shuffles with std::random_shuffle (type/sampler.hxx:53,120,213), whose rand() state also depends on every
 * shuffled parfor before it (sshmt/sshmt_util.hxx:18,37, sshmt/input.hxx:43): its batch sequence is not a function of its inputs, so
 * no parity is possible or claimed.  Here permutation number s of a stream is a pure function of (seed, stream, s, n) (DESIGN.md
 * 3.17; glia_amd/csrc/mlp_batch.hpp); streams: 0 = merge paths, 1 = labelled rows, 2 + c = class c of a balanced batch.
 * Samplers (sshmt/sshmt_util.hxx:69-107): sup_batch_size B > 0: UniformBatchSampler over the labelled rows (type/sampler.hxx:45-102: a
 * batch that reaches the end of the permutation goes on from its START, then the permutation is reshuffled and the batch ends the
 * epoch); with balance_sup_batch: ClassBatchSampler (type/sampler.hxx:105-233), B / 2 rows of the positive target then B - B / 2 of the
 * negative; balance_sup_batch alone: the smaller class's size from BOTH classes, classes in ascending target; uns_batch_size B > 0:
 * uniform over the merge PATHS.  A step of the optimiser (alg/gd.hxx:86-157) is then epochs_per_iteration epochs of { draw, gradient
 * over the batch, update } -- a draw asks the path sampler, then the row sampler, and ends the epoch when EITHER does
 * (type/energy_function.hxx:42-49) -- or, with epochs_per_iteration <= 0, batches_per_iteration batches.  A term without a sampler takes
 * all its rows in every batch (type/function_input.hxx:119-134).  An iteration still begins with the evaluation over all rows
 * (alg/gd.hxx:59-71,176,226); the adaptive rule's roll-back runs the step again on NEW batches (alg/gd.hxx:242-252). */
typedef struct {
  uint64_t seed;                     /* --bseed */
  int epochs_per_iteration;          /* --te 1 */
  int batches_per_iteration;         /* --tb 1 */
} glia_hmt_batch_opts;
void glia_hmt_batch_opts_default(glia_hmt_batch_opts* opts);
/* glia_hmt_mlp_train / glia_hmt_sshmt_train with opts' sup_batch_size, uns_batch_size and balance_sup_batch honoured (ctx NULL: on one
 * host thread, the definition).  With no sampler asked for they return what those return, byte for byte.  GLIA_HMT_ERR_ARG: fewer
 * labelled rows or paths than the batch size ("Error: totalSize must be greater than batchSize"), a class without a row or with fewer
 * rows than its share (the reference reads out of range there), equal targets under balance_sup_batch, a sampler for a term that is
 * off.  alt_su stays GLIA_HMT_ERR_UNSUPPORTED.  On the device the batches of a step run back to back on the stream, weights and
 * optimiser state in device memory, one wait per step; option GLIA_HMT_BATCH = step runs one batch per evaluation with the update on
 * the host instead and gives the same bytes. */
int glia_hmt_mlp_train_batches(glia_hmt_ctx* ctx, const double* h_rows, int64_t n_rows, int dim, const int32_t* h_labels,
                               const glia_hmt_mlp_train_opts* opts, const glia_hmt_batch_opts* batch, const double* h_min, const double* h_max,
                               const double* h_init, glia_hmt_mlp_model** out);
int glia_hmt_sshmt_train_batches(glia_hmt_ctx* ctx, const double* h_rows, int64_t n_rows, int dim, const int32_t* h_labels,
                                 const glia_hmt_sshmt_block* blocks, int n_blocks, const glia_hmt_sshmt_train_opts* opts,
                                 const glia_hmt_batch_opts* batch, const double* h_min, const double* h_max, const double* h_init,
                                 glia_hmt_mlp_model** out);
/* Host-only: the next k draws of the samplers.  h_labels [n_rows]: +1 / -1 of the labelled rows in the trainer's order (every row
 * counts); n_paths merge paths.  Call with the four arrays NULL for *n_sup and *n_uns (entries over all k draws), then with
 * sup_offsets [k + 1], sup_rows [*n_sup], uns_offsets [k + 1], uns_paths [*n_uns]; end_of_epoch [k] (or NULL): whether draw i ended the
 * epoch.  A sampler that was not asked for leaves its lists empty. */
int glia_hmt_batch_plan(const int32_t* h_labels, int64_t n_rows, int64_t n_paths, int sup_batch_size, int uns_batch_size,
                        int balance_sup_batch, double pos_target, double neg_target, uint64_t seed, int k, int64_t* n_sup, int64_t* n_uns,
                        int64_t* sup_offsets, int32_t* sup_rows, int64_t* uns_offsets, int32_t* uns_paths, int32_t* end_of_epoch);
/* the last *_train_batches call of this context; option GLIA_HMT_BATCH = stream (default) | step, read per call */
enum { GLIA_HMT_BATCH_STREAM = 0, GLIA_HMT_BATCH_STEP = 1 };
typedef struct {
  int64_t steps, batches;            /* mini-batch steps (each in the place of one update); batches over all of them */
  double ms_plan, ms_upload;         /* the host builds the plans of the steps; their copies to the device (one per step) */
  double ms_steps;                   /* device time of the steps, from events (route step: wall clock of its evaluations and updates) */
  double ms_wall;                    /* wall clock of the steps, all of the above and the waits included */
  int64_t syncs;                     /* waits for the stream inside the steps: one per step on the stream route */
  int32_t route;                     /* GLIA_HMT_BATCH_STREAM | GLIA_HMT_BATCH_STEP */
  uint64_t plan_bytes;               /* the largest plan */
} glia_hmt_batch_timing;
int glia_hmt_last_batch_timing(const glia_hmt_ctx* ctx, glia_hmt_batch_timing* out);

/* Length of one feature vector for the configuration the rag was built with (BoundaryClassificationFeats::dim,
 * hmt/bc_feat.hxx:225-230; or selectFeatures' length with --simpf). */
int glia_hmt_feat_dim(const glia_hmt_rag* rag);

/* Replaces genMergeOrderGreedyUsingBoundaryClassifier (util/struct_merge_bc.hxx:45-58) with the fBcFeat / fBcPred
 * pair of hmt/main_merge_order_bc.cxx:54-137 (bcType 1).  The rag must have been built with a feature
 * configuration and only_contour = 0.  h_feats (optional, [capacity][feat_dim]) receives the feature vector each
 * merged edge was scored with (the -b output, :148-157). */
int glia_hmt_merge_order_bc(glia_hmt_ctx* ctx, glia_hmt_rag* rag, const glia_hmt_forest* forest, uint32_t* h_order,
                            double* h_saliency, double* h_feats, int64_t capacity, int64_t* n_merges);
/* The same loop with the second classifier of hmt/main_merge_order_bc.cxx:111-139 (bcType 2): alg::MLP2v, or three of them behind
 * the ThresholdModelDistributor, which reads the RESCALED, bias-appended vector.  The saliency of an edge is the probability
 * 1 / (1 + exp(-logit)) with the arithmetic of glia_hmt_mlp_predict_host and the host's exp (glia_hmt_ctx_libm_exp):
 * a saturated model gives many edges exactly 1.0 and the tie rule decides among them, as in the reference.  h_feats receives the raw
 * rows (not rescaled).  The loop's own workgroup scores; helper workgroups serve forests only.
 * GLIA_HMT_ERR_ARG with a message, before any kernel: a model with more than glia_hmt_mlp_loop_limits units in a hidden layer, the
 * logsig model (0 / 0), glia_hmt_mlp_dim != glia_hmt_feat_dim of the rag, a model not created on this context's device.  The median
 * layout is refused as for the forest. */
int glia_hmt_merge_order_bc_mlp(glia_hmt_ctx* ctx, glia_hmt_rag* rag, const glia_hmt_mlp* mlp, uint32_t* h_order,
                                double* h_saliency, double* h_feats, int64_t capacity, int64_t* n_merges);

/* Replaces the merge engine of pre_merge (gadget/main_pre_merge.cxx:20-76): pb-mean linkage with updateRegion = true
 * and the size condition -- an edge may merge only if its smaller region has fewer than size_thresholds[0] voxels, or
 * (n_thresholds == 2) a region smaller than size_thresholds[1] has mean pb above rpb_threshold.  The region map must
 * have been built with only_contour = 0 and the pb image.  Relabelling the volume (transformKeys/transformImage,
 * :77-79) stays with the caller. */
int glia_hmt_pre_merge(glia_hmt_ctx* ctx, glia_hmt_rag* rag, const int* size_thresholds, int n_thresholds,
                       double rpb_threshold, uint32_t* h_order, double* h_saliency, int64_t capacity, int64_t* n_merges);

/* Replaces the bc_feat pipeline (hmt/main_bc_feat.cxx:27-112) for a GIVEN merge order: RegionMap(seg, mask, order,
 * false) + RegionFeats of every tree node + BoundaryFeats of every merge (the OpenMP parfor loops of :59-101),
 * without the optional saliency features (see glia_hmt_bc_feat_saliency).  h_order: n_merges triples (x0, x1, x2); h_feats: [n_merges][feat_dim],
 * row i = features of merge i with regions in the file's orientation and the area-ordered swap of :88-91. */
int glia_hmt_bc_feat(glia_hmt_ctx* ctx, glia_hmt_rag* rag, const uint32_t* h_order, int64_t n_merges, double* h_feats);
/* The same with the saliency features of bc_feat -y/--s0/--sb (hmt/main_bc_feat.cxx:50-55, genSaliencyMap
 * hmt/bc_feat.hxx:12-26): h_saliencies[i] belongs to merge i; rows then have glia_hmt_bc_feat_dim(rag, 1) columns
 * (5 more: two in the boundary block, one per region block; none for the simple selection). */
int glia_hmt_bc_feat_saliency(glia_hmt_ctx* ctx, glia_hmt_rag* rag, const uint32_t* h_order, int64_t n_merges,
                              const double* h_saliencies, double init_saliency, double saliency_bias, double* h_feats);
int glia_hmt_bc_feat_dim(const glia_hmt_rag* rag, int with_saliency);
/* The same rows by a second route, parallel over merges as the reference's own loops are (hmt/main_bc_feat.cxx:59-95 under the
 * parfor of util/mp.hxx:24-106): the order is given, so the merge tree is known before any statistic is combined, and every set a
 * row looks at is computed for all tree nodes at once (glia_amd/csrc/bc_feat_batch.hip).  Arguments, row width
 * (glia_hmt_bc_feat_dim) and errors are those of glia_hmt_bc_feat_saliency; h_saliencies may be NULL.  Rows are identical to the replay's wherever the sums are exact (quantised images) and
 * within 1e-12 in the mean / standard deviation columns otherwise (another association of the f64 sums); two calls on one map
 * return identical bytes.  Trees whose tables exceed the memory bound of DESIGN 7: GLIA_HMT_ERR_UNSUPPORTED.
 * Option GLIA_HMT_BCFEAT = replay (default) | batch (glia_hmt_set_option or the environment) sends glia_hmt_bc_feat and
 * glia_hmt_bc_feat_saliency down this route. */
int glia_hmt_bc_feat_batch(glia_hmt_ctx* ctx, glia_hmt_rag* rag, const uint32_t* h_order, int64_t n_merges,
                           const double* h_saliencies, double init_saliency, double saliency_bias, double* h_feats);
/* the stages of the last bc_feat call on this map, whichever route it took */
enum { GLIA_HMT_BCFEAT_REPLAY = 0, GLIA_HMT_BCFEAT_BATCH = 1 };
typedef struct {
  double ms_plan;          /* batch: host plan (tree tables, uploads); replay: 0 */
  double ms_sets;          /* batch: device time of the sets of all tree nodes; replay: table + initial state of the loop */
  double ms_rows;          /* batch: device time of the row kernel; replay: the loop */
  int64_t height;          /* batch: height of the merge tree (levels of the bottom-up pass); replay: 0 */
  int64_t launches;        /* batch: kernel launches of the call; replay: 0 */
  int64_t path_updates;    /* batch: table updates of the min / max lifting (two per entry and channel); replay: 0 */
  int route;               /* GLIA_HMT_BCFEAT_REPLAY | GLIA_HMT_BCFEAT_BATCH */
} glia_hmt_bc_feat_timing;
int glia_hmt_last_bc_feat_timing(const glia_hmt_rag* rag, glia_hmt_bc_feat_timing* out);

/* Replaces hmt/main_bc_label_ri.cxx:27-153 and hmt/main_bc_label_vi.cxx:27-128 for a GIVEN merge order: the label of every merge,
 * GLIA_HMT_BC_MERGE (-1) or GLIA_HMT_BC_SPLIT (+1), decided against truth volumes (genBoundaryClassificationLabelF1 / RI / VI,
 * hmt/bc_label.hxx:16-109; stats::pairStats / pairF1 / randIndex / vi, util/image_stats.hxx:69-110,173-245, util/stats.hxx:189-261;
 * truth label 0 excluded).  The region sets are those of RegionMap(seg, mask, order, false): the map must be a whole-volume build
 * with only_contour = 0 (else GLIA_HMT_ERR_UNSUPPORTED / GLIA_HMT_ERR_ARG); the mask given to the build is the tools' -n / -m.
 * d_truth: n_truth device volumes of the map's shape (u32); several only for GLIA_HMT_BC_LABEL_VI (majority, util/container.hxx:356).
 * h_order: n_merges triples validated as glia_hmt_bc_feat does; h_labels: [n_merges], row i = merge i (with global_opt: the inner
 * nodes of genTree, which are the merges in order).  opts NULL = the tools' defaults.  Labels are exact; the F1 / RI values behind
 * them are too up to counts beyond 2^53 (converted to double rounded to nearest; the reference's int512_t conversion is not pinned),
 * VI values are sums in another order than the reference's hash order. */
enum { GLIA_HMT_BC_LABEL_F1 = 0, GLIA_HMT_BC_LABEL_RI = 1, GLIA_HMT_BC_LABEL_VI = 2 };
#define GLIA_HMT_BC_MERGE (-1)
#define GLIA_HMT_BC_SPLIT 1
typedef struct {
  int metric;              /* GLIA_HMT_BC_LABEL_F1 (bc_label_ri, --f1 true), _RI (bc_label_ri --f1 false), _VI (bc_label_vi) */
  int tweak;               /* bc_label_ri --tweak (-w): F1 only */
  double max_prec_drop;    /* bc_label_ri --mpd (-d), >= 1 disables: F1 only */
  int opt_split;           /* bc_label_ri --optSplit (-p): F1 only (ignored with RI, as by the reference) */
  int global_opt;          /* --opt (-g): 0 none, 1 path consistency by merging, 2 by splitting; with 1 / 2 the RI tool compares
                              pair F1 whatever the metric (main_bc_label_ri.cxx:121-124) and ignores tweak / mpd / optSplit */
} glia_hmt_bc_label_opts;
int glia_hmt_bc_label(glia_hmt_ctx* ctx, glia_hmt_rag* rag, const uint32_t* const* d_truth, int n_truth, const uint32_t* h_order,
                      int64_t n_merges, const glia_hmt_bc_label_opts* opts, int32_t* h_labels);
/* the stages of the last glia_hmt_bc_label call on this map */
typedef struct {
  double ms_count;         /* device time of the counting pass(es), all truth volumes (label_overlap.hip) */
  double ms_nodes;         /* host: per-node values (small-to-large merging) */
  double ms_rules;         /* host: the label rules */
  int64_t entries;         /* (leaf, truth) entries of the contingency tables, truth 0 included */
  int64_t moves;           /* map entries moved by the small-to-large merging */
  int64_t node_pairs;      /* (tree node, truth != 0) pairs: the visits of a per-node walk */
} glia_hmt_bc_label_timing;
int glia_hmt_last_bc_label_timing(const glia_hmt_rag* rag, glia_hmt_bc_label_timing* out);

/* ---- the step after the merge path: tree resolution (hmt/main_segment_greedy.cxx:33-86), host-only ----
 * glia_hmt_tree_potentials = genTree / genTreeWithNodePotentials (hmt/tree_build.hxx:12-63): array tree of the merge
 * order plus a potential per node -- merge probability of the node, times (1 - p) of its parent; leaves: (1 - p_parent)^2;
 * the root (= last node) squared; optionally times max(region_prob[node], FEPS).  h_merge_probs == NULL: all 1.0.
 * Returns the number of nodes. */
int64_t glia_hmt_tree_potentials(const uint32_t* h_order, int64_t n_merges, const double* h_merge_probs,
                                 const double* h_region_probs, uint32_t* node_label, int32_t* parent, int32_t* child0,
                                 int32_t* child1, double* potential, int64_t capacity);
/* resolveTreeGreedy (hmt/tree_greedy.hxx:36-70,104-152 for one tree, comp = potential <): repeatedly picks the valid
 * node of highest potential (first in node order among equals) and invalidates its ancestors and descendants.
 * h_picks receives node indices in pick order; returns their number. */
int64_t glia_hmt_resolve_tree_greedy(const int32_t* parent, const int32_t* child0, const int32_t* child1,
                                     const double* potential, int64_t n_nodes, int32_t* h_picks, int64_t capacity);
/* The same over several trees (alternative merge orders of overlapping supervoxel sets; hmt/tree_greedy.hxx:104-152):
 * per-tree arrays are passed as arrays of pointers; picks come out as (tree, node) pairs in pick order. */
int64_t glia_hmt_resolve_trees_greedy(int n_trees, const int64_t* n_nodes, const uint32_t* const* node_label,
                                      const int32_t* const* parent, const int32_t* const* child0, const int32_t* const* child1,
                                      const double* const* potential, int32_t* h_pick_tree, int32_t* h_pick_node, int64_t capacity);
/* genLabelTransform (hmt/tree_segment.hxx:10-21): every leaf label under pick k maps to key_to_assign + k.  The pairs
 * feed glia_hmt_transform_image (fill_missing = 1 reproduces segment_greedy's default --ignore true). */
int64_t glia_hmt_label_transform(const uint32_t* node_label, const int32_t* child0, const int32_t* child1, int64_t n_nodes,
                                 const int32_t* h_picks, int64_t n_picks, uint32_t key_to_assign, uint32_t* h_src,
                                 uint32_t* h_dst, int64_t capacity);

/* ---- tree inference of segment_ccm (hmt/main_segment_ccm.cxx, hmt/tree_ccm.hxx), host-only ----
 * glia_hmt_tree_energies = genTree with the node energies of main_segment_ccm.cxx:39-51 + computeEnergyTuples (tree_ccm.hxx:12-27).
 * Node arrays as glia_hmt_tree_potentials lays them out; inner nodes consume h_merge_probs in merge order.  Per node: its own
 * em / es (leaf: 0 / FMAX; inner node with merge probability p: em = isfeq(p, 0) ? FMAX : -log(p), es likewise from 1 - p) and the
 * tuples Em = em + sum Em(child), Es = es + sum min(Em(child), Es(child)), children in the order child0, child1, every sum through
 * the saturating stats::plusEqual (util/stats.hxx:9-17).  Returns the number of nodes. */
int64_t glia_hmt_tree_energies(const uint32_t* h_order, int64_t n_merges, const double* h_merge_probs, uint32_t* node_label,
                               int32_t* parent, int32_t* child0, int32_t* child1, double* em, double* es, double* Em, double* Es,
                               int64_t capacity);
/* computeEnergyTuples alone (tree_ccm.hxx:12-27), for given own energies: what glia_hmt_tree_energies runs after the energies. */
int glia_hmt_tree_energy_tuples(const int32_t* child0, const int32_t* child1, const double* em, const double* es, int64_t n_nodes,
                                double* Em, double* Es);
/* resolveFactorTree (tree_ccm.hxx:31-47): breadth-first from the last node; a node with Em < Es is picked (a tie splits), else its
 * children are queued, child0 first.  h_picks receives node indices in pick order; returns their number. */
int64_t glia_hmt_resolve_tree_ccm(const int32_t* child0, const int32_t* child1, const double* Em, const double* Es, int64_t n_nodes,
                                  int32_t* h_picks, int64_t capacity);
/* The node value of segment_ccm -b (main_segment_ccm.cxx:76-86): pos / plusEqual(neg, pos) with pos = computeFactorNodeEnergyPositive
 * and neg = computeFactorNodeEnergyNegative (tree_ccm.hxx:62-115), every sum in the reference's own order (O(nodes * depth), like
 * the reference).  pos / neg / confidence: [n_nodes], pos and neg may be NULL.  The confidence array is the `potential` of
 * glia_hmt_boundary_confidence. */
int glia_hmt_tree_ccm_confidence(const int32_t* parent, const int32_t* child0, const int32_t* child1, const double* es, const double* Em,
                                 const double* Es, int64_t n_nodes, double* pos, double* neg, double* confidence);

/* genBoundaryConfidenceImage with all tree nodes (hmt/tree_segment.hxx:66-203; segment_greedy -b): every voxel on a
 * directed boundary of two supervoxels receives the largest (float) node potential among the tree nodes whose region
 * still owns an entry of that supervoxel pair; every other voxel 0.  rag: the region map of the segmentation image
 * (glia_hmt_rag_build, whole volume); trees as produced by glia_hmt_tree_potentials; d_out: float volume. */
int glia_hmt_boundary_confidence(glia_hmt_ctx* ctx, glia_hmt_rag* rag, int n_trees, const int64_t* n_nodes,
                                 const uint32_t* const* node_label, const int32_t* const* parent, const int32_t* const* child0,
                                 const double* const* potential, float* d_out);

/* ---- label-volume rewrites either side of the path (gadget/main_pre_merge.cxx:77-79, gadget/main_apply_merges.cxx:28-34) ----
 * transformKeys (util/struct_merge.hxx:188-210): every key that is merged and is not itself created by a merge maps
 * to the key it finally ends up in.  Host-only; pairs come out sorted by source key.  Returns the number of pairs
 * (capacity: 2 * n_merges is always enough) or a negative status. */
int64_t glia_hmt_transform_keys(const uint32_t* h_order, int64_t n_merges, uint32_t* h_src, uint32_t* h_dst, int64_t capacity);

/* transformImage (util/image.hxx:227-242 and :246-257): rewrites d_labels IN PLACE -- every voxel whose mask value is
 * not MASK_OUT_VAL (0; d_mask may be NULL) and whose label has an entry in (h_src -> h_dst) receives the mapped label;
 * labels without an entry are kept, or set to BG_VAL (0) when fill_missing != 0.  Volumes must be 16-byte aligned. */
int glia_hmt_transform_image(glia_hmt_ctx* ctx, uint32_t* d_labels, int64_t n_voxels, const uint32_t* h_src,
                             const uint32_t* h_dst, int64_t n_map, const uint32_t* d_mask, int fill_missing);

/* relabelImage (util/image.hxx:992-1001) = itk::RelabelComponentImageFilter, in place: objects (labels != 0) get the
 * consecutive labels 1..n by decreasing voxel count (ties: smaller original label first), objects smaller than
 * min_size (> 0) become 0.  ITK is not available to pin this against. */
int glia_hmt_relabel_image(glia_hmt_ctx* ctx, uint32_t* d_labels, int64_t n_voxels, int64_t min_size, uint32_t* n_labels);

/* milliseconds of the last glia_hmt_transform_image kernel on this context (HIP events) */
double glia_hmt_last_transform_ms(const glia_hmt_ctx* ctx);

/* Replaces hmt::genTree (hmt/tree_build.hxx:12-38): merge order -> array tree (children before parents, root last).
 * Host-only.  Returns the number of nodes (2 * n_merges + 1 for one connected tree) or a negative status. */
int64_t glia_hmt_gen_tree(const uint32_t* h_order, int64_t n_merges, uint32_t* node_label, int32_t* parent,
                          int32_t* child0, int32_t* child1, int64_t capacity);

/* TBoundaryTable::init with the classifier linkage only (type/boundary_table.hxx:91-114 driven by
 * util/struct_merge_bc.hxx:18-27): feature vector + score of every initial table edge, no merging.
 * *ms = device time of the feature + forest kernel. */
int glia_hmt_score_initial_edges(glia_hmt_ctx* ctx, glia_hmt_rag* rag, const glia_hmt_forest* forest,
                                 int64_t* n_edges, double* ms);
/* The same, sharded for several GPUs (scoring of the initial edges is independent per edge): this call
 * scores the records e with e % n_shards == shard.  h_scores[e] (e < *n_records, one record per unordered adjacent
 * leaf pair in lexicographic order) = P(merge) for the table edges of the shard, -inf for every other record; the
 * element-wise maximum over the shards is the full result.  h_scores may be NULL to query *n_records (<= directed pairs). */
int glia_hmt_score_initial_edges_shard(glia_hmt_ctx* ctx, glia_hmt_rag* rag, const glia_hmt_forest* forest, int shard,
                                       int n_shards, double* h_scores, int64_t capacity, int64_t* n_records);
/* The same with the MLP (hmt/main_merge_order_bc.cxx:111-139); the limits of glia_hmt_merge_order_bc_mlp apply. */
int glia_hmt_score_initial_edges_shard_mlp(glia_hmt_ctx* ctx, glia_hmt_rag* rag, const glia_hmt_mlp* mlp, int shard,
                                           int n_shards, double* h_scores, int64_t capacity, int64_t* n_records);

/* Phase timings of the last merge_order_* call on this rag (ms): edge-table build, init, greedy loop. */
int glia_hmt_last_merge_timing(const glia_hmt_rag* rag, double* ms_table, double* ms_init, double* ms_loop,
                               int64_t* n_edges_scored);

/* ---- the step before the path: watershed over-segmentation (gadget/main_watershed.cxx, util/image_alg.hxx:9-21) ----------
 * glia::watershed = itk::MorphologicalWatershedImageFilter(level, MarkWatershedLineOff, face connectivity): h-minima transform
 * of the image (minima shallower than `level` vanish), regional minima as markers numbered in raster order, flooding without
 * watershed lines.  ITK decides flooding ties by the arrival order of a sequential hierarchical queue; here every tie has an
 * order-free rule (lowest flood level, then shortest way on the plateau, then smaller label), so labels are reproducible but
 * NOT pinned against ITK (absent from this image).  d_labels: uint32 volume, labels 1..*n_labels; *sweeps (optional): whole-volume
 * passes it took. */
int glia_hmt_watershed(glia_hmt_ctx* ctx, int dim, const int64_t dims[3], const float* d_image, double level, uint32_t* d_labels,
                       uint32_t* n_labels, int* sweeps);

/* ---- face-connected components of a label volume (gadget/main_labelicc_image.cxx, gadget/main_labelcc_image.cxx) ----------
 * A component is a maximal face-connected set of voxels that take part (4 neighbours in 2D, 6 in 3D, in the reference order
 * -x, +x, -y, +y, -z, +z of type/neighbor.hxx:72-89; the order does not influence the result).  Components are numbered
 * 1..*n_components in raster order of their first voxel (x fastest); every other voxel gets BG_VAL (0).
 *   GLIA_HMT_CC_IDENTITY         labelIdentityConnectedComponents (util/image.hxx:331-373, "Used to relabel 3D label sub-volume
 *                                cut from bigger volume"): a voxel takes part if its label != 0 and it is not masked out; two
 *                                neighbours are joined if both take part and their labels are equal.  Pinned exactly.
 *   GLIA_HMT_CC_BINARY           labelConnectedComponents (util/image.hxx:302-313) = itk::ConnectedComponentImageFilter with
 *                                SetFullyConnected(false): takes part if label != 0 and not masked out; neighbours are joined if
 *                                both take part.  The partition is the filter's; ITK's label ORDER is unpinned.
 *   GLIA_HMT_CC_BINARY_INVERTED  labelcc_image --invert (gadget/main_labelcc_image.cxx:10-18): takes part if label == 0 and not
 *                                masked out; otherwise as GLIA_HMT_CC_BINARY.
 * d_mask: u32 volume or NULL; MASK_OUT_VAL (0) masks a voxel out: it is never a start and never a neighbour (image.hxx:349,
 * type/neighbor.hxx:80-86) and its output is 0.  The reference gives only the identity mode a mask; accepting one in the binary
 * modes is an extension.  dims as for glia_hmt_watershed (dims[2] ignored when dim == 2); between 1 and 2^32 - 2 voxels.
 * d_labels_out must not be d_labels_in: the volume cannot be labelled in place (tile borders are merged from the input labels
 * while other workgroups already write).  GLIA_HMT_ERR_ARG, message "label_components: ...", before any HIP call for: a NULL ctx,
 * dims, input, output or n_components; dim other than 2 or 3; a non-positive extent or a size outside the range; a mode outside
 * 0..2; d_labels_out == d_labels_in; an unknown value of the option GLIA_HMT_CC.
 * Option GLIA_HMT_CC = tiled (default) | global: two routes to the same bytes -- tile-local union-find in LDS, tile faces united in
 * global memory; or every voxel pair united in global memory (the cross-check). */
enum { GLIA_HMT_CC_IDENTITY = 0, GLIA_HMT_CC_BINARY = 1, GLIA_HMT_CC_BINARY_INVERTED = 2 };
int glia_hmt_label_components(glia_hmt_ctx* ctx, int dim, const int64_t dims[3], const uint32_t* d_labels_in,
                              const uint32_t* d_mask, int mode, uint32_t* d_labels_out, uint32_t* n_components);

/* ---- scoring a label volume against truth (gadget/main_eval_ri.cxx, gadget/main_eval_vi.cxx) ----------
 * glia_hmt_label_overlap is the table the reference's evaluation family shares: the loops of stats::pairStats and stats::centropy on
 * images (util/image_stats.hxx:248-273, :122-158) and stats::getOverlap (:308-335) each walk two label images and a mask and count
 * the voxels of every label pair in an unordered_map.  d_a (proposed) and d_b (reference) are u32 streams of n_voxels -- 2D and 3D
 * are the same call --, 1 <= n_voxels <= 2^32 - 2; d_mask (optional, u32): MASK_OUT_VAL = 0 drops the voxel; flags drop the voxels
 * with a == 0 / b == 0 (the `excluded` sets {BG_VAL} of the callers).  Labels are arbitrary 32-bit values on both sides.
 * h_entries receives the pairs with count > 0, ascending by (a, b); two calls on the same input return identical bytes.
 * *n_entries = their number; more than `capacity`: GLIA_HMT_ERR_CAPACITY, *n_entries still set, h_entries untouched (h_entries may be
 * NULL when capacity is 0).  Vector loads need d_a, d_b and d_mask 16-byte aligned; other pointers take a scalar path to the same
 * result.  GLIA_HMT_ERR_ARG, message "label_overlap: ...", before any HIP call for: a NULL ctx, volume or n_entries, NULL h_entries
 * with capacity > 0, capacity < 0, n_voxels outside the range, unknown flag bits. */
#define GLIA_HMT_OVERLAP_DROP_ZERO_A 1
#define GLIA_HMT_OVERLAP_DROP_ZERO_B 2
typedef struct {
  uint32_t a, b;
  uint64_t count;
} glia_hmt_overlap_entry;
int glia_hmt_label_overlap(glia_hmt_ctx* ctx, const uint32_t* d_a, const uint32_t* d_b, const uint32_t* d_mask, int64_t n_voxels,
                           int flags, glia_hmt_overlap_entry* h_entries, int64_t capacity, int64_t* n_entries);

/* Host-only (no ctx, no HIP call): the numbers eval_ri and eval_vi print, from the tables of one or more image pairs.  The entries
 * are taken as given -- whatever filtering the caller applied has already happened --; a (a, b) pair occurs once per table and
 * counts are > 0 (a zero count is GLIA_HMT_ERR_ARG).
 * Pair counts (stats::pairStats, util/stats.hxx:189-229): per table n = sum of counts, TP = sum c (c - 1) / 2, pairs of equal a /
 * equal b from the marginals, TN / FP / FN as :225-228; the four are SUMMED over the tables before any ratio is taken
 * (main_eval_ri.cxx:41-47) and returned as 128-bit integers in lo / hi words.  precision, recall, rand_index (util/stats.hxx:232-256)
 * keep the guard den = isfeq(den, 0) ? den + FEPS : den, FEPS = 2.22e-16; f1 = 2 p r / (p + r) (:259-261) is NaN at 0 / 0, as in the
 * reference.  Integer -> double conversions are exact up to 2^53 and round to nearest above (the reference converts Boost's
 * int512_t, whose rounding is not pinned).
 * Entropies (stats::centropy, util/image_stats.hxx:122-158): per table false_split = H(a | b) = sum c_ab log2(q) / n with q = n_b / c_ab,
 * false_merge = H(b | a) likewise with n_a; the result is stats::mean over the tables (main_eval_vi.cxx:26).  The reference computes
 * std::log2(up.second / bp.second) on two `uint`s (:153): q is the INTEGER quotient floor(marginal / c_ab).  GLIA_HMT_VI_REFERENCE
 * reproduces that (what the reference tool prints; the tools' default); GLIA_HMT_VI_EXACT takes the real quotient as a double --
 * the conditional entropy of the textbook.  The two agree when every quotient is an integer.  log2 is the host libm's.  Terms are
 * added in entry order, in double; the reference adds them in unordered_map order, so its own last bits are not pinned: every
 * term is >= 0 (q >= 1), a sum over E entries is within about E * 2^-53 relative of the correctly rounded one.
 * No voxel selected (all tables empty): 0 / 0 = NaN for the entropies and f1, 0 for precision and recall, 0 / FEPS = 0 for
 * rand_index -- what the C++ returns; not an error.  GLIA_HMT_ERR_ARG, message "eval: ...": n_tables < 1, a NULL argument, a
 * negative length, an unknown mode. */
enum { GLIA_HMT_VI_REFERENCE = 0, GLIA_HMT_VI_EXACT = 1 };
typedef struct {
  uint64_t tp_lo, tp_hi, tn_lo, tn_hi, fp_lo, fp_hi, fn_lo, fn_hi;   /* pairs: value = hi * 2^64 + lo */
  double precision, recall, f1, rand_index;
  double false_split, false_merge;
} glia_hmt_eval_result;
int glia_hmt_overlap_scores(const glia_hmt_overlap_entry* const* h_tables, const int64_t* n_entries, int n_tables, int vi_mode,
                            glia_hmt_eval_result* out);

/* Replaces the operation() of gadget/main_eval_ri.cxx:9-61 and gadget/main_eval_vi.cxx:7-29 for volumes on the device: one counting
 * pass per image pair with GLIA_HMT_OVERLAP_DROP_ZERO_B (excluded1 = {BG_VAL}: masked-out voxels and voxels with reference label 0
 * are dropped, the proposed label 0 counts as a label), then glia_hmt_overlap_scores.  d_res / d_ref: n_images device pointers,
 * n_voxels[i] voxels each; d_mask: NULL, or n_images pointers of which any may be NULL (main_eval_ri.cxx:34).  Errors as the two
 * calls above, message "eval: ...". */
int glia_hmt_eval(glia_hmt_ctx* ctx, int n_images, const uint32_t* const* d_res, const uint32_t* const* d_ref,
                  const uint32_t* const* d_mask, const int64_t* n_voxels, int vi_mode, glia_hmt_eval_result* out);
/* the counting passes of the last glia_hmt_label_overlap or glia_hmt_eval call on this context */
typedef struct {
  double ms_count;         /* device time of the counting kernel, every pass of every image pair (label_overlap.hip) */
  int64_t entries;         /* entries of the tables */
  int64_t repeats;         /* passes repeated because the global table filled up */
} glia_hmt_eval_timing;
int glia_hmt_last_eval_timing(const glia_hmt_ctx* ctx, glia_hmt_eval_timing* out);

/* ---- smoothing the probability map before the watershed (gadget/main_blur_image.cxx, blurImage util/image.hxx:376-407) ----------
 * blurImage is itk::DiscreteGaussianImageFilter(variance = sigma^2, MaximumKernelWidth = w); with a dimension argument
 * (util/image.hxx:389-407) the filter of one dimension less runs slice by slice.  ITK is absent from this image, so -- as for the
 * watershed -- the operator is defined here and every route reproduces that definition bit for bit; parity with
 * ITK's last digits is NOT claimed (its Bessel values are polynomial fits good to about 1e-7, the ones here are exact to rounding;
 * the cut-off rule is itk::GaussianOperator's as understood, unpinned).
 *
 * glia_hmt_gaussian_kernel (host-only, no ctx, no HIP call) replaces itk::GaussianOperator::GenerateCoefficients for one axis:
 * T(n) = exp(-variance) I_n(variance) by the power series of I_n in double; c = [T(0), T(1)], then T(i) is appended while the covered
 * mass c0 + 2 (c1 + ...) stays below 1 - max_error, stopping after an append that is <= 0 or that makes the one-sided length exceed
 * max_width; every entry is divided by the covered mass.  coeffs[0..*radius] (one-sided; 1 <= *radius <= max_width), *covered = the
 * mass before the division (optional).  A kernel cut by max_width is not an error.  GLIA_HMT_ERR_ARG, message "gaussian_kernel: ...":
 * NULL coeffs or radius, variance not in (0, GLIA_HMT_BLUR_MAX_VARIANCE], max_width not in 1..GLIA_HMT_BLUR_MAX_WIDTH, max_error not in
 * (0, 1); GLIA_HMT_ERR_CAPACITY (with *radius set): capacity < *radius + 1. */
#define GLIA_HMT_BLUR_MAX_VARIANCE 256.0
#define GLIA_HMT_BLUR_MAX_WIDTH 128
#define GLIA_HMT_BLUR_MAX_ERROR 0.01 /* ITK's default MaximumError: what blur_image and the two calls below use */
int glia_hmt_gaussian_kernel(double variance, int max_width, double max_error, double* coeffs, int capacity, int* radius, double* covered);

/* The operator.  Axes go x, then y, then z; the axis skip_axis (-1: none) is left alone -- blurImage(image, sigma, kernelWidth, dim),
 * the slice-wise mode.  One axis pass maps a float32 volume to a float32 volume:
 *   out[p] = f32( sum_{o = -r..+r} c[|o|] * (double) in[clamp(p + o e_axis)] ),
 * summed in double with o ascending from an accumulator of +0.0, every product and sum rounded on its own (no fused multiply-add),
 * coordinates clamped into [0, extent - 1] (ITK's zero-flux Neumann boundary), rounded to float32 once per pass; NaN and infinities
 * follow IEEE.  variance[a] (voxel units; spacing is the caller's business) is read for the blurred axes only; the kernel of an axis
 * is glia_hmt_gaussian_kernel(variance[a], max_width, GLIA_HMT_BLUR_MAX_ERROR).  Pixel types: GLIA_HMT_PIXEL_UINT8 / _UINT16 are converted to
 * float32 (exact), go through the same passes, and after the last one are clamped to the type's range and truncated toward zero
 * (ITK casts).  With no axis blurred the output equals the input.  dims as for glia_hmt_watershed; 1 to 2^32 - 2 voxels.
 *
 * glia_hmt_blur_image_host is the definition as plain C++ on host memory: no ctx, no GPU.  glia_hmt_blur_image works on device memory;
 * d_out must not be d_in.  Option GLIA_HMT_BLUR = passes | march: two routes to the same bytes --
 *   passes  one launch per blurred axis through float32 scratch volumes from the context's block cache (one volume per pass but the
 *           last); any radius;
 *   march   a workgroup owns a tile of tile_x x tile_y voxels plus its halo and walks along z: per input plane the x pass and the y
 *           pass run in LDS, the x-y blurred planes are kept in a ring of 2 r + 1 planes in LDS, the z-blurred plane is written; every
 *           voxel is read once apart from the halo and written once, no scratch.  Radii up to max_march_radius (64 KiB of static LDS);
 *           a larger radius on any blurred axis takes `passes`, and glia_hmt_last_blur_timing says so.
 * GLIA_HMT_ERR_ARG, message "blur_image: ...", before any HIP call for: a NULL ctx (device call), dims, variance, input or output; dim
 * other than 2 or 3; a non-positive extent or a size outside the range; an unknown pixel type; skip_axis outside -1..dim - 1; a
 * variance of a blurred axis that is not finite, <= 0 or above GLIA_HMT_BLUR_MAX_VARIANCE; max_width outside 1..GLIA_HMT_BLUR_MAX_WIDTH;
 * d_out == d_in; an unknown value of GLIA_HMT_BLUR (device call). */
enum { GLIA_HMT_PIXEL_FLOAT32 = 0, GLIA_HMT_PIXEL_UINT8 = 1, GLIA_HMT_PIXEL_UINT16 = 2 };
enum { GLIA_HMT_BLUR_ROUTE_PASSES = 0, GLIA_HMT_BLUR_ROUTE_MARCH = 1 };
int glia_hmt_blur_image_host(int dim, const int64_t dims[3], int pixel_type, const void* h_in, const double variance[3], int max_width,
                             int skip_axis, void* h_out);
int glia_hmt_blur_image(glia_hmt_ctx* ctx, int dim, const int64_t dims[3], int pixel_type, const void* d_in, const double variance[3],
                        int max_width, int skip_axis, void* d_out);
/* what the kernels really use (host-only; any pointer may be NULL): the march tile, the largest radius the march route takes, the
 * largest radius at all (= GLIA_HMT_BLUR_MAX_WIDTH) */
int glia_hmt_blur_limits(int* tile_x, int* tile_y, int* max_march_radius, int* max_radius);
/* the last glia_hmt_blur_image call on this context: device time of its kernels and the route that ran (GLIA_HMT_BLUR_ROUTE_*) */
int glia_hmt_last_blur_timing(const glia_hmt_ctx* ctx, double* ms, int* route_used);

/* ---- synthetic inputs for tests / bench, generated on the device -------------- */
int glia_hmt_synth(glia_hmt_ctx* ctx, int dim, const int64_t dims[3], int S, int G, uint64_t seed,
                   int variant, uint32_t* d_labels, float* d_pb);

#ifdef __cplusplus
}
#endif
#endif
