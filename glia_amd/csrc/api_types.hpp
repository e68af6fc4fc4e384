// glia_amd/csrc/api_types.hpp -- the opaque handles of include/glia_hmt.h as the library sees them (api.cpp, api_rag.cpp, api_loops.cpp,
// slab_dist.cpp), and the few host functions those files share.
#pragma once
#include "forest.hpp"
#include "forest_model.hpp"
#include "glibc_math.hpp"
#include "greedy_common.hpp"
#include "hmt_internal.hpp"
#include "mlp.hpp"

using namespace glia;

struct glia_hmt_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  // accumulation hash tables (kept clean between builds: compaction clears what it consumes)
  uint32_t rcap = 0, pcap = 0;
  uint32_t* rkeys = nullptr; uint32_t* rrec = nullptr;
  unsigned long long* pkeys = nullptr; uint32_t* prec = nullptr;
  uint32_t* flags = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  uint32_t hint_rcap = 0, hint_pcap = 0;
  double transform_ms = 0;
  glia_hmt_eval_timing evt = {0, 0, 0};   // the last glia_hmt_label_overlap / glia_hmt_eval call
  glia_hmt_forest_train_timing trt = {};  // the last glia_hmt_forest_train call
  glia_hmt_forest_oob_timing obt = {};    // its out-of-bag passes (glia_hmt_forest_train_oob)
  glia_hmt_mlp_train_timing mlt = {};     // the last glia_hmt_mlp_train call
  glia_hmt_sshmt_train_timing sst = {};   // the last glia_hmt_sshmt_train call
  glia_hmt_batch_timing bat = {};         // the last glia_hmt_*_train_batches call
  double blur_ms = 0; int blur_route = 0; // the last glia_hmt_blur_image call: device time, GLIA_HMT_BLUR_ROUTE_* that ran
  int tz = kTZ;                  // tile depth of the accumulation pass; halved when the LDS tables of a pass overflowed a lot
  LibmSel libm = {kLibmDevice, kLibmDevice, kLibmDevice, kLibmDevice};   // restatement of the host's log2 / log / pow / exp the kernels use (glibc_math.hpp)
};

struct glia_hmt_rag {
  glia_hmt_ctx* ctx = nullptr;
  int dim = 3;
  int64_t dims[3] = {1, 1, 1};
  bool only_contour = false;
  int bins = 0, nthr = 0;
  RagArrays arr;
  double pass_ms = 0, alg_bytes = 0;
  double ms_table = 0, ms_init = 0, ms_loop = 0;
  glia_hmt_bc_label_timing bcl;   // the last glia_hmt_bc_label call
  glia_hmt_bc_feat_timing bft = {0, 0, 0, 0, 0, 0, 0};   // the last bc_feat call, either route
  int64_t n_scored = 0;
  glia_hmt_feat_config cfg;
  bool has_cfg = false;
  VolumeRef vol;                 // whole-volume builds only: the caller keeps the volumes alive while the handle lives
  VolumeRef slab;                // slab builds: the planes handed in and the owned range (valid while the caller keeps them)
  uint32_t* d_folded = nullptr;  // labels with the mask folded in (owned)
  int map_region[GLIA_HMT_MAX_IMAGES] = {0}, map_rlabel[GLIA_HMT_MAX_IMAGES] = {0}, map_boundary[GLIA_HMT_MAX_IMAGES] = {0};   // list entry -> channel
};
// a handle like this one, owning nothing yet: no arrays, no folded labels, no volume or planes to re-read
inline glia_hmt_rag* rag_like(const glia_hmt_rag* like) {
  glia_hmt_rag* rag = new glia_hmt_rag(*like);
  rag->arr = RagArrays(); rag->d_folded = nullptr; rag->vol = VolumeRef(); rag->slab = VolumeRef();
  return rag;
}

struct glia_hmt_forest {
  int device = 0;
  glia::DeviceClassifier dc;
  OwnedArrays allocs;            // the packed trees of every model
  int max_var = 0;
};

struct glia_hmt_mlp {
  int device = -1;               // -1: a host-only handle (created without a context)
  glia::HostMlp host;
  glia::DeviceMlp dm;
  OwnedArrays allocs;
};

struct glia_hmt_forest_model {
  glia::ForestModel m;
};

int free_tables(glia_hmt_ctx* c);          // api_rag.cpp: the accumulation tables of a context
namespace glia { float ceil_f32(double d); uint32_t next_pow2(uint64_t v); HistSpec make_hist_spec(int bins, double lo, double hi); }   // api.cpp
