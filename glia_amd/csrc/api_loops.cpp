// glia_amd/csrc/api_loops.cpp -- C ABI: the entry points that run a merge loop or consume a merge order (merge orders, initial
// scores, bc_feat, bc_label), and the classifier they score with (forest load and predict).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <unordered_map>

#include "bc_features.hpp"
#include "dense_order.hpp"
#include "api_types.hpp"
#include "forest_train.hpp"
#include "median_layout.hpp"

namespace glia {
int greedy_bc(const RagArrays& rag, const BcCfg& cfg, const DeviceClassifier& clf, hipStream_t stream, const BcRequest& req, MergeResult* out) {
  auto* fn = &greedy_bc_generic;
  const bool common = cfg.K == 1 && cfg.n_region == 1 && cfg.n_rlabel == 0 && cfg.n_boundary == 1 && !cfg.use_hist && !cfg.use_log &&
                      !cfg.use_simple && !option("GLIA_HMT_BC_NOCOMMON");
  if (cfg.libm_log2 == kLibmSse2 && cfg.libm_log == kLibmFma && cfg.libm_pow == kLibmFma) fn = common ? &greedy_bc_fma_common : &greedy_bc_fma;
  else if (cfg.libm_log2 == kLibmSse2 && cfg.libm_log == kLibmSse2 && cfg.libm_pow == kLibmSse2) fn = common ? &greedy_bc_sse2_common : &greedy_bc_sse2;
  if (option("GLIA_HMT_BC_GENERIC")) fn = &greedy_bc_generic;       // tests: the run-time-dispatch instance
  if (clf.kind == 2) fn = &greedy_bc_mlp;                           // the one instance that holds the MLP scorer
  const int rc = greedy_bc_run(fn(), rag, cfg, clf, stream, req, out);
  return req.init_only ? rc : finish_merge_order(rc, out->order.data(), out->n, (uint32_t)rag.R, stream);
}
}  // namespace glia

extern "C" {

// A loop's order in keys, for the caller.  Dense id -> key: leaves = i-th label ascending; merged regions = maxKey + 1 + k
// (util/struct_merge.hxx:19,27-31), maxKey over the regions the reference's map holds: every label, or with contour_keys
// (merge_order_pb in contour-only mode, type/region_map.hxx:99-111) every label that owns a directed boundary.
static int order_to_keys(const glia_hmt_rag* rag, const MergeResult& res, const char* who, bool contour_keys, int64_t capacity,
                         uint32_t* h_order, double* h_sal, int64_t* n_merges) {
  const int64_t R = rag->arr.R, n = res.n;
  if (n > capacity) { set_error(std::string(who) + ": output capacity too small"); return GLIA_HMT_ERR_CAPACITY; }
  std::vector<uint32_t> lab((size_t)R);
  GLIA_HIP_TRY(hipMemcpy(lab.data(), rag->arr.d_rlabel, sizeof(uint32_t) * R, hipMemcpyDeviceToHost));
  uint32_t maxKey = lab[R - 1];
  if (contour_keys) GLIA_HIP_TRY(hipMemcpy(&maxKey, rag->arr.d_pa + (rag->arr.P - 1), sizeof(uint32_t), hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < 3 * n; ++i) {
    const uint32_t id = res.order[i];
    h_order[i] = id < (uint32_t)R ? lab[id] : maxKey + 1u + (id - (uint32_t)R);
  }
  std::copy(res.sal.begin(), res.sal.begin() + n, h_sal);
  *n_merges = n;
  return GLIA_HMT_OK;
}

static void keep_timing(glia_hmt_rag* rag, const MergeResult& res) {
  rag->ms_table = res.ms_table; rag->ms_init = res.ms_init; rag->ms_loop = res.ms_loop; rag->n_scored = res.n_scored;
}
// the pb-mean, median and pre_merge loops: run, keep the times, hand the order out in keys
static int pb_loop(glia_hmt_ctx* c, glia_hmt_rag* rag, const PbRequest& req, const char* who, bool contour_keys, int64_t capacity, uint32_t* h_order,
                   double* h_sal, int64_t* n_merges) {
  GLIA_HIP_TRY(hipSetDevice(c->device));
  *n_merges = 0;
  if (rag->arr.R == 0 || rag->arr.P == 0) return GLIA_HMT_OK;
  MergeResult res;
  if (int rc = greedy_mean(rag->arr, c->stream, req, &res)) return rc;
  keep_timing(rag, res);
  return order_to_keys(rag, res, who, contour_keys, capacity, h_order, h_sal, n_merges);
}

int glia_hmt_merge_order_pb(glia_hmt_ctx* c, glia_hmt_rag* rag, int type, uint32_t* h_order, double* h_sal,
                            int64_t capacity, int64_t* n_merges) {
  if (!c || !rag || !h_order || !h_sal || !n_merges || rag->ctx != c) {
    set_error("merge_order_pb: invalid argument");
    return GLIA_HMT_ERR_ARG;
  }
  if (type == 3 && rag->only_contour) {
    set_error("merge_order_pb: the median x min-size linkage needs region sizes (only_contour = 0)");
    return GLIA_HMT_ERR_ARG;
  }
  if ((type == 1 || type == 3) && !rag->vol.lab && !rag->arr.d_pv_off) {
    set_error("merge_order_pb: median linkage needs the volumes the RAG was built from (whole-volume build) or a map that carries its "
              "boundary values (glia_hmt_rag_build_distributed with with_values)");
    return GLIA_HMT_ERR_UNSUPPORTED;
  }
  if (type != 1 && type != 2 && type != 3) {   // hmt/main_merge_order_pb.cxx:36 (3: this library's name for ...AndMinSize)
    set_error("Error: unsupported boundary stats type...");
    return GLIA_HMT_ERR_ARG;
  }
  PbRequest req;
  if (type == 1 || type == 3) req.median_of = &rag->vol;
  req.size_weight = type == 3;
  return pb_loop(c, rag, req, "merge_order_pb", rag->only_contour, capacity, h_order, h_sal, n_merges);
}

static int upload_forest(const HostForest& hf, glia_hmt_forest* f, int slot, hipStream_t stream) {
  std::vector<PackedNode> nodes;
  std::vector<int> roots;
  int rc = pack_forest(hf, &nodes, &roots);
  if (rc) return rc;
  PackedNode* d_nodes = nullptr;
  int* d_roots = nullptr;
  if ((rc = f->allocs.alloc(&d_nodes, nodes.size())) || (rc = f->allocs.alloc(&d_roots, roots.size()))) return rc;
  GLIA_HIP_TRY(hipMemcpyAsync(d_nodes, nodes.data(), sizeof(PackedNode) * nodes.size(), hipMemcpyHostToDevice, stream));
  GLIA_HIP_TRY(hipMemcpyAsync(d_roots, roots.data(), sizeof(int) * roots.size(), hipMemcpyHostToDevice, stream));
  std::vector<PackedTriple> lines;
  std::vector<int> proots;
  rc = pack_forest_triples(hf, &lines, &proots);
  if (rc) return rc;
  PackedTriple* d_lines = nullptr;
  int* d_proots = nullptr;
  if ((rc = f->allocs.alloc(&d_lines, lines.size())) || (rc = f->allocs.alloc(&d_proots, proots.size()))) return rc;
  GLIA_HIP_TRY(hipMemcpyAsync(d_lines, lines.data(), sizeof(PackedTriple) * lines.size(), hipMemcpyHostToDevice, stream));
  GLIA_HIP_TRY(hipMemcpyAsync(d_proots, proots.data(), sizeof(int) * proots.size(), hipMemcpyHostToDevice, stream));
  GLIA_HIP_TRY(hipStreamSynchronize(stream));
  f->dc.f[slot].ntree = hf.ntree; f->dc.f[slot].nrnodes = hf.nrnodes; f->dc.f[slot].nnodes = (int)nodes.size();
  f->dc.f[slot].nodes = d_nodes; f->dc.f[slot].root = d_roots;
  f->dc.f[slot].triples = d_lines; f->dc.f[slot].troot = d_proots;
  if (hf.max_var > f->max_var) f->max_var = hf.max_var;
  return GLIA_HMT_OK;
}

int glia_hmt_forest_load(glia_hmt_ctx* c, int n_models, const char* const* paths, int predict_label,
                         const double* dist, glia_hmt_forest** out) {
  if (!c || !paths || !out || (n_models != 1 && n_models != 3)) {
    set_error("forest_load: one model, or three models with distributor arguments, expected");
    return GLIA_HMT_ERR_ARG;
  }
  if (n_models == 3 && !dist) { set_error("Error: model distributor needs 3 arguments..."); return GLIA_HMT_ERR_ARG; }
  GLIA_HIP_TRY(hipSetDevice(c->device));
  glia_hmt_forest* f = new glia_hmt_forest;
  f->device = c->device;
  memset(&f->dc, 0, sizeof(f->dc));
  f->dc.kind = 0; f->dc.n_models = n_models;
  if (dist) {
    f->dc.dim0 = (int)dist[0]; f->dc.dim1 = (int)dist[1]; f->dc.threshold = dist[2];
    if (f->dc.dim0 < 0 || f->dc.dim1 < 0) { delete f; set_error("forest_load: negative distributor dimension"); return GLIA_HMT_ERR_ARG; }
    f->max_var = std::max(f->dc.dim0, f->dc.dim1);
  }
  for (int i = 0; i < n_models; ++i) {
    HostForest hf;
    int rc = load_forest_file(paths[i], predict_label, &hf);
    if (rc == GLIA_HMT_OK) rc = upload_forest(hf, f, i, c->stream);
    if (rc) { glia_hmt_forest_free(f); return rc; }
  }
  *out = f;
  return GLIA_HMT_OK;
}

int glia_hmt_forest_file_parse(const char* path, int predict_label, int* ntree, int* nrnodes, int* nclass,
                               double* h_split, int* h_meta, int64_t capacity_nodes) {
  if (!path || !ntree || !nrnodes || !nclass) { set_error("forest_file_parse: invalid argument"); return GLIA_HMT_ERR_ARG; }
  HostForest hf;
  int rc = load_forest_file(path, predict_label, &hf);
  if (rc) return rc;
  *ntree = hf.ntree; *nrnodes = hf.nrnodes; *nclass = hf.nclass;
  const int64_t nodes = (int64_t)hf.ntree * hf.nrnodes;
  if (h_split || h_meta) {
    if (nodes > capacity_nodes) { set_error("forest_file_parse: capacity too small"); return GLIA_HMT_ERR_CAPACITY; }
    if (h_split) memcpy(h_split, hf.split.data(), sizeof(double) * nodes);
    if (h_meta) memcpy(h_meta, hf.meta.data(), sizeof(int) * 4 * nodes);
  }
  return GLIA_HMT_OK;
}

int glia_hmt_forest_stub(glia_hmt_ctx* c, int feature_index, glia_hmt_forest** out) {
  if (!c || !out || feature_index < 0) { set_error("forest_stub: invalid argument"); return GLIA_HMT_ERR_ARG; }
  glia_hmt_forest* f = new glia_hmt_forest;
  f->device = c->device;
  memset(&f->dc, 0, sizeof(f->dc));
  f->dc.kind = 1; f->dc.n_models = 1; f->dc.stub_index = feature_index; f->max_var = feature_index;
  *out = f;
  return GLIA_HMT_OK;
}

void glia_hmt_forest_free(glia_hmt_forest* f) {
  if (!f) return;
  (void)hipSetDevice(f->device);
  delete f;                               // (its arrays go with it)
}

// ---- training (forest_train.hip) ----
void glia_hmt_train_opts_default(glia_hmt_train_opts* o) {
  if (!o) return;
  const TrainOptions d;
  o->ntree = d.ntree; o->mtry = d.mtry; o->sample_ratio = d.sample_ratio; o->nodesize = d.nodesize; o->balance = d.balance;
  o->max_depth = d.max_depth; o->seed = d.seed;
}

void glia_hmt_oob_opts_default(glia_hmt_oob_opts* o) {
  if (!o) return;
  o->oob = 0; o->importance = 0;
}

int glia_hmt_forest_train(glia_hmt_ctx* c, const double* h_rows, int64_t n_rows, int dim, const int32_t* h_labels, const glia_hmt_train_opts* opts,
                          glia_hmt_forest_model** out) {
  return glia_hmt_forest_train_oob(c, h_rows, n_rows, dim, h_labels, opts, nullptr, out);
}

int glia_hmt_forest_train_oob(glia_hmt_ctx* c, const double* h_rows, int64_t n_rows, int dim, const int32_t* h_labels, const glia_hmt_train_opts* opts,
                              const glia_hmt_oob_opts* oob_opts, glia_hmt_forest_model** out) {
  if (!c || !out) { set_error("forest_train: NULL context or output"); return GLIA_HMT_ERR_ARG; }
  if ((n_rows > 0 && dim > 0 && !h_rows) || (n_rows > 0 && !h_labels)) { set_error("forest_train: NULL rows or labels"); return GLIA_HMT_ERR_ARG; }
  TrainOptions o;
  if (opts) {
    o.ntree = opts->ntree; o.mtry = opts->mtry; o.sample_ratio = opts->sample_ratio; o.nodesize = opts->nodesize; o.balance = opts->balance;
    o.max_depth = opts->max_depth; o.seed = opts->seed;
  }
  TrainPlan plan;
  const std::string bad = train_plan(h_rows, n_rows, dim, h_labels, o, &plan);
  if (!bad.empty()) { set_error(bad); return GLIA_HMT_ERR_ARG; }
  GLIA_HIP_TRY(hipSetDevice(c->device));
  glia_hmt_forest_model* m = new glia_hmt_forest_model;
  OobOptions oo;
  if (oob_opts) { oo.oob = oob_opts->oob ? 1 : 0; oo.importance = oob_opts->importance ? 1 : 0; }
  const int rc = forest_train_device(h_rows, n_rows, dim, plan, o, c->stream, &m->m, &c->trt, &oo, &c->obt);
  if (rc) { delete m; return rc; }
  *out = m;
  return GLIA_HMT_OK;
}

int glia_hmt_forest_model_from_arrays(int ntree, int nrnodes, int nclass, int mtry, const double* xbestsplit, const int* treemap,
                                      const int* nodestatus, const int* nodeclass, const int* bestvar, const int* ndbigtree, const double* classwt,
                                      const double* cutoff, const int* orig_labels, const int* new_labels, glia_hmt_forest_model** out) {
  if (ntree < 1 || nrnodes < 1 || nclass < 1 || !xbestsplit || !treemap || !nodestatus || !nodeclass || !bestvar || !ndbigtree || !classwt ||
      !cutoff || !orig_labels || !new_labels || !out) {
    set_error("forest_model_from_arrays: invalid argument");
    return GLIA_HMT_ERR_ARG;
  }
  const size_t nn = (size_t)ntree * (size_t)nrnodes;
  glia_hmt_forest_model* m = new glia_hmt_forest_model;
  ForestModel& f = m->m;
  f.ntree = ntree; f.nrnodes = nrnodes; f.nclass = nclass; f.mtry = mtry;
  f.xbestsplit.assign(xbestsplit, xbestsplit + nn); f.treemap.assign(treemap, treemap + 2 * nn);
  f.nodestatus.assign(nodestatus, nodestatus + nn); f.nodeclass.assign(nodeclass, nodeclass + nn); f.bestvar.assign(bestvar, bestvar + nn);
  f.ndbigtree.assign(ndbigtree, ndbigtree + ntree); f.classwt.assign(classwt, classwt + nclass); f.cutoff.assign(cutoff, cutoff + nclass);
  f.orig_labels.assign(orig_labels, orig_labels + nclass); f.new_labels.assign(new_labels, new_labels + nclass);
  *out = m;
  return GLIA_HMT_OK;
}

int glia_hmt_forest_model_sizes(const glia_hmt_forest_model* m, int* ntree, int* nrnodes, int* nclass, int* mtry) {
  if (!m) { set_error("forest_model_sizes: NULL model"); return GLIA_HMT_ERR_ARG; }
  if (ntree) *ntree = m->m.ntree;
  if (nrnodes) *nrnodes = m->m.nrnodes;
  if (nclass) *nclass = m->m.nclass;
  if (mtry) *mtry = m->m.mtry;
  return GLIA_HMT_OK;
}

int glia_hmt_forest_model_arrays(const glia_hmt_forest_model* m, double* xbestsplit, int* treemap, int* nodestatus, int* nodeclass, int* bestvar,
                                 int* ndbigtree, double* classwt, double* cutoff, int* orig_labels, int* new_labels) {
  if (!m) { set_error("forest_model_arrays: NULL model"); return GLIA_HMT_ERR_ARG; }
  const ForestModel& f = m->m;
  auto put = [](auto* dst, const auto& v) { if (dst && !v.empty()) memcpy(dst, v.data(), sizeof(v[0]) * v.size()); };
  put(xbestsplit, f.xbestsplit); put(treemap, f.treemap); put(nodestatus, f.nodestatus); put(nodeclass, f.nodeclass); put(bestvar, f.bestvar);
  put(ndbigtree, f.ndbigtree); put(classwt, f.classwt); put(cutoff, f.cutoff); put(orig_labels, f.orig_labels); put(new_labels, f.new_labels);
  return GLIA_HMT_OK;
}

int glia_hmt_forest_model_oob_sizes(const glia_hmt_forest_model* m, int64_t* n_rows, int* dim, int* has_oob, int* has_importance) {
  if (!m) { set_error("forest_model_oob_sizes: NULL model"); return GLIA_HMT_ERR_ARG; }
  if (!m->m.has_oob() && !m->m.has_importance()) { set_error("forest_model_oob_sizes: the model holds no out-of-bag arrays"); return GLIA_HMT_ERR_ARG; }
  if (n_rows) *n_rows = m->m.oob_rows;
  if (dim) *dim = m->m.oob_dim;
  if (has_oob) *has_oob = m->m.has_oob() ? 1 : 0;
  if (has_importance) *has_importance = m->m.has_importance() ? 1 : 0;
  return GLIA_HMT_OK;
}

int glia_hmt_forest_model_oob_arrays(const glia_hmt_forest_model* m, int* outcl, int* counttr, int* votes, int* oob_times, double* errtr,
                                     int64_t* err_wrong, int64_t* err_seen, double* importance, double* importanceSD) {
  if (!m) { set_error("forest_model_oob_arrays: NULL model"); return GLIA_HMT_ERR_ARG; }
  const ForestModel& f = m->m;
  if (!f.has_oob() && !f.has_importance()) { set_error("forest_model_oob_arrays: the model holds no out-of-bag arrays"); return GLIA_HMT_ERR_ARG; }
  auto put = [](auto* dst, const auto& v) { if (dst && !v.empty()) memcpy(dst, v.data(), sizeof(v[0]) * v.size()); };
  static_assert(sizeof(long long) == sizeof(int64_t), "err_wrong / err_seen are copied as they are");
  put(outcl, f.outcl); put(counttr, f.counttr); put(votes, f.votes); put(oob_times, f.oob_times); put(errtr, f.errtr);
  put(err_wrong, f.err_wrong); put(err_seen, f.err_seen); put(importance, f.importance); put(importanceSD, f.importanceSD);
  return GLIA_HMT_OK;
}

int glia_hmt_forest_model_set_oob(glia_hmt_forest_model* m, int64_t n_rows, int dim, const int* outcl, const int* counttr, const int* votes,
                                  const int* oob_times, const double* errtr, const double* importance, const double* importanceSD) {
  if (!m || n_rows < 1 || n_rows >= (1ll << 28) || dim < 1 || (!outcl && !importance) || (outcl && (!counttr || !votes || !oob_times || !errtr)) ||
      (importance && !importanceSD)) {
    set_error("forest_model_set_oob: invalid argument");
    return GLIA_HMT_ERR_ARG;
  }
  ForestModel& f = m->m;
  const size_t N = (size_t)n_rows, nc = (size_t)f.nclass, D = (size_t)dim;
  f.oob_rows = n_rows; f.oob_dim = dim;
  f.outcl.clear(); f.counttr.clear(); f.votes.clear(); f.oob_times.clear(); f.errtr.clear(); f.err_wrong.clear(); f.err_seen.clear();
  f.importance.clear(); f.importanceSD.clear();
  if (outcl) {
    f.outcl.assign(outcl, outcl + N); f.counttr.assign(counttr, counttr + nc * N); f.votes.assign(votes, votes + nc * N);
    f.oob_times.assign(oob_times, oob_times + N); f.errtr.assign(errtr, errtr + (size_t)f.ntree * (nc + 1));
  }
  if (importance) { f.importance.assign(importance, importance + D * (nc + 2)); f.importanceSD.assign(importanceSD, importanceSD + D * (nc + 1)); }
  return GLIA_HMT_OK;
}

int glia_hmt_forest_model_write(const glia_hmt_forest_model* m, const char* path) {
  if (!m || !path) { set_error("forest_model_write: NULL argument"); return GLIA_HMT_ERR_ARG; }
  const std::string bad = write_forest_model(m->m, path);
  if (!bad.empty()) { set_error(bad); return GLIA_HMT_ERR_IO; }
  return GLIA_HMT_OK;
}

void glia_hmt_forest_model_free(glia_hmt_forest_model* m) { delete m; }

int glia_hmt_forest_from_model(glia_hmt_ctx* c, const glia_hmt_forest_model* m, int predict_label, glia_hmt_forest** out) {
  if (!c || !m || !out) { set_error("forest_from_model: NULL argument"); return GLIA_HMT_ERR_ARG; }
  HostForest hf;
  int rc = model_to_host_forest(m->m, predict_label, &hf);
  if (rc) return rc;
  GLIA_HIP_TRY(hipSetDevice(c->device));
  glia_hmt_forest* f = new glia_hmt_forest;
  f->device = c->device;
  memset(&f->dc, 0, sizeof(f->dc));
  f->dc.kind = 0; f->dc.n_models = 1;
  if ((rc = upload_forest(hf, f, 0, c->stream))) { glia_hmt_forest_free(f); return rc; }
  *out = f;
  return GLIA_HMT_OK;
}

int glia_hmt_last_forest_train_timing(const glia_hmt_ctx* c, glia_hmt_forest_train_timing* out) {
  if (!c || !out) { set_error("last_forest_train_timing: NULL argument"); return GLIA_HMT_ERR_ARG; }
  *out = c->trt;
  return GLIA_HMT_OK;
}

int glia_hmt_last_forest_oob_timing(const glia_hmt_ctx* c, glia_hmt_forest_oob_timing* out) {
  if (!c || !out) { set_error("last_forest_oob_timing: NULL argument"); return GLIA_HMT_ERR_ARG; }
  *out = c->obt;
  return GLIA_HMT_OK;
}

// ---- batch prediction (forest_predict.hip) ----
static int check_predict_args(const char* who, const glia_hmt_ctx* c, const glia_hmt_forest* f, const void* rows, int64_t n_rows, int dim,
                              int64_t row_stride, const void* pred) {
  if (!c || !f) { set_error(std::string(who) + ": NULL context or forest"); return GLIA_HMT_ERR_ARG; }
  if (n_rows < 0 || dim < 1 || row_stride < dim || (n_rows > 0 && (!rows || !pred))) { set_error(std::string(who) + ": invalid argument"); return GLIA_HMT_ERR_ARG; }
  if (dim <= f->max_var) {
    set_error(std::string(who) + ": rows of " + std::to_string(dim) + " columns, but the classifier reads column " + std::to_string(f->max_var));
    return GLIA_HMT_ERR_ARG;
  }
  return GLIA_HMT_OK;
}

int glia_hmt_forest_predict_tile_rows(int64_t n_rows, int dim) {
  if (n_rows < 0 || dim < 1) { set_error("forest_predict_tile_rows: invalid argument"); return GLIA_HMT_ERR_ARG; }
  return forest_predict_tile_rows(n_rows, dim);
}

int glia_hmt_forest_predict_device(glia_hmt_ctx* c, const glia_hmt_forest* f, const double* d_rows, int64_t n_rows, int dim, int64_t row_stride,
                                   double* d_pred) {
  const int rc = check_predict_args("forest_predict_device", c, f, d_rows, n_rows, dim, row_stride, d_pred);
  if (rc || n_rows == 0) return rc;
  GLIA_HIP_TRY(hipSetDevice(c->device));
  return launch_forest_predict(f->dc, d_rows, n_rows, dim, row_stride, d_pred, c->stream);
}

int glia_hmt_forest_predict(glia_hmt_ctx* c, const glia_hmt_forest* f, const double* h_rows, int64_t n_rows, int dim, double* h_pred) {
  int rc = check_predict_args("forest_predict", c, f, h_rows, n_rows, dim, dim, h_pred);
  if (rc || n_rows == 0) return rc;
  GLIA_HIP_TRY(hipSetDevice(c->device));
  // rows stream through device buffers of at most 128 MiB (GLIA_HMT_MINCAP: 256 rows, so that tests cross chunk boundaries)
  const int64_t chunk = std::min<int64_t>(n_rows, option("GLIA_HMT_MINCAP") ? 256 : std::max<int64_t>(1, (int64_t)(1 << 24) / dim));
  OwnedArrays own;
  double *d_rows = nullptr, *d_pred = nullptr;
  if ((rc = own.alloc(&d_rows, (size_t)chunk * dim)) || (rc = own.alloc(&d_pred, (size_t)chunk))) return rc;
  hipError_t e = hipSuccess;
  for (int64_t r0 = 0; e == hipSuccess && rc == GLIA_HMT_OK && r0 < n_rows; r0 += chunk) {
    const int64_t n = std::min(chunk, n_rows - r0);
    e = hipMemcpyAsync(d_rows, h_rows + r0 * dim, sizeof(double) * (size_t)n * dim, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) rc = launch_forest_predict(f->dc, d_rows, n, dim, dim, d_pred, c->stream);
    if (e == hipSuccess && rc == GLIA_HMT_OK) e = hipMemcpyAsync(h_pred + r0, d_pred, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  }
  if (e != hipSuccess) { set_error(std::string("forest_predict: ") + hipGetErrorString(e)); return GLIA_HMT_ERR_HIP; }
  return rc;
}

static inline double sdivide_host(double l, double r) { return std::fabs(r) >= 2.22e-16 ? l / r : 0.0; }   // glia_base.hxx:77-78

static bool make_bc_cfg(const glia_hmt_rag* rag, BcCfg* c) {
  if (!rag->has_cfg) return false;
  const glia_hmt_feat_config& g = rag->cfg;
  memset(c, 0, sizeof(*c));
  c->D = rag->dim; c->T = g.n_thresholds; c->bins = rag->bins;
  c->K = rag->arr.K;
  for (int k = 0; k < kMaxChannels; ++k) c->cbins[k] = k < rag->arr.K ? rag->arr.c_bins[k] : 0;
  c->n_region = g.n_region; c->n_rlabel = g.n_rlabel; c->n_boundary = g.n_boundary;
  for (int i = 0; i < kMaxListed; ++i) { c->rc[i] = rag->map_region[i]; c->lc[i] = rag->map_rlabel[i]; c->bc[i] = rag->map_boundary[i]; }
  c->use_log = g.use_log_shape; c->use_simple = g.use_simple_features; c->use_hist = g.use_histogram_features;
  c->norm_area = g.normalizing_area; c->norm_len = g.normalizing_length;
  c->rfdim = bc_rf_dim(*c); c->bfdim = bc_bf_dim(*c); c->fdim = bc_feat_dim(*c);
  c->libm_log2 = rag->ctx->libm.log2_variant; c->libm_log = rag->ctx->libm.log_variant; c->libm_pow = rag->ctx->libm.pow_variant;
  return true;
}

// GLIA_USE_MEDIAN_AS_FEATS: the columns the layout adds (median_layout.hpp), 0 for a map built without it
static int median_extra_cols(const glia_hmt_rag* rag, const BcCfg& c) { return rag->cfg.use_median_features ? median_extra_cols(c) : 0; }
// the greedy loop keeps mergeable statistics, not value multisets: with this layout bc_feat (a given order) and the scores of the
// initial edges (both regions are leaves: median_init.hip) are implemented, the loop itself is not
static int refuse_median_in_loop(const glia_hmt_rag* rag, const char* who) {
  if (!rag->has_cfg || !rag->cfg.use_median_features) return GLIA_HMT_OK;
  set_error(std::string(who) + ": the GLIA_USE_MEDIAN_AS_FEATS layout (type/feat.hxx:677-722) is implemented for a given merge order only (glia_hmt_bc_feat): "
            "inside the greedy loop every contraction changes the value multisets of its regions and boundary sets");
  return GLIA_HMT_ERR_UNSUPPORTED;
}

int glia_hmt_feat_dim(const glia_hmt_rag* rag) {
  BcCfg c;
  if (!rag || !make_bc_cfg(rag, &c)) return -1;
  return c.fdim + median_extra_cols(rag, c);
}

// What the classifier entry points check before a run of the loop (`who` prefixes the messages).  forest == nullptr: a given
// order (bc_feat), where no classifier reads the vector.  The median layout is accepted where `median` is given -- bc_feat and the
// initial scores, which get the images and the volume of the map there -- and refused by the loop.
static int bc_setup(glia_hmt_ctx* c, const glia_hmt_rag* rag, const glia_hmt_forest* forest, const char* who, BcCfg* cfg, MedianFeatIn* median = nullptr) {
  if (!make_bc_cfg(rag, cfg) || rag->only_contour) {
    set_error(std::string(who) + ": the region map must be built with a feature configuration and with region points");
    return GLIA_HMT_ERR_ARG;
  }
  if (!median) { if (int rm = refuse_median_in_loop(rag, who)) return rm; }
  if (forest && forest->max_var >= cfg->fdim + median_extra_cols(rag, *cfg)) { set_error(std::string(who) + ": the classifier reads features beyond the vector"); return GLIA_HMT_ERR_ARG; }
  if (median && rag->cfg.use_median_features) {
    if (forest && !rag->vol.lab) { set_error(std::string(who) + " (median features): needs the volumes the region map was built from (whole-volume build)"); return GLIA_HMT_ERR_UNSUPPORTED; }
    const glia_hmt_feat_config& g = rag->cfg;
    memset(median, 0, sizeof(*median));
    median->rag = &rag->arr; median->vol = rag->vol;
    median->n_r = g.n_region; median->n_b = g.n_boundary;
    for (int i = 0; i < g.n_region; ++i) median->r_img[i] = (const float*)g.region[i].d_image;
    for (int i = 0; i < g.n_boundary; ++i) median->b_img[i] = (const float*)g.boundary[i].d_image;
  }
  GLIA_HIP_TRY(hipSetDevice(c->device));
  return GLIA_HMT_OK;
}

// the loop with any classifier (checked by the caller); `who` prefixes the messages
static int merge_order_bc_with(glia_hmt_ctx* c, glia_hmt_rag* rag, const BcCfg& cfg, const DeviceClassifier& clf, const char* who, uint32_t* h_order,
                               double* h_sal, double* h_feats, int64_t capacity, int64_t* n_merges, const DeviceMlp* mlp = nullptr) {
  int rc;
  *n_merges = 0;
  if (rag->arr.R == 0 || rag->arr.P == 0) return GLIA_HMT_OK;
  BcRequest req;
  req.rows = h_feats != nullptr;
  req.mlp = mlp; req.exp_variant = c->libm.exp_variant;
  MergeResult res;
  if ((rc = greedy_bc(rag->arr, cfg, clf, c->stream, req, &res))) return rc;
  keep_timing(rag, res);
  if ((rc = order_to_keys(rag, res, who, false, capacity, h_order, h_sal, n_merges))) return rc;
  if (h_feats) std::copy(res.rows.begin(), res.rows.end(), h_feats);
  return GLIA_HMT_OK;
}

int glia_hmt_merge_order_bc(glia_hmt_ctx* c, glia_hmt_rag* rag, const glia_hmt_forest* forest, uint32_t* h_order,
                            double* h_sal, double* h_feats, int64_t capacity, int64_t* n_merges) {
  if (!c || !rag || !forest || !h_order || !h_sal || !n_merges || rag->ctx != c) {
    set_error("merge_order_bc: invalid argument");
    return GLIA_HMT_ERR_ARG;
  }
  BcCfg cfg;
  if (int rc = bc_setup(c, rag, forest, "merge_order_bc", &cfg)) return rc;
  return merge_order_bc_with(c, rag, cfg, forest->dc, "merge_order_bc", h_order, h_sal, h_feats, capacity, n_merges);
}

// The MLP as the loop's classifier (hmt/main_merge_order_bc.cxx:111-139): what the loop cannot hold is refused here, before any
// HIP call.  The loop scores with the weights the handle already holds on the device.
static int mlp_classifier(glia_hmt_ctx* c, const glia_hmt_rag* rag, const glia_hmt_mlp* mlp, const char* who, BcCfg* cfg, DeviceClassifier* clf) {
  auto bad = [&](const std::string& what) { set_error(std::string(who) + ": " + what); return GLIA_HMT_ERR_ARG; };
  if (!make_bc_cfg(rag, cfg) || rag->only_contour) return bad("the region map must be built with a feature configuration and with region points");
  if (rag->cfg.use_median_features) { (void)refuse_median_in_loop(rag, who); return GLIA_HMT_ERR_ARG; }
  const HostMlp& h = mlp->host;
  if (h.n1 == 0) return bad("the logsig model (no hidden layer) is a batch predictor only (glia_hmt_mlp_predict), not a classifier of the loop");
  if (h.n1 > kMlpLoopMaxHidden || h.n2 > kMlpLoopMaxHidden)
    return bad("hidden layers of " + std::to_string(h.n1) + " and " + std::to_string(h.n2) + " units, but the loop takes at most " +
               std::to_string(kMlpLoopMaxHidden) + " units per hidden layer (glia_hmt_mlp_loop_limits)");
  if (h.D - 1 != cfg->fdim)
    return bad("the model is for rows of " + std::to_string(h.D - 1) + " columns, but the region map's feature vector has " + std::to_string(cfg->fdim));
  if (mlp->device != c->device) return bad("the model was not created on this context's device");
  memset(clf, 0, sizeof(*clf));
  clf->kind = 2; clf->n_models = h.n_models;      // (the weights go beside it: BcRequest::mlp)
  GLIA_HIP_TRY(hipSetDevice(c->device));
  return GLIA_HMT_OK;
}

int glia_hmt_merge_order_bc_mlp(glia_hmt_ctx* c, glia_hmt_rag* rag, const glia_hmt_mlp* mlp, uint32_t* h_order, double* h_sal, double* h_feats,
                                int64_t capacity, int64_t* n_merges) {
  if (!c || !rag || !mlp || !h_order || !h_sal || !n_merges || rag->ctx != c) {
    set_error("merge_order_bc_mlp: invalid argument");
    return GLIA_HMT_ERR_ARG;
  }
  BcCfg cfg;
  DeviceClassifier clf;
  if (int rc = mlp_classifier(c, rag, mlp, "merge_order_bc_mlp", &cfg, &clf)) return rc;
  return merge_order_bc_with(c, rag, cfg, clf, "merge_order_bc_mlp", h_order, h_sal, h_feats, capacity, n_merges, &mlp->dm);
}

int glia_hmt_pre_merge(glia_hmt_ctx* c, glia_hmt_rag* rag, const int* size_thresholds, int n_thresholds,
                       double rpb_threshold, uint32_t* h_order, double* h_sal, int64_t capacity, int64_t* n_merges) {
  if (!c || !rag || !size_thresholds || n_thresholds < 1 || n_thresholds > 2 || !h_order || !h_sal || !n_merges || rag->ctx != c) {
    set_error("pre_merge: invalid argument");
    return GLIA_HMT_ERR_ARG;
  }
  if (rag->only_contour) { set_error("pre_merge: the region map must hold region points (only_contour = 0)"); return GLIA_HMT_ERR_ARG; }
  PbRequest req;
  req.cond_n = n_thresholds;
  req.cond_sizes[0] = size_thresholds[0]; req.cond_sizes[1] = n_thresholds > 1 ? size_thresholds[1] : 0;
  req.cond_rpb = rpb_threshold;
  return pb_loop(c, rag, req, "pre_merge", false, capacity, h_order, h_sal, n_merges);
}

int glia_hmt_bc_feat(glia_hmt_ctx* c, glia_hmt_rag* rag, const uint32_t* h_order, int64_t n_merges, double* h_feats) {
  return glia_hmt_bc_feat_saliency(c, rag, h_order, n_merges, nullptr, 1.0, 1.0, h_feats);
}

int glia_hmt_bc_feat_dim(const glia_hmt_rag* rag, int with_saliency) {
  BcCfg cfg;
  if (!rag || !make_bc_cfg(rag, &cfg)) return -1;
  return cfg.fdim + median_extra_cols(rag, cfg) + ((with_saliency && !cfg.use_simple) ? 5 : 0);
}

// ---- a given merge order: what bc_feat and bc_label share ----
// keys -> dense ids: leaves by label, the region created by merge i is R + i (RegionMap(seg, mask, order, false),
// type/region_map.hxx:42-48,67-68); the order is validated on the way (dense_order.hpp), `who` prefixes the messages; *lab = the
// region labels, [R] ascending
static int dense_order_of(const glia_hmt_rag* rag, const char* who, const uint32_t* h_order, int64_t n_merges, std::vector<uint32_t>* lab,
                          std::vector<uint32_t>* forced) {
  const int64_t R = rag->arr.R;
  lab->resize((size_t)R);
  if (R) GLIA_HIP_TRY(hipMemcpy(lab->data(), rag->arr.d_rlabel, sizeof(uint32_t) * R, hipMemcpyDeviceToHost));
  const DenseOrderResult r = dense_order(lab->data(), R, h_order, n_merges, forced);
  if (r.error == kDenseOrderOk) return GLIA_HMT_OK;
  set_error(std::string(who) + (r.error == kDenseOrderTooMany ? ": more merges than regions" : r.error == kDenseOrderReusedKey ? ": merge order reuses a region key"
                                                                                             : ": merge order refers to an unknown or already merged region"));
  return GLIA_HMT_ERR_ARG;
}

// GLIA_USE_MEDIAN_AS_FEATS: the statistic rows (built from the statistics monoids) + the medians, means and standard deviations
// of the value multisets (median_feats.hip), spliced into the reference's layout (median_layout.hpp); *feats is replaced
static int bc_feat_median_rows(glia_hmt_ctx* c, const glia_hmt_rag* rag, const BcCfg& cfg, MedianFeatIn& in, const std::vector<uint32_t>& forced, int64_t n,
                               std::vector<double>* feats, int* bfdim, int* rfdim, int* fdim) {
  in.forced = forced.data(); in.n_merges = n;
  std::vector<double> reg, bnd;
  std::vector<unsigned long long> marea;
  if (int rc = median_feature_stats(in, c->stream, &reg, &bnd, &marea)) return rc;
  const int nr = in.n_r, nb = in.n_b;
  const int nd = cfg.fdim + median_extra_cols(rag, cfg);
  std::vector<double> rows((size_t)n * nd);
  for (int64_t i = 0; i < n; ++i) {
    const bool swap = sdivide_host((double)marea[forced[2 * i]], cfg.norm_area) > sdivide_host((double)marea[forced[2 * i + 1]], cfg.norm_area);
    // x1 = the smaller region (main_bc_feat.cxx:84-88): k of the statistics arrays for block b of the row
    const int kreg[3] = {swap ? 1 : 0, swap ? 0 : 1, 2};
    auto RS = [&](int blk, int img, int q) { return reg[(((size_t)i * 3 + kreg[blk]) * nr + img) * 3 + q]; };
    auto BS = [&](int blk, int img, int q) { return bnd[(((size_t)i * 4 + (blk < 3 ? kreg[blk] : 3)) * nb + img) * 3 + q]; };
    if (median_splice(cfg, &(*feats)[(size_t)i * cfg.fdim], &rows[(size_t)i * nd], RS, BS) != nd) { set_error("bc_feat: internal error, median feature layout"); return GLIA_HMT_ERR_INTERNAL; }
  }
  feats->swap(rows);
  *fdim = nd;
  if (!cfg.use_simple) { *bfdim = cfg.bfdim + in.n_r + in.n_b; *rfdim = cfg.rfdim + in.n_r + in.n_b; }
  return GLIA_HMT_OK;
}

// Saliency features (hmt/main_bc_feat.cxx:50-55): every region of the order carries a number -- initSal for the
// regions that are only merged, saliency + bias for the region a merge creates (genSaliencyMap, hmt/bc_feat.hxx:12-26).
// They do not depend on the image: each region block gets its number appended (bc_feat.hxx:76), the boundary block
// (min, max) of |s(x1) - s(x3)|, |s(x2) - s(x3)| (:163-166, :208-213).  Which region is x1 follows the area rule of
// main_bc_feat.cxx:88-91, for which the voxel counts of the tree nodes are summed up here.
static int bc_feat_saliency_rows(const glia_hmt_rag* rag, const BcCfg& cfg, const uint32_t* h_order, const std::vector<uint32_t>& forced, int64_t n_merges,
                                 const double* h_saliencies, double init_saliency, double saliency_bias, const std::vector<double>& feats, int bfdim,
                                 int rfdim, int fdim, double* h_feats) {
  const int64_t R = rag->arr.R;
  std::vector<uint32_t> rrec((size_t)R * kRegionWords);
  GLIA_HIP_TRY(hipMemcpy(rrec.data(), rag->arr.d_rrec, sizeof(uint32_t) * kRegionWords * R, hipMemcpyDeviceToHost));
  std::vector<unsigned long long> area((size_t)R + n_merges);
  for (int64_t i = 0; i < R; ++i) area[i] = rrec[(size_t)i * kRegionWords + R_CNT];
  std::unordered_map<uint32_t, double> smap;
  for (int64_t i = 0; i < n_merges; ++i) {
    if (!smap.count(h_order[3 * i])) smap[h_order[3 * i]] = init_saliency;
    if (!smap.count(h_order[3 * i + 1])) smap[h_order[3 * i + 1]] = init_saliency;
    smap[h_order[3 * i + 2]] = h_saliencies[i] + saliency_bias;
  }
  const int od = fdim + 5;
  for (int64_t i = 0; i < n_merges; ++i) {
    const uint32_t a = forced[2 * i], b = forced[2 * i + 1];
    area[R + i] = area[a] + area[b];
    const bool swap = sdivide_host((double)area[a], cfg.norm_area) > sdivide_host((double)area[b], cfg.norm_area);
    const double s0 = smap[h_order[3 * i]], s1 = smap[h_order[3 * i + 1]], s2 = smap[h_order[3 * i + 2]];
    const double sx1 = swap ? s1 : s0, sx2 = swap ? s0 : s1;
    const double d02 = std::fabs(sx1 - s2), d12 = std::fabs(sx2 - s2);
    const double* in = &feats[(size_t)i * fdim];
    double* out = &h_feats[(size_t)i * od];
    int k = 0;
    for (int q = 0; q < bfdim; ++q) out[k++] = in[q];
    out[k++] = std::min(d02, d12); out[k++] = std::max(d02, d12);
    for (int q = 0; q < rfdim; ++q) out[k++] = in[bfdim + q];
    out[k++] = sx1;
    for (int q = 0; q < rfdim; ++q) out[k++] = in[bfdim + rfdim + q];
    out[k++] = sx2;
    for (int q = 0; q < rfdim; ++q) out[k++] = in[bfdim + 2 * rfdim + q];
    out[k++] = s2;
  }
  return GLIA_HMT_OK;
}

// route: the replay through the classifier loop (greedy_bc.hip, one contraction at a time) or the batch formulation over the known
// tree (bc_feat_batch.hip); everything after the statistic rows is common
static int bc_feat_rows(glia_hmt_ctx* c, glia_hmt_rag* rag, const uint32_t* h_order, int64_t n_merges, const double* h_saliencies, double init_saliency,
                        double saliency_bias, double* h_feats, int route) {
  if (!c || !rag || !h_order || !h_feats || n_merges < 0 || rag->ctx != c) { set_error("bc_feat: invalid argument"); return GLIA_HMT_ERR_ARG; }
  BcCfg cfg;
  int rc;
  MedianFeatIn in;
  if ((rc = bc_setup(c, rag, nullptr, "bc_feat", &cfg, &in))) return rc;
  if (n_merges == 0) return GLIA_HMT_OK;
  std::vector<uint32_t> rlabel, forced;
  if ((rc = dense_order_of(rag, "bc_feat", h_order, n_merges, &rlabel, &forced))) return rc;
  MergeResult res;
  memset(&rag->bft, 0, sizeof(rag->bft));
  if (route == GLIA_HMT_BCFEAT_BATCH) {
    BcFeatBatchInfo info;
    if ((rc = bc_feat_batch_rows(rag->arr, cfg, forced.data(), n_merges, c->stream, &res.rows, &info))) return rc;
    res.n = n_merges;
    rag->bft = glia_hmt_bc_feat_timing{info.ms_plan, info.ms_sets, info.ms_rows, info.height, info.launches, info.path_updates, GLIA_HMT_BCFEAT_BATCH};
  } else {
    DeviceClassifier none;
    memset(&none, 0, sizeof(none));
    none.kind = 1;
    BcRequest req;
    req.forced = forced.data(); req.n_forced = n_merges; req.rows = true;
    if ((rc = greedy_bc(rag->arr, cfg, none, c->stream, req, &res))) return rc;
    keep_timing(rag, res);
    rag->bft = glia_hmt_bc_feat_timing{0.0, res.ms_table + res.ms_init, res.ms_loop, 0, 0, 0, GLIA_HMT_BCFEAT_REPLAY};
    if (res.n != n_merges) { set_error("bc_feat: merges not completed (internal error)"); count_internal_error(); return GLIA_HMT_ERR_INTERNAL; }
  }
  const int64_t n = res.n;
  std::vector<double>& feats = res.rows;
  int bfdim = cfg.bfdim, rfdim = cfg.rfdim, fdim = cfg.fdim;
  if (rag->cfg.use_median_features && (rc = bc_feat_median_rows(c, rag, cfg, in, forced, n, &feats, &bfdim, &rfdim, &fdim))) return rc;
  if (!h_saliencies || cfg.use_simple) {       // selectFeatures carries no saliency (hmt/bc_feat.hxx:247-279)
    memcpy(h_feats, feats.data(), sizeof(double) * (size_t)n * fdim);
    return GLIA_HMT_OK;
  }
  return bc_feat_saliency_rows(rag, cfg, h_order, forced, n_merges, h_saliencies, init_saliency, saliency_bias, feats, bfdim, rfdim, fdim, h_feats);
}

// GLIA_HMT_BCFEAT = replay (default) | batch, read per call: which route the two older entry points take
static int bc_feat_default_route(int* route) {
  std::string v;
  *route = GLIA_HMT_BCFEAT_REPLAY;
  if (!option("GLIA_HMT_BCFEAT", &v) || v == "replay") return GLIA_HMT_OK;
  if (v == "batch") { *route = GLIA_HMT_BCFEAT_BATCH; return GLIA_HMT_OK; }
  set_error("bc_feat: GLIA_HMT_BCFEAT must be replay or batch, not '" + v + "'");
  return GLIA_HMT_ERR_ARG;
}

int glia_hmt_bc_feat_saliency(glia_hmt_ctx* c, glia_hmt_rag* rag, const uint32_t* h_order, int64_t n_merges,
                              const double* h_saliencies, double init_saliency, double saliency_bias, double* h_feats) {
  int route;
  if (int rc = bc_feat_default_route(&route)) return rc;
  return bc_feat_rows(c, rag, h_order, n_merges, h_saliencies, init_saliency, saliency_bias, h_feats, route);
}

int glia_hmt_bc_feat_batch(glia_hmt_ctx* c, glia_hmt_rag* rag, const uint32_t* h_order, int64_t n_merges,
                           const double* h_saliencies, double init_saliency, double saliency_bias, double* h_feats) {
  return bc_feat_rows(c, rag, h_order, n_merges, h_saliencies, init_saliency, saliency_bias, h_feats, GLIA_HMT_BCFEAT_BATCH);
}

int glia_hmt_last_bc_feat_timing(const glia_hmt_rag* r, glia_hmt_bc_feat_timing* out) {
  if (!r || !out) { set_error("last_bc_feat_timing: NULL argument"); return GLIA_HMT_ERR_ARG; }
  *out = r->bft;
  return GLIA_HMT_OK;
}

int glia_hmt_boundary_confidence(glia_hmt_ctx* c, glia_hmt_rag* rag, int n_trees, const int64_t* n_nodes, const uint32_t* const* node_label,
                                 const int32_t* const* parent, const int32_t* const* child0, const double* const* potential, float* d_out) {
  if (!c || !rag || rag->ctx != c || n_trees < 1 || !n_nodes || !node_label || !parent || !child0 || !potential || !d_out) {
    set_error("boundary_confidence: invalid argument");
    return GLIA_HMT_ERR_ARG;
  }
  if (!rag->vol.lab) { set_error("boundary_confidence: needs the volumes the region map was built from (whole-volume build)"); return GLIA_HMT_ERR_UNSUPPORTED; }
  GLIA_HIP_TRY(hipSetDevice(c->device));
  const int64_t P = rag->arr.P;
  std::vector<uint32_t> pa((size_t)(P ? P : 1)), pb((size_t)(P ? P : 1));
  if (P) {
    GLIA_HIP_TRY(hipMemcpy(pa.data(), rag->arr.d_pa, sizeof(uint32_t) * P, hipMemcpyDeviceToHost));
    GLIA_HIP_TRY(hipMemcpy(pb.data(), rag->arr.d_pb, sizeof(uint32_t) * P, hipMemcpyDeviceToHost));
  }
  std::vector<float> val;
  int rc = boundary_confidence_values(n_trees, n_nodes, node_label, parent, child0, potential, pa.data(), pb.data(), P, &val);
  if (rc) return rc;
  return paint_pair_values(rag->vol, rag->arr.d_pa, rag->arr.d_pb, P, val.data(), d_out, c->stream);
}

int glia_hmt_score_initial_edges(glia_hmt_ctx* c, glia_hmt_rag* rag, const glia_hmt_forest* forest, int64_t* n_edges,
                                 double* ms) {
  if (!c || !rag || !forest || rag->ctx != c) { set_error("score_initial_edges: invalid argument"); return GLIA_HMT_ERR_ARG; }
  int64_t n_records;                     // the one shard that is everything, its scores not asked for
  if (int rc = glia_hmt_score_initial_edges_shard(c, rag, forest, 0, 1, nullptr, 0, &n_records)) return rc;
  if (n_edges) *n_edges = rag->n_scored;
  if (ms) *ms = rag->ms_init;
  return GLIA_HMT_OK;
}

// one record per unordered leaf pair; the count is needed before the scores can be copied out
static int score_initial_with(glia_hmt_ctx* c, glia_hmt_rag* rag, const BcCfg& cfg, const DeviceClassifier& clf, const MedianFeatIn* median, int shard,
                              int n_shards, double* h_scores, int64_t capacity, int64_t* n_records, const DeviceMlp* mlp = nullptr) {
  BcRequest req;
  req.mlp = mlp; req.exp_variant = c->libm.exp_variant;
  req.init_only = true; req.scores = h_scores != nullptr; req.shard = shard; req.n_shards = n_shards;
  req.median = median;
  MergeResult res;
  if (int rc = greedy_bc(rag->arr, cfg, clf, c->stream, req, &res)) return rc;
  keep_timing(rag, res);
  *n_records = res.n;
  if (h_scores) {
    if (res.n > capacity) { set_error("score_initial_edges_shard: output capacity too small"); return GLIA_HMT_ERR_CAPACITY; }
    std::copy(res.sal.begin(), res.sal.begin() + res.n, h_scores);
  }
  return GLIA_HMT_OK;
}

int glia_hmt_score_initial_edges_shard(glia_hmt_ctx* c, glia_hmt_rag* rag, const glia_hmt_forest* forest, int shard, int n_shards,
                                       double* h_scores, int64_t capacity, int64_t* n_records) {
  if (!c || !rag || !forest || rag->ctx != c || n_shards < 1 || shard < 0 || shard >= n_shards || !n_records) {
    set_error("score_initial_edges_shard: invalid argument");
    return GLIA_HMT_ERR_ARG;
  }
  BcCfg cfg;
  MedianFeatIn median;
  if (int rc = bc_setup(c, rag, forest, "score_initial_edges", &cfg, &median)) return rc;
  return score_initial_with(c, rag, cfg, forest->dc, rag->cfg.use_median_features ? &median : nullptr, shard, n_shards, h_scores, capacity, n_records);
}

int glia_hmt_score_initial_edges_shard_mlp(glia_hmt_ctx* c, glia_hmt_rag* rag, const glia_hmt_mlp* mlp, int shard, int n_shards, double* h_scores,
                                           int64_t capacity, int64_t* n_records) {
  if (!c || !rag || !mlp || rag->ctx != c || n_shards < 1 || shard < 0 || shard >= n_shards || !n_records) {
    set_error("score_initial_edges_shard_mlp: invalid argument");
    return GLIA_HMT_ERR_ARG;
  }
  BcCfg cfg;
  DeviceClassifier clf;
  if (int rc = mlp_classifier(c, rag, mlp, "score_initial_edges_shard_mlp", &cfg, &clf)) return rc;
  return score_initial_with(c, rag, cfg, clf, nullptr, shard, n_shards, h_scores, capacity, n_records, &mlp->dm);
}

// hmt/main_bc_label_ri.cxx:27-153 (F1 / RI, --optSplit, --opt) and hmt/main_bc_label_vi.cxx:27-128 (VI, majority over truths, --opt):
// the contingency table of labels and each truth volume on the device (label_overlap.hip), its labels -> leaves (dense_order.hpp),
// per-node values and the label rules (bc_label.cpp) on the host
int glia_hmt_bc_label(glia_hmt_ctx* c, glia_hmt_rag* rag, const uint32_t* const* d_truth, int n_truth, const uint32_t* h_order,
                      int64_t n_merges, const glia_hmt_bc_label_opts* opts, int32_t* h_labels) {
  glia_hmt_bc_label_opts o = {GLIA_HMT_BC_LABEL_F1, 0, 1.0, 0, 0};         // the tools' defaults (main_bc_label_ri.cxx:19-23)
  if (opts) o = *opts;
  if (!c || !rag || rag->ctx != c || !d_truth || n_truth < 1 || n_merges < 0 || (n_merges && (!h_order || !h_labels))) {
    set_error("bc_label: invalid argument");
    return GLIA_HMT_ERR_ARG;
  }
  for (int t = 0; t < n_truth; ++t) if (!d_truth[t]) { set_error("bc_label: null truth volume"); return GLIA_HMT_ERR_ARG; }
  if (o.metric < GLIA_HMT_BC_LABEL_F1 || o.metric > GLIA_HMT_BC_LABEL_VI) { set_error("bc_label: unknown metric"); return GLIA_HMT_ERR_ARG; }
  if (o.global_opt < 0 || o.global_opt > 2) { set_error("Error: unsupported globalOpt type..."); return GLIA_HMT_ERR_ARG; }   // :147
  if (n_truth > 1 && o.metric != GLIA_HMT_BC_LABEL_VI) { set_error("bc_label: several truth volumes need the VI metric (bc_label_vi)"); return GLIA_HMT_ERR_ARG; }
  if (o.metric == GLIA_HMT_BC_LABEL_VI && (o.tweak || o.opt_split || o.max_prec_drop < 1.0)) {
    set_error("bc_label: tweak, mpd and optSplit are options of bc_label_ri, not of bc_label_vi");
    return GLIA_HMT_ERR_ARG;
  }
  if (rag->only_contour) { set_error("bc_label: the region map must hold region points (only_contour = 0)"); return GLIA_HMT_ERR_ARG; }
  if (!rag->vol.lab) { set_error("bc_label: needs the volumes the region map was built from (whole-volume build)"); return GLIA_HMT_ERR_UNSUPPORTED; }
  const int64_t R = rag->arr.R;
  std::vector<uint32_t> rlabel, forced;
  if (int rc = dense_order_of(rag, "bc_label", h_order, n_merges, &rlabel, &forced)) return rc;
  rag->bcl = glia_hmt_bc_label_timing{0, 0, 0, 0, 0, 0};
  if (n_merges == 0) return GLIA_HMT_OK;
  GLIA_HIP_TRY(hipSetDevice(c->device));
  const unsigned long long N = (unsigned long long)(rag->vol.nx * rag->vol.ny * rag->vol.nz);
  std::vector<NodeTruthStats> st((size_t)n_truth);
  for (int t = 0; t < n_truth; ++t) {
    // with a mask vol.lab is the folded copy (masked-out voxels hold kMaskedLabel): no mask argument, 8 B per voxel
    std::vector<glia_hmt_overlap_entry> table;
    OverlapPass pass;
    if (int rc = label_overlap(rag->vol.lab, d_truth[t], nullptr, N, 0, c->stream, &table, &pass)) return rc;
    std::vector<TruthCount> cnt;
    leaf_truth_counts(table.data(), table.size(), rlabel.data(), R, kMaskedLabel, &cnt);
    const auto t0 = std::chrono::steady_clock::now();
    int64_t moves = 0, pairs = 0;
    node_truth_stats(cnt, (uint32_t)R, forced.data(), n_merges, &st[t], &moves, &pairs);
    rag->bcl.ms_count += pass.ms;
    rag->bcl.ms_nodes += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    rag->bcl.entries += (int64_t)cnt.size(); rag->bcl.moves += moves; rag->bcl.node_pairs += pairs;
  }
  const auto t1 = std::chrono::steady_clock::now();
  int rc = bc_label_rules(st, (uint32_t)R, forced.data(), n_merges, o, h_labels);
  rag->bcl.ms_rules = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
  return rc;
}

int glia_hmt_last_bc_label_timing(const glia_hmt_rag* r, glia_hmt_bc_label_timing* out) {
  if (!r || !out) return GLIA_HMT_ERR_ARG;
  *out = r->bcl;
  return GLIA_HMT_OK;
}

int glia_hmt_last_merge_timing(const glia_hmt_rag* r, double* ms_table, double* ms_init, double* ms_loop,
                               int64_t* n_scored) {
  if (!r) return GLIA_HMT_ERR_ARG;
  if (ms_table) *ms_table = r->ms_table;
  if (ms_init) *ms_init = r->ms_init;
  if (ms_loop) *ms_loop = r->ms_loop;
  if (n_scored) *n_scored = r->n_scored;
  return GLIA_HMT_OK;
}

}  // extern "C"
