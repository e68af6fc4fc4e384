// glia_amd/csrc/api_mlp.cpp -- C ABI: the MLP / logsig batch predictors (mlp_model.hpp: files, shapes, the host forward pass;
// mlp_predict.hip: the kernel).
#include <algorithm>
#include <cstring>

#include "api_types.hpp"
#include "mlp.hpp"

static int upload_doubles(glia_hmt_mlp* m, const std::vector<double>& v, const double** out, hipStream_t stream) {
  double* d = nullptr;
  if (int rc = m->allocs.alloc(&d, v.size())) return rc;
  if (!v.empty()) GLIA_HIP_TRY(hipMemcpyAsync(d, v.data(), sizeof(double) * v.size(), hipMemcpyHostToDevice, stream));
  GLIA_HIP_TRY(hipStreamSynchronize(stream));       // v may be a temporary
  *out = d;
  return GLIA_HMT_OK;
}

static int upload_mlp(glia_hmt_ctx* c, glia_hmt_mlp* m) {
  const HostMlp& h = m->host;
  DeviceMlp& d = m->dm;
  memset(&d, 0, sizeof(d));
  d.n_models = h.n_models; d.n1 = h.n1; d.n2 = h.n2; d.D = h.D;
  d.rescale = h.rescale ? 1 : 0; d.dim0 = h.dim0; d.dim1 = h.dim1; d.threshold = h.threshold;
  if (h.n1 > 0) {
    d.ub1 = mlp_unit_block(h.n1); d.nb1 = (h.n1 + d.ub1 - 1) / d.ub1;
    d.ub2 = mlp_unit_block(h.n2); d.nb2 = (h.n2 + d.ub2 - 1) / d.ub2;
  }
  int rc;
  for (int i = 0; i < h.n_models; ++i) {
    const double* w = h.w[i].data();
    if (h.n1 > 0) {
      const double* w1 = w + (size_t)h.D * h.n1;
      const double* w2 = w1 + (size_t)(h.n1 + 1) * h.n2;
      if ((rc = upload_doubles(m, mlp_block_weights(w, h.D, h.n1, d.ub1), &d.w0[i], c->stream))) return rc;
      if ((rc = upload_doubles(m, mlp_block_weights(w1, h.n1 + 1, h.n2, d.ub2), &d.w1[i], c->stream))) return rc;
      if ((rc = upload_doubles(m, std::vector<double>(w2, w2 + h.n2 + 1), &d.w2[i], c->stream))) return rc;
    } else if ((rc = upload_doubles(m, h.w[i], &d.w2[i], c->stream))) return rc;
  }
  for (int i = h.n_models; i < 3; ++i) { d.w0[i] = d.w0[0]; d.w1[i] = d.w1[0]; d.w2[i] = d.w2[0]; }
  if (h.rescale) {
    std::vector<double> den(h.mn.size());
    for (size_t j = 0; j < den.size(); ++j) den[j] = (h.mx[j] - h.mn[j]) + kMlpFeps;      // the denominator of mlp_rescale, row-independent
    if ((rc = upload_doubles(m, h.mn, &d.mn, c->stream)) || (rc = upload_doubles(m, den, &d.den, c->stream))) return rc;
  }
  return GLIA_HMT_OK;
}

static int check_mlp_predict_args(const char* who, const glia_hmt_mlp* m, const void* rows, int64_t n_rows, int dim, int64_t row_stride,
                                  const void* pred, const void* logit) {
  if (!m) { set_error(std::string(who) + ": NULL model"); return GLIA_HMT_ERR_ARG; }
  if (n_rows < 0 || dim < 1 || row_stride < dim || (n_rows > 0 && (!rows || (!pred && !logit)))) {
    set_error(std::string(who) + ": invalid argument");
    return GLIA_HMT_ERR_ARG;
  }
  if (dim != m->host.D - 1) {
    set_error(std::string(who) + ": rows of " + std::to_string(dim) + " columns, but the model is for " + std::to_string(m->host.D - 1));
    return GLIA_HMT_ERR_ARG;
  }
  return GLIA_HMT_OK;
}

extern "C" {

int glia_hmt_mlp_file_parse(const char* path, double* h_w, int64_t capacity, int64_t* n_weights) {
  if (!path || !n_weights) { set_error("mlp_file_parse: invalid argument"); return GLIA_HMT_ERR_ARG; }
  std::vector<double> w;
  const std::string bad = mlp_read_doubles(path, &w);
  if (!bad.empty()) { set_error(bad); return GLIA_HMT_ERR_IO; }
  if (w.empty()) { set_error(std::string("mlp: the model holds no weights: ") + path); return GLIA_HMT_ERR_IO; }
  *n_weights = (int64_t)w.size();
  if (h_w) {
    if ((int64_t)w.size() > capacity) { set_error("mlp_file_parse: capacity too small"); return GLIA_HMT_ERR_CAPACITY; }
    memcpy(h_w, w.data(), sizeof(double) * w.size());
  }
  return GLIA_HMT_OK;
}

int glia_hmt_mlp_limits(int n1, int n2, int* stage_max_dim, int* unit_block, int* slots, int* max_hidden, int* max_dim) {
  if (n1 < 0 || n2 < 0 || n1 > kMlpMaxHidden || n2 > kMlpMaxHidden || (n1 == 0) != (n2 == 0)) { set_error("mlp_limits: invalid hidden sizes"); return GLIA_HMT_ERR_ARG; }
  if (stage_max_dim) *stage_max_dim = mlp_stage_max_dim(n1, n2);
  if (unit_block) *unit_block = kMlpUnitBlock;
  if (slots) *slots = kMlpSlots;
  if (max_hidden) *max_hidden = kMlpMaxHidden;
  if (max_dim) *max_dim = kMlpMaxDim;
  return GLIA_HMT_OK;
}

int glia_hmt_mlp_loop_limits(int* max_hidden) {
  if (max_hidden) *max_hidden = kMlpLoopMaxHidden;
  return GLIA_HMT_OK;
}

int glia_hmt_mlp_predict_tile_rows(int dim, int n1, int n2, int* staged) {
  if (dim < 1 || dim > kMlpMaxDim || n1 < 0 || n2 < 0 || n1 > kMlpMaxHidden || n2 > kMlpMaxHidden || (n1 == 0) != (n2 == 0)) {
    set_error("mlp_predict_tile_rows: invalid argument");
    return GLIA_HMT_ERR_ARG;
  }
  const MlpPlan p = mlp_plan(dim, n1, n2);
  if (staged) *staged = p.staged;
  return p.tile_rows;
}

int glia_hmt_mlp_create(glia_hmt_ctx* c, int n_models, const double* const* h_weights, const int64_t* n_weights, int n1, int n2, const double* h_min,
                        const double* h_max, int64_t n_minmax, const double* dist, glia_hmt_mlp** out) {
  if (!out || !h_weights || !n_weights || (n_models != 1 && n_models != 3)) {
    set_error("mlp_create: one model, or three models with distributor arguments, expected");
    return GLIA_HMT_ERR_ARG;
  }
  if (n_models == 3 && !dist) { set_error("Error: model distributor needs 3 arguments..."); return GLIA_HMT_ERR_ARG; }
  if ((h_min == nullptr) != (h_max == nullptr) || (h_min && n_minmax < 0)) { set_error("mlp_create: minima and maxima come together"); return GLIA_HMT_ERR_ARG; }
  if (n1 < 0 || n2 < 0 || (n1 == 0) != (n2 == 0)) { set_error("mlp: hidden sizes must both be positive (or both 0: the logsig model)"); return GLIA_HMT_ERR_ARG; }
  for (int i = 0; i < n_models; ++i)
    if (!h_weights[i] || n_weights[i] < 0) { set_error("mlp_create: NULL weights"); return GLIA_HMT_ERR_ARG; }
  int D = 0;
  bool beyond_limits = false;
  std::string bad = mlp_shape(n_weights[0], n1, n2, &D, &beyond_limits);
  if (!bad.empty()) { set_error(bad); return beyond_limits ? GLIA_HMT_ERR_UNSUPPORTED : GLIA_HMT_ERR_ARG; }
  glia_hmt_mlp* m = new glia_hmt_mlp;
  HostMlp& h = m->host;
  h.n_models = n_models; h.n1 = n1; h.n2 = n2; h.D = D;
  for (int i = 0; i < n_models; ++i) h.w[i].assign(h_weights[i], h_weights[i] + n_weights[i]);
  if (h_min) {
    if (n_minmax < D - 1) {
      delete m;
      set_error("mlp: fewer min/max entries (" + std::to_string(n_minmax) + ") than columns (" + std::to_string(D - 1) + ")");
      return GLIA_HMT_ERR_ARG;
    }
    h.rescale = true;
    h.mn.assign(h_min, h_min + (D - 1)); h.mx.assign(h_max, h_max + (D - 1));
  }
  if (dist && n_models == 3) {
    // the reference converts the arguments to int the same way (type/function.hxx:76-78); NaN and out-of-range values are refused
    if (!(dist[0] >= 0.0 && dist[0] <= (double)(D - 1) && dist[1] >= 0.0 && dist[1] <= (double)(D - 1))) {
      delete m;
      set_error("mlp: distributor dimension outside [0, " + std::to_string(D - 1) + "]");
      return GLIA_HMT_ERR_ARG;
    }
    h.dim0 = (int)dist[0]; h.dim1 = (int)dist[1]; h.threshold = dist[2];
  }
  bad = mlp_check(h);
  if (!bad.empty()) { delete m; set_error(bad); return GLIA_HMT_ERR_ARG; }
  if (c) {
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) { delete m; set_error(std::string("mlp_create: ") + hipGetErrorString(e)); return GLIA_HMT_ERR_HIP; }
    m->device = c->device;
    if (int rc = upload_mlp(c, m)) { delete m; return rc; }
  }
  *out = m;
  return GLIA_HMT_OK;
}

int glia_hmt_mlp_load(glia_hmt_ctx* c, int n_models, const char* const* paths, int n1, int n2, const char* minmax_path, const double* dist,
                      glia_hmt_mlp** out) {
  if (!paths || !out || (n_models != 1 && n_models != 3)) {
    set_error("mlp_load: one model, or three models with distributor arguments, expected");
    return GLIA_HMT_ERR_ARG;
  }
  std::vector<double> w[3], mn, mx;
  const double* ptr[3] = {nullptr, nullptr, nullptr};
  int64_t n[3] = {0, 0, 0};
  for (int i = 0; i < n_models; ++i) {
    if (!paths[i]) { set_error("mlp_load: NULL path"); return GLIA_HMT_ERR_ARG; }
    const std::string bad = mlp_read_doubles(paths[i], &w[i]);
    if (!bad.empty()) { set_error(bad); return GLIA_HMT_ERR_IO; }
    if (w[i].empty()) { set_error(std::string("mlp: the model holds no weights: ") + paths[i]); return GLIA_HMT_ERR_IO; }
    ptr[i] = w[i].data(); n[i] = (int64_t)w[i].size();
  }
  if (minmax_path) {
    const std::string bad = mlp_read_minmax(minmax_path, &mn, &mx);
    if (!bad.empty()) { set_error(bad); return GLIA_HMT_ERR_IO; }
  }
  const int64_t nmm = (int64_t)std::min(mn.size(), mx.size());
  return glia_hmt_mlp_create(c, n_models, ptr, n, n1, n2, minmax_path ? mn.data() : nullptr, minmax_path ? mx.data() : nullptr, nmm, dist, out);
}

int glia_hmt_mlp_dim(const glia_hmt_mlp* m) {
  if (!m) { set_error("mlp_dim: NULL model"); return GLIA_HMT_ERR_ARG; }
  return m->host.D - 1;
}

void glia_hmt_mlp_free(glia_hmt_mlp* m) {
  if (!m) return;
  if (m->device >= 0) (void)hipSetDevice(m->device);
  delete m;                               // (its arrays go with it)
}

int glia_hmt_mlp_predict_host(const glia_hmt_mlp* m, const double* h_rows, int64_t n_rows, int dim, double* h_pred, double* h_logit) {
  const int rc = check_mlp_predict_args("mlp_predict_host", m, h_rows, n_rows, dim, dim, h_pred, h_logit);
  if (rc || n_rows == 0) return rc;
  mlp_forward(m->host, h_rows, n_rows, dim, h_pred, h_logit);
  return GLIA_HMT_OK;
}

int glia_hmt_mlp_predict_device(glia_hmt_ctx* c, const glia_hmt_mlp* m, const double* d_rows, int64_t n_rows, int dim, int64_t row_stride,
                                double* d_pred, double* d_logit) {
  if (!c) { set_error("mlp_predict_device: NULL context"); return GLIA_HMT_ERR_ARG; }
  const int rc = check_mlp_predict_args("mlp_predict_device", m, d_rows, n_rows, dim, row_stride, d_pred, d_logit);
  if (rc) return rc;
  if (m->device != c->device) { set_error("mlp_predict_device: the model was not created on this context's device"); return GLIA_HMT_ERR_ARG; }
  if (n_rows == 0) return GLIA_HMT_OK;
  GLIA_HIP_TRY(hipSetDevice(c->device));
  return launch_mlp_predict(m->dm, d_rows, n_rows, row_stride, d_pred, d_logit, c->stream);
}

int glia_hmt_mlp_predict(glia_hmt_ctx* c, const glia_hmt_mlp* m, const double* h_rows, int64_t n_rows, int dim, double* h_pred, double* h_logit) {
  if (!c) { set_error("mlp_predict: NULL context"); return GLIA_HMT_ERR_ARG; }
  int rc = check_mlp_predict_args("mlp_predict", m, h_rows, n_rows, dim, dim, h_pred, h_logit);
  if (rc) return rc;
  if (m->device != c->device) { set_error("mlp_predict: the model was not created on this context's device"); return GLIA_HMT_ERR_ARG; }
  if (n_rows == 0) return GLIA_HMT_OK;
  GLIA_HIP_TRY(hipSetDevice(c->device));
  // rows stream through device buffers of at most 128 MiB (GLIA_HMT_MINCAP: 256 rows, so that tests cross chunk boundaries); the
  // kernel hands back logits, the sigmoid is the host's (its own exp: what a host program computes from that logit)
  const int64_t chunk = std::min<int64_t>(n_rows, option("GLIA_HMT_MINCAP") ? 256 : std::max<int64_t>(1, (int64_t)(1 << 24) / dim));
  OwnedArrays own;
  double *d_rows = nullptr, *d_logit = nullptr;
  if ((rc = own.alloc(&d_rows, (size_t)chunk * dim)) || (rc = own.alloc(&d_logit, (size_t)chunk))) return rc;
  std::vector<double> lg((size_t)chunk);
  hipError_t e = hipSuccess;
  for (int64_t r0 = 0; e == hipSuccess && rc == GLIA_HMT_OK && r0 < n_rows; r0 += chunk) {
    const int64_t n = std::min(chunk, n_rows - r0);
    e = hipMemcpyAsync(d_rows, h_rows + r0 * dim, sizeof(double) * (size_t)n * dim, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) rc = launch_mlp_predict(m->dm, d_rows, n, dim, nullptr, d_logit, c->stream);
    if (e == hipSuccess && rc == GLIA_HMT_OK) e = hipMemcpyAsync(lg.data(), d_logit, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess && rc == GLIA_HMT_OK) {
      for (int64_t i = 0; i < n; ++i) {
        if (h_logit) h_logit[r0 + i] = lg[i];
        if (h_pred) h_pred[r0 + i] = mlp_sigmoid(lg[i]);
      }
    }
  }
  if (e != hipSuccess) { set_error(std::string("mlp_predict: ") + hipGetErrorString(e)); return GLIA_HMT_ERR_HIP; }
  return rc;
}

}  // extern "C"
