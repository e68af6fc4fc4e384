// glia_amd/csrc/api_mlp_train.cpp -- C ABI: training the MLP / logsig classifier (mlp_backward.hpp: the definition and the trainer;
// mlp_train.hip: the device evaluator), without and with the merge-path term (sshmt_paths.hpp; sshmt_train.hip): one path through both.
#include <chrono>
#include <cstdio>
#include <cstring>

#include "api_types.hpp"
#include "mlp_backward.hpp"
#include "mlp_batch.hpp"
#include "sshmt_paths.hpp"

struct glia_hmt_mlp_model {
  glia::MlpTrainResult r;
};

namespace {

// the unlabelled blocks of glia_hmt_sshmt_train: checked, the rows prepared as the labelled ones are, the paths and incidence lists built
int prepare_blocks(const glia_hmt_sshmt_block* blocks, int n_blocks, int dim, const double* h_min, const double* h_max,
                   const glia_hmt_sshmt_train_opts& so, SshmtInput* input) {
  if (n_blocks < 0 || (n_blocks > 0 && !blocks)) { set_error("sshmt_train: invalid blocks"); return GLIA_HMT_ERR_ARG; }
  const std::string bad = sshmt_bad_lengths(so.max_path_length, so.min_path_length);
  if (!bad.empty()) { set_error(bad); return GLIA_HMT_ERR_UNSUPPORTED; }
  SshmtInput& in = *input;
  in.D = dim + 1;
  sshmt_fill_tables(so.merge_target, so.path_target, &in.tb);
  for (int b = 0; b < n_blocks; ++b) {
    const glia_hmt_sshmt_block& B = blocks[b];
    const std::string me = "sshmt_train: block " + std::to_string(b);
    if (B.n_merges < 0 || (B.n_merges > 0 && (!B.rows || !B.order))) { set_error(me + ": rows and order must both be given, one row per merge"); return GLIA_HMT_ERR_ARG; }
    const int64_t first_bad = sshmt_check_order(B.order, B.n_merges);
    if (first_bad >= 0) {
      set_error(me + ": merge " + std::to_string(first_bad) + " of its order joins a region that does not exist (any more) or creates one that does");
      return GLIA_HMT_ERR_ARG;
    }
    for (int64_t i = 0; i < B.n_merges * dim; ++i)
      if (!std::isfinite(B.rows[i])) { set_error(me + ": row " + std::to_string(i / dim) + " holds a value that is not finite"); return GLIA_HMT_ERR_ARG; }
    merge_paths(B.order, B.n_merges, so.max_path_length, so.min_path_length, in.n_rows, &in.offsets, &in.members);
    for (int64_t r = 0; r < B.n_merges; ++r) {
      for (int j = 0; j < dim; ++j) {
        const double v = B.rows[(size_t)r * dim + j];
        in.X.push_back(h_min ? mlp_rescale_den(v, h_min[j], (h_max[j] - h_min[j]) + kMlpTrainFeps) : v);
      }
      in.X.push_back(1.0);
    }
    in.n_rows += B.n_merges;
  }
  for (double v : in.X)
    if (!std::isfinite(v)) { set_error("sshmt_train: a rescaled unlabelled row holds a value that is not finite"); return GLIA_HMT_ERR_ARG; }
  sshmt_incidence(in.offsets, in.members, in.n_rows, &in.inc_off, &in.inc);
  return GLIA_HMT_OK;
}

// One training call, whichever entry point it came through.  c == NULL: the definition on one host thread.  with_u: the caller has the
// merge-path term (glia_hmt_sshmt_train): wu, update_sigma_u, so's own fields and the blocks count, and labelled rows may be absent
// while ws is off.  bo != NULL: the caller is a *_train_batches entry point: the batch fields of the options are
// honoured, and with a sampler on the mini-batch step takes the update's place.
int train(glia_hmt_ctx* c, bool with_u, const double* h_rows, int64_t n_rows, int dim, const int32_t* h_labels, const glia_hmt_sshmt_block* blocks,
          int n_blocks, const glia_hmt_sshmt_train_opts& so, const double* h_min, const double* h_max, const double* h_init,
          glia_hmt_mlp_model** out, const glia_hmt_batch_opts* bo = nullptr) {
  const auto t0 = std::chrono::steady_clock::now();
  const std::string me = std::string(with_u ? "sshmt_train" : "mlp_train") + (c ? ": " : "_host: ");
  if (!out || n_rows < 0 || dim < 1 || (n_rows > 0 && (!h_rows || !h_labels))) { set_error(me + "invalid argument"); return GLIA_HMT_ERR_ARG; }
  *out = nullptr;
  if ((h_min == nullptr) != (h_max == nullptr)) { set_error(me + "minima and maxima come together"); return GLIA_HMT_ERR_ARG; }
  const glia_hmt_mlp_train_opts& o = so.base;
  std::string bad = with_u ? sshmt_train_bad_opts(so) : mlp_train_bad_opts(o);
  if (!bad.empty()) { set_error(bad); return GLIA_HMT_ERR_ARG; }
  bad = mlp_train_unsupported(o, with_u, bo != nullptr);
  if (!bad.empty()) { set_error(bad); return GLIA_HMT_ERR_UNSUPPORTED; }
  if (dim > kMlpTrainMaxDim) { set_error("mlp_train: rows of more than " + std::to_string(kMlpTrainMaxDim) + " columns are not supported"); return GLIA_HMT_ERR_UNSUPPORTED; }
  for (int64_t i = 0; i < n_rows * dim; ++i)
    if (!std::isfinite(h_rows[i])) { set_error("mlp_train: row " + std::to_string(i / dim) + " holds a value that is not finite"); return GLIA_HMT_ERR_ARG; }
  for (int j = 0; h_min && j < dim; ++j)
    if (!std::isfinite(h_min[j]) || !std::isfinite(h_max[j])) { set_error("mlp_train: the min/max table holds a value that is not finite"); return GLIA_HMT_ERR_ARG; }
  const int D = dim + 1;
  const long long d = mlp_train_n_weights(D, o.n1, o.n2);
  std::vector<double> X, t, w((size_t)d);      // the labelled rows as the trainer sees them, their targets, the weights
  SshmtInput in;                               // the unlabelled blocks as the path term sees them
  if (h_init) {
    for (long long p = 0; p < d; ++p) {
      if (!std::isfinite(h_init[p])) { set_error("mlp_train: initial weight " + std::to_string(p) + " is not finite"); return GLIA_HMT_ERR_ARG; }
      w[p] = h_init[p];
    }
  } else if (o.n1 > 0) {
    for (long long p = 0; p < d; ++p) w[p] = mlp_init_weight(o.seed, (uint64_t)p);
  }
  mlp_train_prepare(h_rows, n_rows, dim, h_labels, h_min, h_max, o.pos_target, o.neg_target, &X, &t);
  if (t.empty() && (!with_u || !mlp_isfeq(o.ws, 0.0))) { set_error("mlp_train: no row is labelled +1 or -1"); return GLIA_HMT_ERR_ARG; }
  for (double v : X)
    if (!std::isfinite(v)) { set_error("mlp_train: a rescaled row holds a value that is not finite"); return GLIA_HMT_ERR_ARG; }
  if (with_u)
    if (int rc = prepare_blocks(blocks, n_blocks, dim, h_min, h_max, so, &in)) return rc;

  // an evaluator exists only for a term that is on: the trainer asks no other (the supervised trainer has always had its own)
  const bool on_s = !with_u || (!t.empty() && !mlp_isfeq(o.ws, 0.0)), on_u = with_u && in.n_paths() > 0 && !mlp_isfeq(o.wu, 0.0);
  std::unique_ptr<MlpTrainEval> ev, eu;
  // the context's record of its last call: the device evaluators add to it; a call that fails leaves it zeroed
  glia_hmt_mlp_train_timing* tm = !c ? nullptr : with_u ? &c->sst.sup : &c->mlt;
  auto zero_timing = [&]() {
    if (c && with_u) c->sst = glia_hmt_sshmt_train_timing();
    if (c && !with_u) c->mlt = glia_hmt_mlp_train_timing();
    if (c && bo) c->bat = glia_hmt_batch_timing();
  };
  // the samplers (sshmt_util.hxx:69-107), before any kernel
  std::unique_ptr<MlpBatchHostStep> step;
  if (bo) {
    MlpBatchSamplers S;
    std::vector<int32_t> lab;
    for (int64_t r = 0; r < n_rows; ++r) if (h_labels[r] == 1 || h_labels[r] == -1) lab.push_back(h_labels[r]);
    bad = mlp_batch_make_uns(in.n_paths(), o.uns_batch_size, bo->seed, &S.U, &S.on_u);
    if (bad.empty()) bad = mlp_batch_make_sup(lab.data(), (int64_t)lab.size(), o.sup_batch_size, o.balance_sup_batch, o.pos_target, o.neg_target, bo->seed, &S.S, &S.on_s);
    if (bad.empty() && ((S.on_u && !on_u) || (S.on_s && (!on_s || mlp_isfeq(o.ws, 0.0))))) bad = "train_batches: a batch sampler for a term that is off";
    if (!bad.empty()) { set_error(bad); return GLIA_HMT_ERR_ARG; }
    if (S.on_u || S.on_s) {
      int route = GLIA_HMT_BATCH_STREAM;
      std::string v;
      if (option("GLIA_HMT_BATCH", &v) && v != "stream") {
        if (v != "step") { set_error("train_batches: GLIA_HMT_BATCH must be stream or step, not '" + v + "'"); return GLIA_HMT_ERR_ARG; }
        route = GLIA_HMT_BATCH_STEP;
      }
      if (c) {
        GLIA_HIP_TRY(hipSetDevice(c->device));
        if (int rc = mlp_batch_device_create(c->stream, route, d, &step)) return rc;
      } else step.reset(new MlpBatchHostStep);
      step->bo = *bo; step->samplers = S; step->in = &in;
    }
  }
  if (c) {
    GLIA_HIP_TRY(hipSetDevice(c->device));
    zero_timing();
    if (on_s)
      if (int rc = mlp_train_device_create(X.data(), t.data(), (long long)t.size(), D, o.n1, o.n2, c->libm.exp_variant, c->stream, tm, &ev)) { zero_timing(); return rc; }
    if (on_u)
      if (int rc = sshmt_train_device_create(in, o.n1, o.n2, c->libm.exp_variant, c->stream, &c->sst, &eu)) { zero_timing(); return rc; }
  } else {
    if (on_s) {
      MlpTrainHostEval* h = new MlpTrainHostEval;
      ev.reset(h);
      h->D = D; h->n1 = o.n1; h->n2 = o.n2; h->X = X.data(); h->t = t.data(); h->n = (int64_t)t.size();
    }
    if (on_u) {
      SshmtHostEval* h = new SshmtHostEval;
      eu.reset(h);
      h->n1 = o.n1; h->n2 = o.n2; h->in = &in;
    }
  }
  std::unique_ptr<glia_hmt_mlp_model> m(new glia_hmt_mlp_model);
  MlpTrainResult& R = m->r;
  R.D = D; R.n1 = o.n1; R.n2 = o.n2; R.n_used = (int64_t)t.size();
  if (h_min) { R.mn.assign(h_min, h_min + dim); R.mx.assign(h_max, h_max + dim); }
  R.n_paths = in.n_paths(); R.n_uns_rows = in.n_rows;
  MlpTrainUns U;
  U.ev = eu.get(); U.n_paths = R.n_paths; U.n_rows = R.n_uns_rows; U.wu = o.wu; U.sigma_u = so.sigma_u; U.min_sigma2 = o.min_sigma2;
  U.update_sigma_u = o.update_sigma_u;
  if (step) { step->ev = ev.get(); step->eu = eu.get(); }
  if (int rc = mlp_train_run(o, R.n_used, w, ev.get(), &R, with_u ? &U : nullptr, step.get())) { zero_timing(); return rc; }
  if (c && step) c->bat = step->tm;
  if (R.round_w.empty()) R.round_w.push_back(w);
  if (c) {
    for (const glia_hmt_mlp_train_record& r : R.trace) tm->iterations += r.kind == 0;
    tm->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (with_u) { c->sst.n_paths = R.n_paths; c->sst.n_uns_rows = R.n_uns_rows; }
  }
  *out = m.release();
  return GLIA_HMT_OK;
}

int pick_round(const glia_hmt_mlp_model* m, int round, const char* who) {
  const int n = (int)m->r.round_w.size();
  if (round == -1) round = n - 1;
  if (round < 0 || round >= n) { set_error(std::string(who) + ": the model holds rounds 0 to " + std::to_string(n - 1)); return -1; }
  return round;
}

}  // namespace

extern "C" {

void glia_hmt_mlp_train_opts_default(glia_hmt_mlp_train_opts* opts) {
  if (opts) mlp_train_opts_default(opts);
}

int glia_hmt_mlp_train(glia_hmt_ctx* c, const double* h_rows, int64_t n_rows, int dim, const int32_t* h_labels,
                       const glia_hmt_mlp_train_opts* opts, const double* h_min, const double* h_max, const double* h_init,
                       glia_hmt_mlp_model** out) {
  glia_hmt_sshmt_train_opts so;
  sshmt_train_opts_default(&so);
  if (opts) so.base = *opts;
  return train(c, false, h_rows, n_rows, dim, h_labels, nullptr, 0, so, h_min, h_max, h_init, out);
}

int glia_hmt_mlp_train_host(const double* h_rows, int64_t n_rows, int dim, const int32_t* h_labels, const glia_hmt_mlp_train_opts* opts,
                            const double* h_min, const double* h_max, const double* h_init, glia_hmt_mlp_model** out) {
  return glia_hmt_mlp_train(nullptr, h_rows, n_rows, dim, h_labels, opts, h_min, h_max, h_init, out);
}

void glia_hmt_sshmt_train_opts_default(glia_hmt_sshmt_train_opts* opts) {
  if (opts) sshmt_train_opts_default(opts);
}

int glia_hmt_sshmt_train(glia_hmt_ctx* c, const double* h_rows, int64_t n_rows, int dim, const int32_t* h_labels,
                         const glia_hmt_sshmt_block* blocks, int n_blocks, const glia_hmt_sshmt_train_opts* opts, const double* h_min,
                         const double* h_max, const double* h_init, glia_hmt_mlp_model** out) {
  glia_hmt_sshmt_train_opts so;
  sshmt_train_opts_default(&so);
  if (opts) so = *opts;
  return train(c, true, h_rows, n_rows, dim, h_labels, blocks, n_blocks, so, h_min, h_max, h_init, out);
}

int glia_hmt_sshmt_train_host(const double* h_rows, int64_t n_rows, int dim, const int32_t* h_labels, const glia_hmt_sshmt_block* blocks,
                              int n_blocks, const glia_hmt_sshmt_train_opts* opts, const double* h_min, const double* h_max,
                              const double* h_init, glia_hmt_mlp_model** out) {
  return glia_hmt_sshmt_train(nullptr, h_rows, n_rows, dim, h_labels, blocks, n_blocks, opts, h_min, h_max, h_init, out);
}

void glia_hmt_batch_opts_default(glia_hmt_batch_opts* opts) {
  if (opts) { opts->seed = 0; opts->epochs_per_iteration = 1; opts->batches_per_iteration = 1; }
}

int glia_hmt_mlp_train_batches(glia_hmt_ctx* c, const double* h_rows, int64_t n_rows, int dim, const int32_t* h_labels,
                               const glia_hmt_mlp_train_opts* opts, const glia_hmt_batch_opts* batch, const double* h_min, const double* h_max,
                               const double* h_init, glia_hmt_mlp_model** out) {
  glia_hmt_sshmt_train_opts so;
  glia_hmt_batch_opts bo;
  sshmt_train_opts_default(&so);
  glia_hmt_batch_opts_default(&bo);
  if (opts) so.base = *opts;
  if (batch) bo = *batch;
  return train(c, false, h_rows, n_rows, dim, h_labels, nullptr, 0, so, h_min, h_max, h_init, out, &bo);
}

int glia_hmt_sshmt_train_batches(glia_hmt_ctx* c, const double* h_rows, int64_t n_rows, int dim, const int32_t* h_labels,
                                 const glia_hmt_sshmt_block* blocks, int n_blocks, const glia_hmt_sshmt_train_opts* opts,
                                 const glia_hmt_batch_opts* batch, const double* h_min, const double* h_max, const double* h_init,
                                 glia_hmt_mlp_model** out) {
  glia_hmt_sshmt_train_opts so;
  glia_hmt_batch_opts bo;
  sshmt_train_opts_default(&so);
  glia_hmt_batch_opts_default(&bo);
  if (opts) so = *opts;
  if (batch) bo = *batch;
  return train(c, true, h_rows, n_rows, dim, h_labels, blocks, n_blocks, so, h_min, h_max, h_init, out, &bo);
}

int glia_hmt_batch_plan(const int32_t* h_labels, int64_t n_rows, int64_t n_paths, int sup_batch_size, int uns_batch_size,
                        int balance_sup_batch, double pos_target, double neg_target, uint64_t seed, int k, int64_t* n_sup, int64_t* n_uns,
                        int64_t* sup_offsets, int32_t* sup_rows, int64_t* uns_offsets, int32_t* uns_paths, int32_t* end_of_epoch) {
  const bool fill = sup_offsets != nullptr;
  if (n_rows < 0 || n_paths < 0 || k < 0 || (n_rows > 0 && !h_labels) || !n_sup || !n_uns || fill != (sup_rows != nullptr) ||
      fill != (uns_offsets != nullptr) || fill != (uns_paths != nullptr)) {
    set_error("batch_plan: invalid argument");
    return GLIA_HMT_ERR_ARG;
  }
  for (int64_t r = 0; r < n_rows; ++r)
    if (h_labels[r] != 1 && h_labels[r] != -1) { set_error("batch_plan: label " + std::to_string(r) + " is neither +1 nor -1"); return GLIA_HMT_ERR_ARG; }
  MlpBatchSamplers S;
  std::string bad = mlp_batch_make_uns(n_paths, uns_batch_size, seed, &S.U, &S.on_u);
  if (bad.empty()) bad = mlp_batch_make_sup(h_labels, n_rows, sup_batch_size, balance_sup_batch, pos_target, neg_target, seed, &S.S, &S.on_s);
  if (!bad.empty()) { set_error(bad); return GLIA_HMT_ERR_ARG; }
  const int64_t ns = S.on_s ? (int64_t)k * S.S.batch_size() : 0, nu = S.on_u ? (int64_t)k * S.U.batch_size() : 0;
  if (fill && (*n_sup != ns || *n_uns != nu)) { set_error("batch_plan: the sizes are not those of the first call"); return GLIA_HMT_ERR_ARG; }
  *n_sup = ns; *n_uns = nu;
  if (!fill) return GLIA_HMT_OK;
  std::vector<int32_t> paths, rows;
  sup_offsets[0] = uns_offsets[0] = 0;
  for (int i = 0; i < k; ++i) {
    const bool end = S.draw(&paths, &rows);
    std::copy(rows.begin(), rows.end(), sup_rows + sup_offsets[i]);
    std::copy(paths.begin(), paths.end(), uns_paths + uns_offsets[i]);
    sup_offsets[i + 1] = sup_offsets[i] + (int64_t)rows.size();
    uns_offsets[i + 1] = uns_offsets[i] + (int64_t)paths.size();
    if (end_of_epoch) end_of_epoch[i] = end ? 1 : 0;
  }
  return GLIA_HMT_OK;
}

int glia_hmt_last_batch_timing(const glia_hmt_ctx* c, glia_hmt_batch_timing* out) {
  if (!c || !out) { set_error("last_batch_timing: invalid argument"); return GLIA_HMT_ERR_ARG; }
  *out = c->bat;
  return GLIA_HMT_OK;
}

int glia_hmt_merge_paths(const uint32_t* h_order, int64_t n_merges, int max_len, int min_len, int64_t* n_paths, int64_t* n_members,
                         int64_t* offsets, int64_t* members) {
  if (n_merges < 0 || (n_merges > 0 && !h_order) || !n_paths || !n_members || (offsets == nullptr) != (members == nullptr)) {
    set_error("merge_paths: invalid argument");
    return GLIA_HMT_ERR_ARG;
  }
  const std::string bad = sshmt_bad_lengths(max_len, min_len);
  if (!bad.empty()) { set_error(bad); return GLIA_HMT_ERR_UNSUPPORTED; }
  const int64_t first_bad = sshmt_check_order(h_order, n_merges);
  if (first_bad >= 0) {
    set_error("merge_paths: merge " + std::to_string(first_bad) + " joins a region that does not exist (any more) or creates one that does");
    return GLIA_HMT_ERR_ARG;
  }
  std::vector<int64_t> off, mem;
  merge_paths(h_order, n_merges, max_len, min_len, 0, &off, &mem);
  if (offsets) {
    if (*n_paths != (int64_t)off.size() - 1 || *n_members != (int64_t)mem.size()) { set_error("merge_paths: the sizes are not those of the first call"); return GLIA_HMT_ERR_ARG; }
    std::copy(off.begin(), off.end(), offsets);
    std::copy(mem.begin(), mem.end(), members);
  }
  *n_paths = (int64_t)off.size() - 1; *n_members = (int64_t)mem.size();
  return GLIA_HMT_OK;
}

int glia_hmt_mlp_model_sigmas_u(const glia_hmt_mlp_model* m, double* h_sigma2, double* h_sigma2_eval) {
  if (!m) { set_error("mlp_model_sigmas_u: NULL model"); return GLIA_HMT_ERR_ARG; }
  if (h_sigma2) std::copy(m->r.sigma_u2.begin(), m->r.sigma_u2.end(), h_sigma2);
  if (h_sigma2_eval) std::copy(m->r.sigma_u2_eval.begin(), m->r.sigma_u2_eval.end(), h_sigma2_eval);
  return GLIA_HMT_OK;
}

int glia_hmt_mlp_model_paths(const glia_hmt_mlp_model* m, int64_t* n_paths, int64_t* n_uns_rows) {
  if (!m) { set_error("mlp_model_paths: NULL model"); return GLIA_HMT_ERR_ARG; }
  if (n_paths) *n_paths = m->r.n_paths;
  if (n_uns_rows) *n_uns_rows = m->r.n_uns_rows;
  return GLIA_HMT_OK;
}

int glia_hmt_last_sshmt_train_timing(const glia_hmt_ctx* c, glia_hmt_sshmt_train_timing* out) {
  if (!c || !out) { set_error("last_sshmt_train_timing: invalid argument"); return GLIA_HMT_ERR_ARG; }
  *out = c->sst;
  return GLIA_HMT_OK;
}

int glia_hmt_mlp_model_info(const glia_hmt_mlp_model* m, int* rounds, int64_t* n_weights, int64_t* n_trace, int* stopped_nonfinite,
                            int64_t* n_used_rows, int* n_sigma) {
  if (!m) { set_error("mlp_model_info: NULL model"); return GLIA_HMT_ERR_ARG; }
  if (rounds) *rounds = (int)m->r.round_w.size();
  if (n_weights) *n_weights = (int64_t)m->r.round_w[0].size();
  if (n_trace) *n_trace = (int64_t)m->r.trace.size();
  if (stopped_nonfinite) *stopped_nonfinite = m->r.stopped_nonfinite;
  if (n_used_rows) *n_used_rows = m->r.n_used;
  if (n_sigma) *n_sigma = (int)m->r.sigma2.size();
  return GLIA_HMT_OK;
}

int glia_hmt_mlp_model_weights(const glia_hmt_mlp_model* m, int round, double* h_w) {
  if (!m || !h_w) { set_error("mlp_model_weights: invalid argument"); return GLIA_HMT_ERR_ARG; }
  if ((round = pick_round(m, round, "mlp_model_weights")) < 0) return GLIA_HMT_ERR_ARG;
  memcpy(h_w, m->r.round_w[round].data(), sizeof(double) * m->r.round_w[round].size());
  return GLIA_HMT_OK;
}

int glia_hmt_mlp_model_trace(const glia_hmt_mlp_model* m, glia_hmt_mlp_train_record* h_records) {
  if (!m || (!h_records && !m->r.trace.empty())) { set_error("mlp_model_trace: invalid argument"); return GLIA_HMT_ERR_ARG; }
  if (!m->r.trace.empty()) memcpy(h_records, m->r.trace.data(), sizeof(glia_hmt_mlp_train_record) * m->r.trace.size());
  return GLIA_HMT_OK;
}

int glia_hmt_mlp_model_sigmas(const glia_hmt_mlp_model* m, double* h_sigma2, double* h_sigma2_eval) {
  if (!m) { set_error("mlp_model_sigmas: NULL model"); return GLIA_HMT_ERR_ARG; }
  if (h_sigma2) std::copy(m->r.sigma2.begin(), m->r.sigma2.end(), h_sigma2);
  if (h_sigma2_eval) std::copy(m->r.sigma2_eval.begin(), m->r.sigma2_eval.end(), h_sigma2_eval);
  return GLIA_HMT_OK;
}

int glia_hmt_mlp_model_write(const glia_hmt_mlp_model* m, const char* path, int round) {
  if (!m || !path) { set_error("mlp_model_write: invalid argument"); return GLIA_HMT_ERR_ARG; }
  if ((round = pick_round(m, round, "mlp_model_write")) < 0) return GLIA_HMT_ERR_ARG;
  FILE* f = fopen(path, "w");
  if (!f) { set_error(std::string("Error: cannot open file ") + path); return GLIA_HMT_ERR_IO; }
  bool ok = true;
  for (double v : m->r.round_w[round]) ok = fprintf(f, "%.17g\n", v) > 0 && ok;
  ok = fclose(f) == 0 && ok;
  if (!ok) { set_error(std::string("mlp_model_write: cannot write ") + path); return GLIA_HMT_ERR_IO; }
  return GLIA_HMT_OK;
}

int glia_hmt_mlp_model_create_mlp(glia_hmt_ctx* c, const glia_hmt_mlp_model* m, int round, glia_hmt_mlp** out) {
  if (!m || !out) { set_error("mlp_model_create_mlp: invalid argument"); return GLIA_HMT_ERR_ARG; }
  if ((round = pick_round(m, round, "mlp_model_create_mlp")) < 0) return GLIA_HMT_ERR_ARG;
  const double* w = m->r.round_w[round].data();
  const int64_t nw = (int64_t)m->r.round_w[round].size();
  const bool mm = !m->r.mn.empty();
  return glia_hmt_mlp_create(c, 1, &w, &nw, m->r.n1, m->r.n2, mm ? m->r.mn.data() : nullptr, mm ? m->r.mx.data() : nullptr, (int64_t)m->r.mn.size(),
                             nullptr, out);
}

void glia_hmt_mlp_model_free(glia_hmt_mlp_model* m) { delete m; }

int glia_hmt_mlp_train_limits(int* chunk_rows, int* max_hidden, int* max_dim) {
  if (chunk_rows) *chunk_rows = kMlpTrainChunk;
  if (max_hidden) *max_hidden = kMlpTrainMaxHidden;
  if (max_dim) *max_dim = kMlpTrainMaxDim;
  return GLIA_HMT_OK;
}

double glia_hmt_mlp_init_weight(uint64_t seed, uint64_t p) { return mlp_init_weight(seed, p); }

int glia_hmt_rows_minmax(const double* const* h_blocks, const int64_t* n_rows, int n_blocks, int dim, double* h_min, double* h_max) {
  if (!h_blocks || !n_rows || n_blocks < 0 || dim < 1 || !h_min || !h_max) { set_error("rows_minmax: invalid argument"); return GLIA_HMT_ERR_ARG; }
  for (int b = 0; b < n_blocks; ++b)
    if (n_rows[b] < 0 || (n_rows[b] > 0 && !h_blocks[b])) { set_error("rows_minmax: invalid block"); return GLIA_HMT_ERR_ARG; }
  mlp_rows_minmax(h_blocks, n_rows, n_blocks, dim, h_min, h_max);
  return GLIA_HMT_OK;
}

int glia_hmt_last_mlp_train_timing(const glia_hmt_ctx* c, glia_hmt_mlp_train_timing* out) {
  if (!c || !out) { set_error("last_mlp_train_timing: invalid argument"); return GLIA_HMT_ERR_ARG; }
  *out = c->mlt;
  return GLIA_HMT_OK;
}

}  // extern "C"
