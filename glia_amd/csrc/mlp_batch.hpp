// glia_amd/csrc/mlp_batch.hpp -- mini-batch training of the MLP / logsig classifier, host only: the batch samplers of
// type/sampler.hxx:45-233 over a stated source of randomness, the choice of sampler of sshmt/sshmt_util.hxx:69-107, the draw rule of
// type/energy_function.hxx:42-49, the plan of one mini-batch step (alg/gd.hxx:86-157) and the step itself over the evaluators of
// mlp_backward.hpp and sshmt_paths.hpp.  The device's route through the same plan is mlp_batch.hip.
//
// The reference shuffles with std::random_shuffle, whose rand() state depends on everything shuffled before: its batch sequence is
// not a function of its inputs.  Here permutation number s of a stream is Fisher-Yates over the stream's indices in ASCENDING order,
//   h = mix(mix(mix(seed) ^ stream) ^ s);  for i = 1 .. n-1: j = mix(h ^ i) mod (i + 1); swap(a[i], a[j])
// with mix = mlp_mix (splitmix64's finaliser, the one behind the initial weights and the forest's bootstrap): a pure function of
// (seed, stream, s, n).  The reference reshuffles the permuted array in place; starting from the ascending order instead makes every
// permutation computable without replaying the ones before it.  Streams: 0 = paths, 1 = labelled rows, 2 + c = class c.
#pragma once
#include <chrono>
#include <cstring>

#include "sshmt_paths.hpp"

namespace glia {

inline void mlp_batch_perm(uint64_t seed, uint64_t stream, uint64_t s, const std::vector<int32_t>& ascending, std::vector<int32_t>* a) {
  *a = ascending;
  const uint64_t h = mlp_mix(mlp_mix(mlp_mix(seed) ^ stream) ^ s);
  for (size_t i = 1; i < a->size(); ++i) std::swap((*a)[i], (*a)[(size_t)(mlp_mix(h ^ (uint64_t)i) % (uint64_t)(i + 1))]);
}

// One stream of indices: its current permutation, the position in it, the number of the permutation.
struct MlpBatchStream {
  uint64_t seed = 0, stream = 0, s = 0;
  std::vector<int32_t> ascending, all;
  int32_t share = 0;      // entries per batch
  size_t cur = 0;
  bool visited = false;
  void shuffle(uint64_t number) { s = number; mlp_batch_perm(seed, stream, s, ascending, &all); }
  // share entries to out; true: the stream reached its end.  The entries after the end come from the START of the same permutation
  // (sampler.hxx:78-84, 203-210).
  bool take(std::vector<int32_t>* out) {
    bool wrapped = false;
    for (int32_t j = 0; j < share; ++j) {
      out->push_back(all[cur++]);
      if (cur >= all.size()) { wrapped = true; cur = 0; }
    }
    return wrapped;
  }
};

// UniformBatchSampler (one stream) or ClassBatchSampler (one stream per class, in the batch's class order)
struct MlpBatchSampler {
  bool by_class = false;
  std::vector<MlpBatchStream> st;
  int64_t batch_size() const { int64_t b = 0; for (const MlpBatchStream& c : st) b += c.share; return b; }
  void reset() {      // sampler.hxx:52-56, 112-121
    for (MlpBatchStream& c : st) { c.cur = 0; c.visited = c.share <= 0; c.shuffle(c.all.empty() ? 0 : c.s + 1); }
  }
  // the next batch to out (cleared first); true: EndOfEpoch
  bool draw(std::vector<int32_t>* out) {
    out->clear();
    for (MlpBatchStream& c : st) {
      const bool wrapped = c.take(out);
      if (wrapped) c.visited = true;
      if (wrapped && by_class) c.shuffle(c.s + 1);      // sampler.hxx:211-215: the class alone, after its share
    }
    for (const MlpBatchStream& c : st) if (!c.visited) return false;
    reset();
    return true;
  }
};

// sshmt_util.hxx:69-107 for the labelled rows (labels [n]: +1 / -1 of the rows the trainer sees) and the paths.  Returns an error
// message or empty; *on: whether a sampler was asked for.
inline std::string mlp_batch_make_sup(const int32_t* labels, int64_t n, int sup_batch_size, int balance, double pos_target, double neg_target,
                                      uint64_t seed, MlpBatchSampler* S, bool* on) {
  *on = sup_batch_size > 0 || balance;
  if (!*on) return std::string();
  if (n > 0x7fffffffll) return "batch sampler: more than 2^31 labelled rows";
  auto stream = [&](uint64_t id, int32_t share) {
    MlpBatchStream c;
    c.seed = seed; c.stream = id; c.share = share;
    return c;
  };
  if (!balance) {
    if (n < sup_batch_size) return "Error: totalSize must be greater than batchSize";
    S->by_class = false;
    S->st.push_back(stream(1, sup_batch_size));
    for (int64_t r = 0; r < n; ++r) S->st[0].ascending.push_back((int32_t)r);
  } else {
    if (pos_target == neg_target) return "batch sampler: pos_target equals neg_target: the balanced sampler has one class";
    S->by_class = true;
    // class 0 then class 1 of the batch: positive then negative with a batch size (sshmt_util.hxx:71-75), ascending target without
    // (std::map, sampler.hxx:159-177)
    const bool pos_first = sup_batch_size > 0 || pos_target < neg_target;
    S->st.push_back(stream(2, 0));
    S->st.push_back(stream(3, 0));
    for (int64_t r = 0; r < n; ++r) S->st[(labels[r] == 1) == pos_first ? 0 : 1].ascending.push_back((int32_t)r);
    const int64_t n0 = (int64_t)S->st[0].ascending.size(), n1 = (int64_t)S->st[1].ascending.size();
    if (sup_batch_size > 0) { S->st[0].share = sup_batch_size / 2; S->st[1].share = sup_batch_size - sup_batch_size / 2; }
    else S->st[0].share = S->st[1].share = (int32_t)std::min(n0, n1);
    for (int c = 0; c < 2; ++c) {
      const int64_t have = (int64_t)S->st[c].ascending.size();
      if (have == 0) return "batch sampler: class " + std::to_string(c) + " of the batch has no row";
      if (have < S->st[c].share)
        return "batch sampler: class " + std::to_string(c) + " has " + std::to_string(have) + " rows, fewer than its share of a batch, " + std::to_string(S->st[c].share);
    }
  }
  for (MlpBatchStream& c : S->st) { c.s = 0; c.cur = 0; c.visited = c.share <= 0; c.shuffle(0); }
  return std::string();
}
inline std::string mlp_batch_make_uns(int64_t n_paths, int uns_batch_size, uint64_t seed, MlpBatchSampler* S, bool* on) {
  *on = uns_batch_size > 0;
  if (!*on) return std::string();
  if (n_paths > 0x7fffffffll) return "batch sampler: more than 2^31 merge paths";
  if (n_paths < uns_batch_size) return "Error: totalSize must be greater than batchSize";
  MlpBatchStream c;
  c.seed = seed; c.stream = 0; c.share = uns_batch_size;
  for (int64_t p = 0; p < n_paths; ++p) c.ascending.push_back((int32_t)p);
  c.shuffle(0);
  S->by_class = false;
  S->st.push_back(c);
  return std::string();
}

// Both samplers and the draw rule: the unsupervised sampler is asked first, then the supervised one; the draw ends the epoch when
// EITHER does (type/energy_function.hxx:42-49).
struct MlpBatchSamplers {
  bool on_u = false, on_s = false;
  MlpBatchSampler U, S;
  bool draw(std::vector<int32_t>* paths, std::vector<int32_t>* rows) {
    bool end = false;
    if (on_u) end = U.draw(paths) || end;
    if (on_s) end = S.draw(rows) || end;
    return end;
  }
};

// The plan of one mini-batch step: every draw of the step, made ahead (the samplers do not depend on the weights), as ONE block of
// memory.  Per draw: the supervised batch's rows; for the path batch the ascending rows its paths name, the paths as a CSR over
// positions in those rows, and the rows' incidence CSR restricted to the batch.  Arrays start at multiples of 8 bytes.
struct MlpBatchPlan {
  struct Draw {
    size_t s_rows = 0, u_rows = 0, u_offsets = 0, u_members = 0, u_inc_off = 0, u_inc = 0;      // byte offsets
    long long n_s = 0, n_u = 0, P = 0;
  };
  std::vector<uint64_t> words;
  std::vector<Draw> draws;
  bool on_u = false, on_s = false;
  size_t bytes() const { return words.size() * 8; }
  size_t put(const void* src, size_t n_bytes) {
    const size_t at = words.size();
    words.resize(at + (n_bytes + 7) / 8, 0);
    if (n_bytes) memcpy(&words[at], src, n_bytes);
    return at * 8;
  }
  void clear() { words.clear(); draws.clear(); }
  // the views of draw i with the block at `base` (host or device memory)
  MlpBatchView sup(const void* base, size_t i) const {
    MlpBatchView v;
    if (!on_s) return v;
    const char* b = (const char*)base;
    v.rows = (const int32_t*)(b + draws[i].s_rows); v.n = draws[i].n_s;
    return v;
  }
  MlpBatchView uns(const void* base, size_t i) const {
    MlpBatchView v;
    if (!on_u) return v;
    const char* b = (const char*)base;
    const Draw& d = draws[i];
    v.rows = (const int32_t*)(b + d.u_rows); v.n = d.n_u; v.P = d.P;
    v.offsets = (const long long*)(b + d.u_offsets); v.members = (const long long*)(b + d.u_members);
    v.inc_off = (const long long*)(b + d.u_inc_off); v.inc = (const uint32_t*)(b + d.u_inc);
    return v;
  }
};

// Adds one draw to the plan.  in: the path term's input (needed only with a path sampler).
inline void mlp_batch_plan_add(const std::vector<int32_t>& paths, const std::vector<int32_t>& rows, const SshmtInput* in, MlpBatchPlan* plan) {
  MlpBatchPlan::Draw d;
  if (plan->on_s) { d.n_s = (long long)rows.size(); d.s_rows = plan->put(rows.data(), 4 * rows.size()); }
  if (plan->on_u) {
    std::vector<int32_t> named;
    for (int32_t p : paths)
      for (int64_t k = in->offsets[(size_t)p]; k < in->offsets[(size_t)p + 1]; ++k) named.push_back((int32_t)in->members[(size_t)k]);
    std::sort(named.begin(), named.end());
    named.erase(std::unique(named.begin(), named.end()), named.end());
    std::vector<int64_t> off{0}, mem, inc_off;
    std::vector<uint32_t> inc;
    for (int32_t p : paths) {
      for (int64_t k = in->offsets[(size_t)p]; k < in->offsets[(size_t)p + 1]; ++k)
        mem.push_back((int64_t)(std::lower_bound(named.begin(), named.end(), (int32_t)in->members[(size_t)k]) - named.begin()));
      off.push_back((int64_t)mem.size());
    }
    sshmt_incidence(off, mem, (int64_t)named.size(), &inc_off, &inc);
    d.n_u = (long long)named.size(); d.P = (long long)paths.size();
    d.u_rows = plan->put(named.data(), 4 * named.size());
    d.u_offsets = plan->put(off.data(), 8 * off.size());
    d.u_members = plan->put(mem.data(), 8 * mem.size());
    d.u_inc_off = plan->put(inc_off.data(), 8 * inc_off.size());
    d.u_inc = plan->put(inc.data(), 4 * inc.size());
  }
  plan->draws.push_back(d);
}

// The mini-batch step on the host's arithmetic: per draw both terms' gradients by their evaluators' batch_grad, g and the update per
// weight by mlp_backward.hpp's rule.  With host evaluators this is the definition; with device evaluators it is the cross-check
// route (GLIA_HMT_BATCH = step): one batch per evaluation, the gradient read back each time.  place(): where the evaluators find the
// plan -- the host's block itself, or (mlp_batch.hip) its copy on the device.
struct MlpBatchHostStep : MlpBatchStep {
  glia_hmt_batch_opts bo;
  MlpBatchSamplers samplers;
  const SshmtInput* in = nullptr;
  MlpTrainEval *ev = nullptr, *eu = nullptr;      // the supervised and the path term's evaluators (NULL: the term is off)
  MlpBatchPlan plan;
  glia_hmt_batch_timing tm = {};
  std::vector<double> gu, gs;

  // alg/gd.hxx:88-106 (epochs: until a draw ends the epoch) and :110-149 (a number of batches)
  void make_plan() {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<int32_t> paths, rows;
    plan.clear();
    plan.on_u = samplers.on_u; plan.on_s = samplers.on_s;
    if (bo.epochs_per_iteration > 0) {
      for (int ep = 0; ep < bo.epochs_per_iteration; ++ep) {
        bool end;
        do { end = samplers.draw(&paths, &rows); mlp_batch_plan_add(paths, rows, in, &plan); } while (!end);
      }
    } else {
      for (int i = 0; i < bo.batches_per_iteration; ++i) { samplers.draw(&paths, &rows); mlp_batch_plan_add(paths, rows, in, &plan); }
    }
    tm.ms_plan += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    tm.steps += 1; tm.batches += (int64_t)plan.draws.size();
    if (plan.bytes() > tm.plan_bytes) tm.plan_bytes = plan.bytes();
  }
  virtual int place(const void** base) { *base = plan.words.data(); return 0; }
  int run_on_host(const void* base, const MlpStepRule& k, double step, std::vector<double>& w, std::vector<double>& om, std::vector<double>& ov) {
    const size_t d = w.size();
    gu.resize(k.use_u ? d : 0); gs.resize(k.use_s ? d : 0);
    for (size_t i = 0; i < plan.draws.size(); ++i) {
      if (k.use_u) { if (int rc = eu->batch_grad(w.data(), plan.uns(base, i), gu.data())) return rc; }
      if (k.use_s) { if (int rc = ev->batch_grad(w.data(), plan.sup(base, i), gs.data())) return rc; }
      for (size_t p = 0; p < d; ++p) {
        const double g = mlp_energy_grad_elem(k, w[p], k.use_u ? gu[p] : 0.0, k.use_s ? gs[p] : 0.0);
        mlp_update_elem(k.optimizer, step, g, &w[p], &om[p], &ov[p]);
      }
    }
    return 0;
  }
  virtual int run_step(const MlpStepRule& k, double step, std::vector<double>& w, std::vector<double>& om, std::vector<double>& ov) {
    const void* base = nullptr;
    if (int rc = place(&base)) return rc;
    return run_on_host(base, k, step, w, om, ov);
  }
  int run(const MlpStepRule& k, double step, std::vector<double>& w, std::vector<double>& om, std::vector<double>& ov) override {
    const auto t0 = std::chrono::steady_clock::now();
    make_plan();
    const int rc = plan.draws.empty() ? 0 : run_step(k, step, w, om, ov);
    tm.ms_wall += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
  }
};

}  // namespace glia
