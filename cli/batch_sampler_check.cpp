// cli/batch_sampler_check.cpp -- the batch samplers and the plan of a mini-batch step alone (glia_amd/csrc/mlp_batch.hpp),
// without the library and without a GPU: a stand-alone host program that checks the sampler's invariants -- every permutation is a
// permutation, no batch repeats an index, every index is seen once per epoch before the wrap, the wrap reads the head of the OLD
// permutation, a class is reshuffled alone, either sampler ends the epoch -- the plan's lists (rows ascending, every local index in
// range, the incidence lists restricted to the batch) and the error cases, then trains one small case twice on one thread.
//   batch_sampler_check      prints OK and exits 0, or names the failed lines and exits 1
// Built plainly by cli/Makefile; `make batch_sampler_check_san` builds it with -fsanitize=address,undefined for a run on the CPU: the
// index arithmetic of the wrap is where a read out of range would hide.
#include <cstdio>
#include <set>

#include "../glia_amd/csrc/mlp_batch.hpp"

using namespace glia;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "batch_sampler_check: line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static bool is_permutation(std::vector<int32_t> a, const std::vector<int32_t>& of) {
  std::vector<int32_t> b = of;
  std::sort(a.begin(), a.end()); std::sort(b.begin(), b.end());
  return a == b;
}
static bool distinct(const std::vector<int32_t>& a) { return std::set<int32_t>(a.begin(), a.end()).size() == a.size(); }

// n merges over leaves 0 .. n: merge k joins the region merge k - 1 created with leaf k + 1
static std::vector<uint32_t> caterpillar(int n) {
  std::vector<uint32_t> o;
  const uint32_t R = (uint32_t)n + 1;
  for (uint32_t k = 0; k < (uint32_t)n; ++k) { o.push_back(k ? R + k - 1 : 0); o.push_back(k + 1); o.push_back(R + k); }
  return o;
}

static void check_uniform(int n, int B, uint64_t seed) {
  std::vector<int32_t> lab((size_t)n, 1), base, p0, p1, out, seen;
  for (int i = 0; i < n; ++i) base.push_back(i);
  MlpBatchSampler S;
  bool on = false;
  EXPECT(mlp_batch_make_sup(lab.data(), n, B, 0, 0.05, 0.95, seed, &S, &on).empty() && on && S.batch_size() == B);
  mlp_batch_perm(seed, 1, 0, base, &p0); mlp_batch_perm(seed, 1, 1, base, &p1);
  EXPECT(is_permutation(p0, base) && is_permutation(p1, base));
  const int draws = (n + B - 1) / B;      // the draw that reaches the end
  for (int i = 0; i < draws; ++i) {
    const bool end = S.draw(&out);
    EXPECT((int)out.size() == B && distinct(out) && end == (i == draws - 1));
    seen.insert(seen.end(), out.begin(), out.end());
  }
  // permutation 0, then its head again
  for (size_t i = 0; i < seen.size(); ++i) EXPECT(seen[i] == p0[i % (size_t)n]);
  S.draw(&out);
  for (int i = 0; i < B; ++i) EXPECT(out[(size_t)i] == p1[(size_t)i % (size_t)n]);
}

static void check_classes(int n_pos, int n_neg, int B, int balance_only, uint64_t seed) {
  std::vector<int32_t> lab, out;
  for (int i = 0; i < n_pos + n_neg; ++i) lab.push_back(i % (n_pos + n_neg) < n_pos ? 1 : -1);
  MlpBatchSampler S;
  bool on = false;
  EXPECT(mlp_batch_make_sup(lab.data(), (int64_t)lab.size(), balance_only ? -1 : B, 1, 0.05, 0.95, seed, &S, &on).empty() && on);
  const int64_t share0 = S.st[0].share, share1 = S.st[1].share;
  EXPECT(balance_only ? share0 == std::min(n_pos, n_neg) && share1 == share0 : share0 == B / 2 && share1 == B - B / 2);
  int ends = 0;
  for (int i = 0; i < 200; ++i) {
    const uint64_t s0 = S.st[0].s, s1 = S.st[1].s;
    const bool end = S.draw(&out);
    EXPECT((int64_t)out.size() == share0 + share1 && distinct(out));
    for (int64_t k = 0; k < share0 + share1; ++k) EXPECT(out[(size_t)k] >= 0 && out[(size_t)k] < n_pos + n_neg && (lab[(size_t)out[(size_t)k]] == 1) == (k < share0));
    EXPECT(S.st[0].s >= s0 && S.st[1].s >= s1 && S.st[0].cur < S.st[0].all.size() && S.st[1].cur < S.st[1].all.size());
    if (end) { EXPECT(S.st[0].s > s0 && S.st[1].s > s1 && S.st[0].cur == 0 && S.st[1].cur == 0); ++ends; }
  }
  EXPECT(ends >= 1);
}

int main() {
  for (int n : {1, 2, 3, 10, 64, 65, 1000})
    for (int B : {1, 2, 3, 7, 64, 65, 1000})
      if (B <= n) check_uniform(n, B, (uint64_t)(n * 131 + B));
  check_classes(7, 13, 6, 0, 4);
  check_classes(7, 13, 0, 1, 5);
  check_classes(13, 7, 1, 0, 6);      // a class whose share is 0
  check_classes(3, 3, 6, 0, 7);       // every batch wraps both classes
  check_classes(50, 2, 4, 0, 8);

  // the errors: messages, no sampler built
  {
    std::vector<int32_t> lab{1, 1, -1, -1, -1};
    MlpBatchSampler S;
    bool on = false;
    EXPECT(mlp_batch_make_sup(lab.data(), 5, 6, 0, 0.05, 0.95, 0, &S, &on) == "Error: totalSize must be greater than batchSize");
    EXPECT(mlp_batch_make_uns(4, 5, 0, &S, &on) == "Error: totalSize must be greater than batchSize");
    MlpBatchSampler S2, S3, S4, S5;
    EXPECT(mlp_batch_make_sup(lab.data(), 5, 6, 1, 0.05, 0.95, 0, &S2, &on).find("class 0 has 2 rows, fewer than its share") != std::string::npos);
    EXPECT(mlp_batch_make_sup(lab.data(), 2, 2, 1, 0.05, 0.95, 0, &S3, &on).find("class 1 of the batch has no row") != std::string::npos);
    EXPECT(mlp_batch_make_sup(lab.data(), 5, -1, 1, 0.5, 0.5, 0, &S4, &on).find("one class") != std::string::npos);
    EXPECT(mlp_batch_make_sup(lab.data(), 5, -1, 0, 0.05, 0.95, 0, &S5, &on).empty() && !on);
  }

  // the plan over the paths of two caterpillars: every list in range, the named rows ascending, the incidence restricted to the batch
  SshmtInput in;
  const int dim = 4, D = dim + 1;
  in.D = D;
  sshmt_fill_tables(0.95, 1.0, &in.tb);
  for (int b = 0; b < 2; ++b) {
    const std::vector<uint32_t> o = caterpillar(40);
    merge_paths(o.data(), 40, 3, 2, in.n_rows, &in.offsets, &in.members);
    for (int r = 0; r < 40; ++r) {
      for (int j = 0; j < dim; ++j) in.X.push_back((double)((5 * (r + 40 * b) + 11 * j) % 19 - 9) / 9.0);
      in.X.push_back(1.0);
    }
    in.n_rows += 40;
  }
  sshmt_incidence(in.offsets, in.members, in.n_rows, &in.inc_off, &in.inc);
  EXPECT(in.n_paths() == 76);
  std::vector<double> rows;
  std::vector<int32_t> labels;
  for (int r = 0; r < 150; ++r) {
    for (int j = 0; j < dim; ++j) rows.push_back((double)((7 * r + 13 * j) % 17 - 8) / 8.0);
    labels.push_back((5 * r) % 7 < 3 ? 1 : -1);
  }
  std::vector<double> X, t;
  mlp_train_prepare(rows.data(), 150, dim, labels.data(), nullptr, nullptr, 0.05, 0.95, &X, &t);

  auto make_step = [&](MlpBatchHostStep* st, MlpTrainHostEval* hs, SshmtHostEval* hu, int te, int tb) {
    glia_hmt_batch_opts bo;
    bo.seed = 3; bo.epochs_per_iteration = te; bo.batches_per_iteration = tb;
    st->bo = bo; st->in = &in;
    EXPECT(mlp_batch_make_uns(in.n_paths(), 70, bo.seed, &st->samplers.U, &st->samplers.on_u).empty());
    EXPECT(mlp_batch_make_sup(labels.data(), 150, 70, 0, 0.05, 0.95, bo.seed, &st->samplers.S, &st->samplers.on_s).empty());
    hs->D = D; hs->n1 = 3; hs->n2 = 3; hs->X = X.data(); hs->t = t.data(); hs->n = 150;
    hu->n1 = 3; hu->n2 = 3; hu->in = &in;
    st->ev = hs; st->eu = hu;
  };
  {
    MlpBatchHostStep st;
    MlpTrainHostEval hs;
    SshmtHostEval hu;
    make_step(&st, &hs, &hu, 2, 1);
    for (int step = 0; step < 5; ++step) {
      st.make_plan();
      EXPECT(!st.plan.draws.empty() && st.plan.draws.size() <= 4);
      for (size_t i = 0; i < st.plan.draws.size(); ++i) {
        const MlpBatchView s = st.plan.sup(st.plan.words.data(), i), u = st.plan.uns(st.plan.words.data(), i);
        EXPECT(s.n == 70 && u.P == 70 && u.n >= 70 && u.n <= 80 && u.offsets[0] == 0 && u.inc_off[0] == 0 && u.inc_off[u.n] == u.offsets[u.P]);
        for (long long k = 0; k < s.n; ++k) EXPECT(s.rows[k] >= 0 && s.rows[k] < 150);
        for (long long k = 0; k < u.n; ++k) EXPECT(u.rows[k] >= 0 && u.rows[k] < 80 && (k == 0 || u.rows[k - 1] < u.rows[k]));
        for (long long k = 0; k < u.offsets[u.P]; ++k) EXPECT(u.members[k] >= 0 && u.members[k] < u.n && u.inc[k] / kSshmtMaxPath < (uint32_t)u.P);
        for (long long r = 0; r < u.n; ++r)
          for (long long k = u.inc_off[r]; k < u.inc_off[r + 1]; ++k) {
            EXPECT(u.members[u.offsets[u.inc[k] / kSshmtMaxPath] + u.inc[k] % kSshmtMaxPath] == r);      // the pair names the row
            EXPECT(k == u.inc_off[r] || u.inc[k - 1] < u.inc[k]);                                        // ascending batch position
          }
        // the full incidence list of a named row is at least as long as the restricted one, and longer for some row (6 paths are outside)
        long long shorter = 0;
        for (long long r = 0; r < u.n; ++r) {
          const long long full = in.inc_off[(size_t)u.rows[r] + 1] - in.inc_off[(size_t)u.rows[r]], part = u.inc_off[r + 1] - u.inc_off[r];
          EXPECT(part >= 1 && part <= full);
          shorter += part < full;
        }
        EXPECT(shorter >= 1);
      }
    }
  }
  // a small case trained twice: the same bits, and not the full-batch trainer's
  std::vector<double> w_run[3];
  for (int run = 0; run < 3; ++run) {
    MlpBatchHostStep st;
    MlpTrainHostEval hs;
    SshmtHostEval hu;
    make_step(&st, &hs, &hu, 1, 1);
    glia_hmt_mlp_train_opts o;
    mlp_train_opts_default(&o);
    o.n1 = o.n2 = 3; o.ws = 1.0; o.wr = 0.01; o.sigma_s = 0.5; o.step = 0.05; o.optimizer = 2; o.max_iterations = 3; o.n_sigma_updates = 2;
    std::vector<double> w((size_t)mlp_train_n_weights(D, 3, 3));
    for (size_t p = 0; p < w.size(); ++p) w[p] = mlp_init_weight(1, p);
    MlpTrainResult R;
    MlpTrainUns U;
    U.ev = &hu; U.n_paths = in.n_paths(); U.n_rows = in.n_rows; U.wu = 0.5; U.sigma_u = 0.7;
    EXPECT(mlp_train_run(o, 150, w, &hs, &R, &U, run < 2 ? &st : nullptr) == 0);
    EXPECT(R.round_w.size() == 2 && !R.stopped_nonfinite);
    if (run < 2) EXPECT(st.tm.steps == 6 && st.tm.batches > st.tm.steps);
    w_run[run] = w;
  }
  EXPECT(w_run[0] == w_run[1] && w_run[0] != w_run[2]);
  if (fails) return 1;
  printf("OK\n");
  return 0;
}
