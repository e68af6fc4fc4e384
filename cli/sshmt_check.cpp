// cli/sshmt_check.cpp -- the definition of the merge-path (unsupervised) term alone (glia_amd/csrc/sshmt_paths.hpp), without the library
// and without a GPU: a stand-alone host program that lists the merge paths of fixed orders, trains fixed small cases on one thread with
// the term on, checks what can be checked without a second author (known paths, two runs agree, a_i = dD/df_i against a central
// difference of D, the refusals) and prints one digest per case -- FNV-1a over the bits of the weights after every round, of the trace
// and of the sigma_u series -- which tests/test_sshmt_tools.py compares with the second author's.
//   sshmt_check      prints the digests and OK and exits 0, or names the failed lines and exits 1
// Built plainly by cli/Makefile; `make sshmt_check_san` builds it with -fsanitize=address,undefined for a run on the CPU.
#include <cstdio>
#include <cstring>

#include "../glia_amd/csrc/sshmt_paths.hpp"

using namespace glia;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "sshmt_check: line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static uint64_t fnv(uint64_t h, const void* p, size_t n) {
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 0x100000001B3ull; }
  return h;
}

// the fixed inputs of mlp_train_check: rows[r][j] = ((7 r + 13 j) mod 17 - 8) / 8, label +1 / -1 / 0 by (5 r) mod 7 (0: dropped)
static void fixed_rows(int n, int dim, std::vector<double>* rows, std::vector<int32_t>* labels) {
  rows->resize((size_t)n * dim); labels->resize(n);
  for (int r = 0; r < n; ++r) {
    for (int j = 0; j < dim; ++j) (*rows)[(size_t)r * dim + j] = (double)((7 * r + 13 * j) % 17 - 8) / 8.0;
    const int m = (5 * r) % 7;
    (*labels)[r] = m < 3 ? 1 : (m < 6 ? -1 : 0);
  }
}
// unlabelled rows: rows[r][j] = ((5 r + 11 j) mod 19 - 9) / 9
static void fixed_uns_rows(int n, int dim, std::vector<double>* rows) {
  rows->resize((size_t)n * dim);
  for (int r = 0; r < n; ++r) for (int j = 0; j < dim; ++j) (*rows)[(size_t)r * dim + j] = (double)((5 * r + 11 * j) % 19 - 9) / 9.0;
}
// n merges over leaves 0 .. n: merge k joins the region merge k - 1 created with leaf k + 1
static std::vector<uint32_t> caterpillar(int n) {
  std::vector<uint32_t> o;
  const uint32_t R = (uint32_t)n + 1;
  for (uint32_t k = 0; k < (uint32_t)n; ++k) { o.push_back(k ? R + k - 1 : 0); o.push_back(k + 1); o.push_back(R + k); }
  return o;
}
// 2^levels leaves merged level by level
static std::vector<uint32_t> balanced(int levels) {
  std::vector<uint32_t> o, live;
  uint32_t next = 1u << levels;
  for (uint32_t i = 0; i < next; ++i) live.push_back(i);
  while (live.size() > 1) {
    std::vector<uint32_t> up;
    for (size_t i = 0; i < live.size(); i += 2) { o.push_back(live[i]); o.push_back(live[i + 1]); o.push_back(next); up.push_back(next++); }
    live = up;
  }
  return o;
}

struct Case { const char* name; int n, dim, n1, n2, optimizer; double step, decay; int usu, tree, max_len, min_len; double ws; };

static uint64_t run_case(const Case& c, MlpTrainResult* R) {
  std::vector<double> rows, urows, X, t;
  std::vector<int32_t> labels;
  fixed_rows(c.n, c.dim, &rows, &labels);
  glia_hmt_sshmt_train_opts so;
  sshmt_train_opts_default(&so);
  glia_hmt_mlp_train_opts& o = so.base;
  o.n1 = c.n1; o.n2 = c.n2; o.wr = 0.01; o.ws = c.ws; o.sigma_s = 0.5; o.optimizer = c.optimizer; o.step = c.step; o.wu = 0.5; so.sigma_u = 0.7;
  o.update_sigma_u = c.usu; o.step_decay = c.decay; o.max_iterations = 4; o.n_sigma_updates = 2; o.seed = 3; o.fixed_step_decay_iterations = 2;
  so.max_path_length = c.max_len; so.min_path_length = c.min_len;
  EXPECT(sshmt_train_bad_opts(so).empty() && mlp_train_unsupported(o, true).empty() && !mlp_train_unsupported(o).empty());
  EXPECT(sshmt_bad_lengths(c.max_len, c.min_len).empty());
  mlp_train_prepare(rows.data(), c.n, c.dim, labels.data(), nullptr, nullptr, o.pos_target, o.neg_target, &X, &t);
  const std::vector<uint32_t> order = c.tree ? balanced(c.tree) : caterpillar(67);
  const int64_t nm = (int64_t)order.size() / 3;
  EXPECT(sshmt_check_order(order.data(), nm) == -1);
  fixed_uns_rows((int)nm, c.dim, &urows);
  SshmtInput in;
  in.D = c.dim + 1; in.n_rows = nm;
  sshmt_fill_tables(so.merge_target, so.path_target, &in.tb);
  merge_paths(order.data(), nm, c.max_len, c.min_len, 0, &in.offsets, &in.members);
  for (int64_t r = 0; r < nm; ++r) { for (int j = 0; j < c.dim; ++j) in.X.push_back(urows[(size_t)r * c.dim + j]); in.X.push_back(1.0); }
  sshmt_incidence(in.offsets, in.members, in.n_rows, &in.inc_off, &in.inc);
  const int D = c.dim + 1;
  std::vector<double> w((size_t)mlp_train_n_weights(D, c.n1, c.n2), 0.0);
  for (size_t p = 0; p < w.size() && c.n1; ++p) w[p] = mlp_init_weight(o.seed, p);
  MlpTrainHostEval ev;
  ev.D = D; ev.n1 = c.n1; ev.n2 = c.n2; ev.X = X.data(); ev.t = t.data(); ev.n = (int64_t)t.size();
  SshmtHostEval eu;
  eu.n1 = c.n1; eu.n2 = c.n2; eu.in = &in;
  MlpTrainUns U;
  U.ev = &eu; U.n_paths = in.n_paths(); U.n_rows = in.n_rows; U.wu = o.wu; U.sigma_u = so.sigma_u; U.min_sigma2 = o.min_sigma2; U.update_sigma_u = o.update_sigma_u;
  R->D = D; R->n1 = c.n1; R->n2 = c.n2; R->n_used = ev.n; R->n_paths = U.n_paths; R->n_uns_rows = U.n_rows;
  EXPECT(mlp_train_run(o, ev.n, w, &ev, R, &U) == 0);
  uint64_t h = 0xCBF29CE484222325ull;
  for (const auto& rw : R->round_w) h = fnv(h, rw.data(), sizeof(double) * rw.size());
  for (const auto& r : R->trace) { const double f[5] = {r.fx, r.xnorm, r.gnorm, r.step, r.sigma2}; h = fnv(h, f, sizeof(f)); }
  h = fnv(h, R->sigma_u2.data(), sizeof(double) * R->sigma_u2.size());
  h = fnv(h, R->sigma_u2_eval.data(), sizeof(double) * R->sigma_u2_eval.size());
  return h;
}

int main() {
  // known paths (hmt/tree_build.hxx:150-180 on this order prints the same)
  {
    const uint32_t order[] = {1, 2, 7, 3, 4, 8, 7, 8, 9, 5, 6, 10, 9, 10, 11};
    std::vector<int64_t> off, mem;
    merge_paths(order, 5, 3, 2, 0, &off, &mem);
    const std::vector<int64_t> want_off = {0, 3, 6, 8}, want_mem = {0, 2, 4, 1, 2, 4, 3, 4};
    EXPECT(off == want_off && mem == want_mem);
    EXPECT(sshmt_check_order(order, 5) == -1);
    off.clear(); mem.clear();
    merge_paths(order, 5, 1, 1, 100, &off, &mem);
    EXPECT(off.size() == 6 && mem.size() == 5 && mem[0] == 100 && mem[4] == 104);
    std::vector<int64_t> inc_off;
    std::vector<uint32_t> inc;
    sshmt_incidence(want_off, want_mem, 5, &inc_off, &inc);
    const std::vector<int64_t> want_inc_off = {0, 1, 2, 4, 5, 8};
    const std::vector<uint32_t> want_inc = {0, 8, 1, 9, 16, 2, 10, 17};
    EXPECT(inc_off == want_inc_off && inc == want_inc);
    const uint32_t twice[] = {1, 2, 7, 1, 3, 8}, late[] = {7, 3, 8, 1, 2, 7}, reused[] = {1, 2, 7, 3, 4, 7}, self[] = {1, 1, 7};
    EXPECT(sshmt_check_order(twice, 2) == 1 && sshmt_check_order(late, 2) == 0 && sshmt_check_order(reused, 2) == 1 && sshmt_check_order(self, 1) == 0);
    EXPECT(!sshmt_bad_lengths(-1, 2).empty() && !sshmt_bad_lengths(9, 2).empty() && !sshmt_bad_lengths(3, 0).empty() && !sshmt_bad_lengths(3, 4).empty());
    EXPECT(sshmt_bad_lengths(8, 8).empty() && sshmt_bad_lengths(1, 1).empty());
  }
  // a_i = dD/df_i against a central difference of D = t - e, n = 1 .. 8
  {
    SshmtTables tb;
    sshmt_fill_tables(0.95, 1.0, &tb);
    double worst = 0.0;
    for (int n = 1; n <= kSshmtMaxPath; ++n) {
      double f[kSshmtMaxPath], q[kSshmtMaxPath];
      for (int i = 0; i < n; ++i) f[i] = 0.15 + 0.09 * i;
      const double e = sshmt_path(f, n, tb.T[n], tb.t[n], q);
      const double e2 = sshmt_path(f, n, tb.T[n], tb.t[n], nullptr);
      EXPECT(memcmp(&e, &e2, sizeof(e)) == 0);
      for (int i = 0; i < n; ++i) {
        const double h = 1e-6, keep = f[i];
        f[i] = keep + h; const double ep = sshmt_path(f, n, tb.T[n], tb.t[n], nullptr);
        f[i] = keep - h; const double em = sshmt_path(f, n, tb.T[n], tb.t[n], nullptr);
        f[i] = keep;
        const double a = q[i] / e, fd = -(ep - em) / (2.0 * h);      // D = t - e
        worst = std::max(worst, std::fabs(a - fd));
      }
    }
    EXPECT(worst < 1e-8);
  }
  static const Case cases[] = {
      {"mlp_3_5_vanilla_fixed_cat", 70, 4, 3, 5, 1, 0.05, 1.0, 0, 0, 3, 2, 1.0}, {"mlp_3_5_adam_adaptive_bal", 70, 4, 3, 5, 2, 0.5, 0.5, 1, 5, 3, 2, 1.0},
      {"mlp_1_1_momentum_len8", 130, 1, 1, 1, 3, 0.05, 1.0, 0, 0, 8, 2, 1.0},    {"logsig_vanilla_adaptive_len1", 65, 6, 0, 0, 1, 100.0, 0.25, 0, 4, 1, 1, 1.0},
      {"mlp_32_32_adam_wu_alone", 9, 12, 32, 32, 2, 0.01, 1.0, 1, 6, 2, 1, 0.0},
  };
  for (const Case& c : cases) {
    MlpTrainResult a, b;
    const uint64_t ha = run_case(c, &a), hb = run_case(c, &b);
    EXPECT(ha == hb && a.round_w.size() == 2 && !a.stopped_nonfinite && a.sigma_u2.size() == 3 && a.sigma2.size() == 3);
    EXPECT(a.n_paths > 0 && a.n_uns_rows > 0);
    printf("sshmt_check: %s %016llx\n", c.name, (unsigned long long)ha);
  }
  // refusals
  {
    glia_hmt_sshmt_train_opts so;
    sshmt_train_opts_default(&so);
    EXPECT(so.max_path_length == 3 && so.min_path_length == 2 && so.merge_target == 0.95 && so.path_target == 1.0 && so.sigma_u == 0.0);
    EXPECT(sshmt_train_bad_opts(so).find("all 0") != std::string::npos);
    so.base.wu = 1.0; EXPECT(sshmt_train_bad_opts(so).find("sigma_u") != std::string::npos);
    so.base.update_sigma_u = 1; EXPECT(sshmt_train_bad_opts(so).empty());
    so.base.uns_batch_size = 4; EXPECT(mlp_train_unsupported(so.base, true).find("uns_batch_size") != std::string::npos);
  }
  if (fails) { fprintf(stderr, "sshmt_check: %d checks failed\n", fails); return 1; }
  printf("sshmt_check: OK\n");
  return 0;
}
