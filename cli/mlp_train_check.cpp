// cli/mlp_train_check.cpp -- the definition of the MLP / logsig trainer alone (glia_amd/csrc/mlp_backward.hpp), without the library
// and without a GPU: a stand-alone host program that trains fixed small cases on one thread, checks what can be checked without a
// second author (two runs agree, the analytic gradient agrees with loops written out here, the refusals) and prints one digest per
// case -- FNV-1a over the bits of the weights after every round and of the trace -- which tests/test_mlp_train_tools.py compares with
// the second author's.
//   mlp_train_check      prints the digests and OK and exits 0, or names the failed lines and exits 1
// Built plainly by cli/Makefile; `make mlp_train_check_san` builds it with -fsanitize=address,undefined for a run on the CPU.
#include <cstdio>
#include <cstring>

#include "../glia_amd/csrc/mlp_backward.hpp"

using namespace glia;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "mlp_train_check: line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static uint64_t fnv(uint64_t h, const void* p, size_t n) {
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 0x100000001B3ull; }
  return h;
}
static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof(a)) == 0; }

// the fixed inputs: rows[r][j] = ((7 r + 13 j) mod 17 - 8) / 8, label +1 / -1 / 0 by (5 r) mod 7 (0: dropped)
static void fixed_rows(int n, int dim, std::vector<double>* rows, std::vector<int32_t>* labels) {
  rows->resize((size_t)n * dim); labels->resize(n);
  for (int r = 0; r < n; ++r) {
    for (int j = 0; j < dim; ++j) (*rows)[(size_t)r * dim + j] = (double)((7 * r + 13 * j) % 17 - 8) / 8.0;
    const int m = (5 * r) % 7;
    (*labels)[r] = m < 3 ? 1 : (m < 6 ? -1 : 0);
  }
}

struct Case { const char* name; int n, dim, n1, n2, optimizer; double step, decay; int uss; };

static uint64_t run_case(const Case& c, MlpTrainResult* R) {
  std::vector<double> rows, X, t;
  std::vector<int32_t> labels;
  fixed_rows(c.n, c.dim, &rows, &labels);
  glia_hmt_mlp_train_opts o;
  mlp_train_opts_default(&o);
  o.n1 = c.n1; o.n2 = c.n2; o.wr = 0.01; o.ws = 1.0; o.sigma_s = 0.5; o.update_sigma_s = c.uss; o.optimizer = c.optimizer; o.step = c.step;
  o.step_decay = c.decay; o.max_iterations = 4; o.n_sigma_updates = 2; o.seed = 3; o.fixed_step_decay_iterations = 2;
  EXPECT(mlp_train_bad_opts(o).empty() && mlp_train_unsupported(o).empty());
  mlp_train_prepare(rows.data(), c.n, c.dim, labels.data(), nullptr, nullptr, o.pos_target, o.neg_target, &X, &t);
  const int D = c.dim + 1;
  std::vector<double> w((size_t)mlp_train_n_weights(D, c.n1, c.n2), 0.0);
  for (size_t p = 0; p < w.size() && c.n1; ++p) w[p] = mlp_init_weight(o.seed, p);
  MlpTrainHostEval ev;
  ev.D = D; ev.n1 = c.n1; ev.n2 = c.n2; ev.X = X.data(); ev.t = t.data(); ev.n = (int64_t)t.size();
  R->D = D; R->n1 = c.n1; R->n2 = c.n2; R->n_used = ev.n;
  EXPECT(mlp_train_run(o, ev.n, w, &ev, R) == 0);
  uint64_t h = 0xCBF29CE484222325ull;
  for (const auto& rw : R->round_w) h = fnv(h, rw.data(), sizeof(double) * rw.size());
  for (const auto& r : R->trace) { const double f[5] = {r.fx, r.xnorm, r.gnorm, r.step, r.sigma2}; h = fnv(h, f, sizeof(f)); }
  return h;
}

// the gradient of one weight, written out once more for a logsig model: rows in, -sum g e out, in the two-level order
static double logsig_grad_elem(const std::vector<double>& w, const std::vector<double>& X, const std::vector<double>& t, int D, int p) {
  double grad = 0.0;
  const int n = (int)t.size();
  for (int r0 = 0; r0 < n; r0 += 64) {
    double S = 0.0;
    for (int r = r0; r < n && r < r0 + 64; ++r) {
      double h = 0.0;
      for (int j = 0; j < D; ++j) { const double q = X[(size_t)r * D + j] * w[j]; h = h + q; }
      const double f = 1.0 / (1.0 + std::exp(-h));
      const double e = t[r] - f;
      if (std::fabs(e) < 2.22e-16) continue;
      const double one = 1.0 - f, dh3 = f * one, g = dh3 * X[(size_t)r * D + p], ge = g * e;
      S = S - ge;
    }
    grad = grad + S;
  }
  return grad;
}

int main() {
  static const Case cases[] = {
      {"mlp_3_5_vanilla_fixed", 70, 4, 3, 5, 1, 0.05, 1.0, 0},  {"mlp_3_5_adam_adaptive", 70, 4, 3, 5, 2, 0.5, 0.5, 1},
      {"mlp_1_1_momentum", 130, 1, 1, 1, 3, 0.05, 1.0, 0},      {"logsig_vanilla_adaptive", 65, 6, 0, 0, 1, 100.0, 0.25, 0},
      {"mlp_32_32_adam", 9, 12, 32, 32, 2, 0.01, 1.0, 1},
  };
  for (const Case& c : cases) {
    MlpTrainResult a, b;
    const uint64_t ha = run_case(c, &a), hb = run_case(c, &b);
    EXPECT(ha == hb && a.round_w.size() == 2 && !a.stopped_nonfinite && a.sigma2.size() == 3);
    EXPECT(a.n_used > 0 && a.n_used < c.n);
    printf("mlp_train_check: %s %016llx\n", c.name, (unsigned long long)ha);
  }
  // the chunked gradient of a logsig model against loops written here
  {
    std::vector<double> rows, X, t;
    std::vector<int32_t> labels;
    fixed_rows(130, 5, &rows, &labels);
    mlp_train_prepare(rows.data(), 130, 5, labels.data(), nullptr, nullptr, 0.05, 0.95, &X, &t);
    std::vector<double> w = {0.3, -0.2, 0.1, 0.05, -0.4, 0.02}, g(6);
    double L = 0.0;
    mlp_loss_grad_host(w.data(), 6, 0, 0, X.data(), t.data(), (int64_t)t.size(), &L, g.data());
    for (int p = 0; p < 6; ++p) EXPECT(same_bits(g[p], logsig_grad_elem(w, X, t, 6, p)));
    double L2 = 0.0;
    mlp_loss_grad_host(w.data(), 6, 0, 0, X.data(), t.data(), (int64_t)t.size(), &L2, nullptr);
    EXPECT(same_bits(L, L2) && L > 0.0);
    EXPECT(t.size() == 112);
  }
  // the initial weights: no libm, bounded, centred
  {
    double s = 0.0, s2 = 0.0;
    for (uint64_t p = 0; p < 20000; ++p) { const double v = mlp_init_weight(0, p); s += v; s2 += v * v; EXPECT(std::fabs(v) <= 0.06); }
    EXPECT(std::fabs(s / 20000.0) < 3e-4 && std::fabs(std::sqrt(s2 / 20000.0) - 0.01) < 3e-4);
    EXPECT(!same_bits(mlp_init_weight(0, 1), mlp_init_weight(1, 1)) && !same_bits(mlp_init_weight(0, 1), mlp_init_weight(0, 2)));
  }
  // refusals
  {
    glia_hmt_mlp_train_opts o;
    mlp_train_opts_default(&o);
    EXPECT(mlp_train_bad_opts(o).find("both 0") != std::string::npos);
    o.ws = 1.0; EXPECT(mlp_train_bad_opts(o).find("sigma_s") != std::string::npos);
    o.update_sigma_s = 1; EXPECT(mlp_train_bad_opts(o).empty());
    o.n2 = 0; EXPECT(mlp_train_bad_opts(o).find("logsig") != std::string::npos);
    o.n2 = 33; EXPECT(mlp_train_bad_opts(o).empty() && mlp_train_unsupported(o).find("32") != std::string::npos);
    o.n2 = 10; o.wu = 1.0; EXPECT(mlp_train_unsupported(o).find("wu") != std::string::npos);
  }
  if (fails) { fprintf(stderr, "mlp_train_check: %d checks failed\n", fails); return 1; }
  printf("mlp_train_check: OK\n");
  return 0;
}
