// cli/mlp_model_check.cpp -- the host side of the MLP / logsig predictors alone, without the library and without a GPU: the parser of
// model and min/max files on good and bad files, the shape arithmetic, the kernel's layout helpers, and the forward pass of
// glia_amd/csrc/mlp_model.hpp against a literal triple loop written here.
//   mlp_model_check      prints OK and exits 0, or names the failed lines and exits 1
// Built plainly by cli/Makefile; `make mlp_model_check_san` builds it with -fsanitize=address,undefined for a run on the CPU.
#include <unistd.h>

#include <cstring>
#include <limits>

#include "../glia_amd/csrc/mlp_model.hpp"

using namespace glia;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "mlp_model_check: line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static std::string tmpdir;
static std::string write_file(const char* name, const std::string& text) {
  const std::string path = tmpdir + "/" + name;
  FILE* f = fopen(path.c_str(), "wb");
  if (f) { fwrite(text.data(), 1, text.size(), f); fclose(f); }
  return path;
}
static bool same_bits(double a, double b) { return (a != a && b != b) || memcmp(&a, &b, sizeof(a)) == 0; }

// a small deterministic generator (values in [-1, 1) with a few exact ties)
static uint64_t rng_state = 0x243F6A8885A308D3ull;
static double rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(int64_t)(rng_state >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}

// the definition, written out once more: rows in, logits out
static void triple_loop(const HostMlp& m, const double* rows, int n, double* logit) {
  const int D = m.D, N1 = m.n1, N2 = m.n2;
  for (int r = 0; r < n; ++r) {
    std::vector<double> x(D);
    for (int j = 0; j < D - 1; ++j) {
      double v = rows[(size_t)r * (D - 1) + j];
      if (m.rescale) { const double num = 2.0 * (v - m.mn[j]); const double den = (m.mx[j] - m.mn[j]) + 2.22e-16; v = num / den; v = v + (-1.0); }
      x[j] = v;
    }
    x[D - 1] = 1.0;
    int pick = 0;
    if (m.n_models == 3) pick = x[m.dim1] < m.threshold ? 0 : x[m.dim0] < m.threshold ? 1 : 2;
    const std::vector<double>& w = m.w[pick];
    double h3 = 0.0;
    if (N1 == 0) {
      for (int j = 0; j < D; ++j) { const double p = x[j] * w[j]; h3 = h3 + p; }
    } else {
      std::vector<double> a1(N1 + 1, 1.0), a2(N2 + 1, 1.0);
      for (int k = 0; k < N1; ++k) {
        double h = 0.0;
        for (int j = 0; j < D; ++j) { const double p = x[j] * w[j + (size_t)D * k]; h = h + p; }
        a1[k] = h > 0.0 ? h : 0.0;
      }
      const size_t o1 = (size_t)D * N1, o2 = o1 + (size_t)(N1 + 1) * N2;
      for (int k = 0; k < N2; ++k) {
        double h = 0.0;
        for (int j = 0; j <= N1; ++j) { const double p = a1[j] * w[o1 + j + (size_t)(N1 + 1) * k]; h = h + p; }
        a2[k] = h > 0.0 ? h : 0.0;
      }
      for (int j = 0; j <= N2; ++j) { const double p = a2[j] * w[o2 + j]; h3 = h3 + p; }
    }
    logit[r] = h3;
  }
}

static HostMlp random_model(int n_models, int dim, int n1, int n2, bool rescale) {
  HostMlp m;
  m.n_models = n_models; m.n1 = n1; m.n2 = n2; m.D = dim + 1;
  const size_t W = n1 ? (size_t)m.D * n1 + (size_t)(n1 + 1) * n2 + n2 + 1 : (size_t)m.D;
  for (int i = 0; i < n_models; ++i) { m.w[i].resize(W); for (double& v : m.w[i]) v = rnd(); }
  if (rescale) {
    m.rescale = true;
    m.mn.resize(dim); m.mx.resize(dim);
    for (int j = 0; j < dim; ++j) { m.mn[j] = rnd() - 1.0; m.mx[j] = m.mn[j] + (j % 5 == 0 ? 0.0 : rnd() + 1.5); }
  }
  if (n_models == 3) { m.dim0 = 0; m.dim1 = dim; m.threshold = 0.1; if (dim > 1) m.dim1 = 1; }
  return m;
}

static void check_forward(int n_models, int dim, int n1, int n2, bool rescale) {
  const HostMlp m = random_model(n_models, dim, n1, n2, rescale);
  EXPECT(mlp_check(m).empty());
  const int n = 37;
  std::vector<double> rows((size_t)n * dim);
  for (double& v : rows) v = rnd() * 2.0;
  rows[0] = std::numeric_limits<double>::quiet_NaN();
  if (rows.size() > 3) { rows[1] = std::numeric_limits<double>::infinity(); rows[2] = -0.0; rows[3] = -std::numeric_limits<double>::infinity(); }
  std::vector<double> want(n), logit(n), pred(n);
  triple_loop(m, rows.data(), n, want.data());
  mlp_forward(m, rows.data(), n, dim, pred.data(), logit.data());
  for (int r = 0; r < n; ++r) {
    EXPECT(same_bits(want[r], logit[r]));
    EXPECT(same_bits(pred[r], 1.0 / (1.0 + std::exp(-want[r]))));
  }
  // a padded stride, one output only
  std::vector<double> padded((size_t)n * (dim + 3), std::numeric_limits<double>::quiet_NaN()), l2(n);
  for (int r = 0; r < n; ++r) memcpy(&padded[(size_t)r * (dim + 3)], &rows[(size_t)r * dim], sizeof(double) * dim);
  mlp_forward(m, padded.data(), n, dim + 3, nullptr, l2.data());
  for (int r = 0; r < n; ++r) EXPECT(same_bits(l2[r], logit[r]));
  // the blocked layout holds every weight once, zeros elsewhere
  if (n1) {
    const int ub = mlp_unit_block(n1), nb = (n1 + ub - 1) / ub;
    const std::vector<double> b = mlp_block_weights(m.w[0].data(), m.D, n1, ub);
    EXPECT(b.size() == (size_t)nb * m.D * ub);
    for (int k = 0; k < nb * ub; ++k)
      for (int j = 0; j < m.D; ++j) {
        const double got = b[((size_t)(k / ub) * m.D + j) * ub + k % ub];
        EXPECT(k < n1 ? same_bits(got, m.w[0][j + (size_t)m.D * k]) : same_bits(got, 0.0));
      }
  }
}

int main() {
  char tmpl[] = "/tmp/mlp_model_check_XXXXXX";
  if (!mkdtemp(tmpl)) { fprintf(stderr, "mlp_model_check: cannot create a temporary directory\n"); return 1; }
  tmpdir = tmpl;
  std::vector<double> w, mn, mx;
  // ---- the parser ----
  std::string f = write_file("good.txt", "1 2.5\n-3e-2\tnan  inf -inf 0x1p-3\n\n  7 \n \n");
  EXPECT(mlp_read_doubles(f.c_str(), &w).empty());
  EXPECT(w.size() == 8 && w[0] == 1.0 && w[1] == 2.5 && w[2] == -3e-2 && w[3] != w[3] && w[4] > 1e308 && w[5] < -1e308 && w[6] == 0.125 && w[7] == 7.0);
  f = write_file("noeol.txt", "4 5");
  EXPECT(mlp_read_doubles(f.c_str(), &w).empty() && w.size() == 2 && w[1] == 5.0);
  f = write_file("empty.txt", "");
  EXPECT(mlp_read_doubles(f.c_str(), &w).empty() && w.empty());
  f = write_file("blank.txt", " \n\t\n");
  EXPECT(mlp_read_doubles(f.c_str(), &w).empty() && w.empty());
  f = write_file("bad.txt", "1 2 three 4");
  EXPECT(mlp_read_doubles(f.c_str(), &w).find("invalid value") != std::string::npos);
  EXPECT(mlp_read_doubles((tmpdir + "/missing.txt").c_str(), &w).find("cannot open") != std::string::npos);
  // min/max: two rows, extras kept for the caller to ignore, blank lines skipped
  f = write_file("mm.txt", "\n0 -1 2 \n\n5 6 7 8\n9 9 9\n");
  EXPECT(mlp_read_minmax(f.c_str(), &mn, &mx).empty() && mn.size() == 3 && mx.size() == 4 && mn[1] == -1.0 && mx[3] == 8.0);
  f = write_file("mm1.txt", "0 1 2\n");
  EXPECT(mlp_read_minmax(f.c_str(), &mn, &mx).find("two rows") != std::string::npos);
  f = write_file("mm0.txt", "");
  EXPECT(mlp_read_minmax(f.c_str(), &mn, &mx).find("two rows") != std::string::npos);
  f = write_file("mmbad.txt", "0 1\n2 x\n");
  EXPECT(mlp_read_minmax(f.c_str(), &mn, &mx).find("invalid value") != std::string::npos);
  // ---- shapes ----
  int D = 0;
  EXPECT(mlp_shape(105 * 10 + 11 * 10 + 10 + 1, 10, 10, &D).empty() && D == 105);
  EXPECT(mlp_shape(2 * 1 + 2 * 1 + 1 + 1, 1, 1, &D).empty() && D == 2);
  EXPECT(mlp_shape(105 * 10 + 11 * 10 + 10 + 2, 10, 10, &D).find("do not fit") != std::string::npos && D == 0);      // a remainder
  EXPECT(mlp_shape(1 * 3 + 4 * 2 + 2 + 1, 3, 2, &D).find("D < 2") != std::string::npos);
  EXPECT(mlp_shape(4 * 2 + 2 + 1, 3, 2, &D).find("do not fit") != std::string::npos);                                 // nothing left for w0
  EXPECT(mlp_shape(0, 0, 0, &D).find("no weights") != std::string::npos);
  EXPECT(mlp_shape(1, 0, 0, &D).find("D < 2") != std::string::npos);
  EXPECT(mlp_shape(2, 0, 0, &D).empty() && D == 2);
  EXPECT(!mlp_shape(100, 3, 0, &D).empty() && !mlp_shape(100, 0, 3, &D).empty() && !mlp_shape(100, -1, -1, &D).empty());
  bool beyond = false;
  EXPECT(mlp_shape(1000000, kMlpMaxHidden + 1, 1, &D, &beyond).find("more than") != std::string::npos && beyond);
  EXPECT(mlp_shape((long long)kMlpMaxDim + 2, 0, 0, &D, &beyond).find("columns") != std::string::npos && beyond);
  EXPECT(!mlp_shape(11, 3, 2, &D, &beyond).empty() && !beyond && mlp_shape(2, 0, 0, &D, &beyond).empty() && !beyond);
  EXPECT(mlp_shape((long long)kMlpMaxDim + 1, 0, 0, &D).empty() && D == kMlpMaxDim + 1);
  // ---- model checks ----
  HostMlp m = random_model(3, 7, 3, 17, true);
  EXPECT(mlp_check(m).empty());
  m.dim1 = 8; EXPECT(mlp_check(m).find("distributor") != std::string::npos);
  m.dim1 = 7; EXPECT(mlp_check(m).empty());
  m.dim0 = -1; EXPECT(mlp_check(m).find("distributor") != std::string::npos);
  m.dim0 = 0; m.mx.pop_back(); EXPECT(mlp_check(m).find("min/max") != std::string::npos);
  m = random_model(3, 7, 3, 17, false);
  m.w[2].resize(m.w[2].size() + 3); EXPECT(mlp_check(m).find("different lengths") != std::string::npos);
  m.n_models = 2; EXPECT(!mlp_check(m).empty());
  // ---- the kernel's layout ----
  EXPECT(mlp_unit_block(1) == 1 && mlp_unit_block(4) == 1 && mlp_unit_block(5) == 2 && mlp_unit_block(10) == 3 && mlp_unit_block(17) == 6);
  EXPECT(mlp_unit_block(64) == 16 && mlp_unit_block(65) == 16 && mlp_unit_block(256) == 16 && mlp_unit_block(33) == 12);
  for (int n1 : {0, 1, 10, 64, 256})
    for (int n2 : {1, 10, 64, 256}) {
      const int b = n1 ? n2 : 0, lim = mlp_stage_max_dim(n1, b);
      EXPECT(lim >= 0 && lim < kMlpMaxDim && (lim == 0 || mlp_plan(lim, n1, b).staged) && !mlp_plan(lim + 1, n1, b).staged);   // 0: never staged
      EXPECT((lim == 0) == (n1 == 256 || b == 256));
      for (int dim : {1, 104, lim ? lim : 1, lim + 1, 4096, kMlpMaxDim}) {
        const MlpPlan p = mlp_plan(dim, n1, b);
        EXPECT((p.stride & 1) && p.tile_rows >= 8 && p.tile_rows <= 64 && (long long)p.stride * p.tile_rows * 8 <= kMlpLdsBytes);
        EXPECT(p.compact == (n1 > 0 && n1 <= 64 && b <= 64));
        EXPECT(p.region_a >= (p.staged ? dim + 1 : 0) && p.region_a >= (n1 ? b + 1 : 0) && p.stride >= p.region_a + (n1 && !p.compact ? n1 + 1 : 0));
        EXPECT(!p.compact || p.region_a >= n1 + 1);
      }
    }
  EXPECT(mlp_plan(104, 10, 10).staged && mlp_plan(104, 10, 10).tile_rows == 64 && mlp_plan(104, 10, 10).stride == 105);
  EXPECT(mlp_plan(104, 64, 64).staged && mlp_plan(104, 64, 64).tile_rows == 64 && !mlp_plan(104, 65, 64).compact);
  // ---- the forward pass ----
  rng_state = 7;
  for (int rescale = 0; rescale < 2; ++rescale) {
    check_forward(1, 1, 1, 1, rescale);
    check_forward(1, 7, 3, 17, rescale);
    check_forward(1, 104, 10, 10, rescale);
    check_forward(3, 104, 17, 3, rescale);
    check_forward(3, 33, 64, 33, rescale);
    check_forward(1, 1, 0, 0, rescale);
    check_forward(3, 104, 0, 0, rescale);
  }
  // relu and sigmoid at the edges
  EXPECT(same_bits(mlp_relu(-0.0), 0.0) && same_bits(mlp_relu(std::numeric_limits<double>::quiet_NaN()), 0.0) && mlp_relu(2.0) == 2.0);
  EXPECT(mlp_sigmoid(std::numeric_limits<double>::infinity()) == 1.0 && mlp_sigmoid(-std::numeric_limits<double>::infinity()) == 0.0);
  EXPECT(mlp_sigmoid(800.0) == 1.0 && mlp_sigmoid(-800.0) == 0.0 && mlp_sigmoid(0.0) == 0.5 && mlp_sigmoid(std::nan("")) != mlp_sigmoid(std::nan("")));
  EXPECT(same_bits(mlp_rescale(3.0, 3.0, 3.0), -1.0) && mlp_rescale(4.0, 3.0, 3.0) > 1e15);
  for (const char* name : {"good.txt", "noeol.txt", "empty.txt", "blank.txt", "bad.txt", "mm.txt", "mm1.txt", "mm0.txt", "mmbad.txt"}) (void)remove((tmpdir + "/" + name).c_str());
  (void)rmdir(tmpdir.c_str());
  if (fails) { fprintf(stderr, "mlp_model_check: %d checks failed\n", fails); return 1; }
  printf("mlp_model_check: OK\n");
  return 0;
}
