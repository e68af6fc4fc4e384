// cli/forest_model_check.cpp -- the host side of training alone, without the library and without a GPU: the option arithmetic
// (train_plan: classes, weights, sample size, mtry; the inputs it refuses) and the model-file writer of glia_amd/csrc/forest_model.hpp.
//   forest_model_check [file]     checks the arithmetic, writes a small three-class model to `file` (default: none) and prints OK
// Built plainly by cli/Makefile; `make forest_model_check_san` builds it with -fsanitize=address,undefined for a run on the CPU.
#include <cstdio>
#include <limits>

#include "../glia_amd/csrc/forest_model.hpp"

using namespace glia;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "forest_model_check: line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static std::string plan_of(const std::vector<double>& x, int64_t n, int d, const std::vector<int32_t>& y, const TrainOptions& o, TrainPlan* p) {
  return train_plan(x.data(), n, d, y.data(), o, p);
}

int main(int argc, char** argv) {
  TrainOptions o;
  TrainPlan p;
  EXPECT(o.ntree == 255 && o.mtry == 0 && o.sample_ratio == 0.7 && o.nodesize == 1 && o.balance == 1 && o.max_depth == 0 && o.seed == 0x9E3779B97F4A7C15ull);
  // 40 rows, 30 of class -1 and 10 of class 5, 104 columns
  std::vector<double> x(40 * 104);
  for (size_t i = 0; i < x.size(); ++i) x[i] = (double)(i % 17) - 3.0;
  std::vector<int32_t> y(40, -1);
  for (int i = 0; i < 10; ++i) y[4 * i] = 5;
  EXPECT(plan_of(x, 40, 104, y, o, &p).empty());
  EXPECT(p.nclass == 2 && p.orig_labels[0] == -1 && p.orig_labels[1] == 5 && p.class_count[0] == 30 && p.class_count[1] == 10);
  EXPECT(p.classwt[0] == 1.0 && p.classwt[1] == 3.0 && p.mtry == 10 && p.sampsize == 28 && p.cls[0] == 1 && p.cls[1] == 0);
  o.balance = 0;
  EXPECT(plan_of(x, 40, 104, y, o, &p).empty() && p.classwt[0] == 1.0 && p.classwt[1] == 1.0);
  // (int)((float)N * 0.7 + 0.5) for N = 3, 10, 1001; mtry for D = 1; the clamp
  std::vector<double> col(1001, 0.5);
  std::vector<int32_t> lab(1001, 1);
  lab[0] = 0;
  o = TrainOptions();
  EXPECT(plan_of(col, 3, 1, lab, o, &p).empty() && p.sampsize == 2 && p.mtry == 1);
  EXPECT(plan_of(col, 10, 1, lab, o, &p).empty() && p.sampsize == 7);
  EXPECT(plan_of(col, 1001, 1, lab, o, &p).empty() && p.sampsize == 701);
  o.mtry = 5;
  EXPECT(plan_of(col, 10, 1, lab, o, &p).empty() && p.mtry == 1);
  EXPECT(plan_of(col, 5, 2, lab, o, &p).empty() && p.mtry == 1);                 // 5 > D = 2: floor(sqrt(2))
  o = TrainOptions(); o.sample_ratio = 0.0;
  EXPECT(plan_of(col, 10, 1, lab, o, &p).empty() && p.sampsize == 10);
  o.sample_ratio = 1.0;
  EXPECT(plan_of(col, 10, 1, lab, o, &p).empty() && p.sampsize == 10);
  // refused
  o.sample_ratio = 0.01; EXPECT(plan_of(col, 10, 1, lab, o, &p).find("sample size") != std::string::npos);
  o.sample_ratio = 1.2; EXPECT(plan_of(col, 10, 1, lab, o, &p).find("sample size") != std::string::npos);
  o.sample_ratio = 1e300; EXPECT(plan_of(col, 10, 1, lab, o, &p).find("sample size") != std::string::npos);
  o = TrainOptions();
  EXPECT(plan_of(col, 0, 1, lab, o, &p).find("0 rows") != std::string::npos);
  EXPECT(plan_of(col, 10, 0, lab, o, &p).find("0 columns") != std::string::npos);
  EXPECT(plan_of(col, 1, 1, lab, o, &p).find("two classes") != std::string::npos);
  std::vector<int32_t> nine(10);
  for (int i = 0; i < 10; ++i) nine[i] = i % 9;
  EXPECT(plan_of(col, 10, 1, nine, o, &p).find("more than 8 classes") != std::string::npos);
  std::vector<double> bad = col;
  bad[7] = std::numeric_limits<double>::quiet_NaN();
  EXPECT(plan_of(bad, 10, 1, lab, o, &p).find("non-finite value in row 7, column 0") != std::string::npos);
  bad[7] = -std::numeric_limits<double>::infinity();
  EXPECT(plan_of(bad, 4, 2, lab, o, &p).find("non-finite value in row 3, column 1") != std::string::npos);
  // the writer: 9 trees x 15 nodes (arrays longer than 128 elements take the dense flag), three classes
  ForestModel m;
  m.ntree = 9; m.nrnodes = 15; m.nclass = 3; m.mtry = 7;
  const size_t nn = 135;
  m.xbestsplit.assign(nn, 0.0); m.treemap.assign(2 * nn, 0); m.nodestatus.assign(nn, 0); m.nodeclass.assign(nn, 0); m.bestvar.assign(nn, 0);
  m.ndbigtree.assign(9, 3);
  for (int t = 0; t < 9; ++t) {
    const size_t r = (size_t)t * 15;
    m.xbestsplit[r] = 0.25 * t; m.bestvar[r] = 1 + t; m.nodestatus[r] = 1; m.treemap[2 * r] = 2; m.treemap[2 * r + 1] = 3;
    m.nodestatus[r + 1] = m.nodestatus[r + 2] = -1; m.nodeclass[r + 1] = 1 + t % 3; m.nodeclass[r + 2] = 1 + (t + 1) % 3;
  }
  m.classwt = {1.0, 2.5, 1.0 / 3.0}; m.cutoff = {0.5, 0.25, 0.25}; m.orig_labels = {-1, 1, 5}; m.new_labels = {1, 2, 3};
  EXPECT(model_check(m).empty());
  if (argc > 1) {
    EXPECT(write_forest_model(m, argv[1]).empty());
    FILE* f = fopen(argv[1], "rb");
    EXPECT(f != nullptr);
    if (f) {
      fseek(f, 0, SEEK_END);
      // header + 2 ints + xbestsplit (flag + 135 doubles) + classwt, cutoff + treemap (flag + 270 ints) + 3 x (flag + 135 ints) + ndbigtree + mtry
      // + orig, new labels + nclass
      EXPECT(ftell(f) == 520 + 8 + (1 + 135 * 8) + 2 * 24 + (1 + 270 * 4) + 3 * (1 + 135 * 4) + 36 + 4 + 2 * 12 + 4);
      fclose(f);
    }
  }
  EXPECT(!write_forest_model(m, "/nonexistent-directory/model.bin").empty());
  m.cutoff.pop_back();
  EXPECT(!model_check(m).empty() && !write_forest_model(m, "/dev/null").empty());
  if (fails) return 1;
  printf("OK\n");
  return 0;
}
