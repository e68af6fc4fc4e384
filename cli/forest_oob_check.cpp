// cli/forest_oob_check.cpp -- the host side of the out-of-bag outputs alone, without the library and without a GPU: the arithmetic of
// glia_amd/csrc/forest_oob.hpp on integers worked out by hand, and the model-file writer of glia_amd/csrc/forest_model.hpp with the
// optional arrays in the slots of ml/rf/ml_rf_model.cxx:428-448.
//   forest_oob_check [file]     checks the arithmetic, writes a small model with every optional array to `file` and prints OK
// Built plainly by cli/Makefile; `make forest_oob_check_san` builds it with -fsanitize=address,undefined for a run on the CPU.
#include <cstdio>

#include "../glia_amd/csrc/forest_oob.hpp"

using namespace glia;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "forest_oob_check: line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static long file_size(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) return -1;
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fclose(f);
  return n;
}

int main(int argc, char** argv) {
  EXPECT(oob_perm_bits(1) == 2 && oob_perm_bits(4) == 2 && oob_perm_bits(5) == 4 && oob_perm_bits(16) == 4 && oob_perm_bits(17) == 6 &&
         oob_perm_bits(4097) == 14);
  EXPECT(oob_ratio(0, 0) == 0.0 && oob_ratio(1, 3) == 1.0 / 3.0 && oob_ratio(-2, 4) == -0.5);
  // votes of 4 rows, 2 classes: a tie goes to the lowest class, a row never out of bag gets 0
  const std::vector<int> counttr = {2, 1, 0, 0, /* class 1 */ 1, 1, 0, 3};
  std::vector<int> outcl, times, votes;
  oob_votes(counttr, 2, 4, &outcl, &times, &votes);
  EXPECT(outcl == std::vector<int>({1, 1, 0, 2}) && times == std::vector<int>({3, 2, 0, 3}));
  EXPECT(votes == std::vector<int>({2, 1, 1, 1, 0, 0, 0, 3}));
  // errtr of 2 trees, 2 classes
  std::vector<double> errtr;
  std::vector<long long> wrong, seen;
  oob_errtr({0, 0, 1, 2, /* tree 1 */ 1, 3, 1, 3}, 2, 2, &errtr, &wrong, &seen);
  EXPECT(errtr == std::vector<double>({0.5, 0.0, 0.5, 2.0 / 6.0, 1.0 / 3.0, 1.0 / 3.0}));
  EXPECT(wrong == std::vector<long long>({1, 0, 1, 2, 1, 1}) && seen == std::vector<long long>({2, 0, 2, 6, 3, 3}));
  // importance of 2 columns over 2 trees (a third tree has no out-of-bag rows and adds nothing)
  ImportanceSums s;
  s.init(2, 2);
  const int d0[4] = {1, -1, 0, 0}, d1[4] = {2, 0, 0, 0};
  const long long n0[2] = {2, 4}, n1[2] = {3, 0}, none[2] = {0, 0};
  s.add_tree(d0, n0); s.add_tree(d1, n1); s.add_tree(d1, none);
  // one tree for the Gini column: the root splits 4 + 2 into (4, 0) and (0, 2) on column 2 with weights 1 and 2
  const int left[3] = {2, 0, 0}, var[3] = {2, 0, 0};
  std::vector<long long> cnt = {0, 0, 4, 0, 0, 2};
  const double w[2] = {1.0, 2.0};
  s.add_tree_gini(left, var, 3, &cnt, w);
  EXPECT(cnt[0] == 4 && cnt[1] == 2);
  std::vector<double> imp, sd;
  s.finish(3, &imp, &sd);
  const double t0 = 0.5 + 2.0 / 3.0, t1 = -0.25, ta = 0.0 / 6.0 + 2.0 / 3.0;
  EXPECT(imp.size() == 8 && sd.size() == 6 && imp[0] == t0 / 3.0 && imp[1] == t1 / 3.0 && imp[2] == ta / 3.0 && imp[3] == 0.0);
  EXPECT(imp[4] == 0.0 && imp[5] == 0.0 && imp[6] == 0.0 && imp[7] == ((4.0 + 4.0) - 32.0 / 8.0) / 3.0);
  const double m0 = t0 / 3.0, q0 = (0.25 + (2.0 / 3.0) * (2.0 / 3.0)) / 3.0;
  EXPECT(sd[0] == std::sqrt((q0 - m0 * m0) / 3.0) && sd[3] == 0.0 && sd[4] == 0.0 && sd[5] == 0.0);
  // the writer: the 9 x 15 model of forest_model_check with arrays of 200 rows x 3 columns
  ForestModel m;
  m.ntree = 9; m.nrnodes = 15; m.nclass = 3; m.mtry = 7;
  const size_t nn = 135;
  m.xbestsplit.assign(nn, 0.0); m.treemap.assign(2 * nn, 0); m.nodestatus.assign(nn, 0); m.nodeclass.assign(nn, 0); m.bestvar.assign(nn, 0);
  m.ndbigtree.assign(9, 1);
  for (int t = 0; t < 9; ++t) { m.nodestatus[(size_t)t * 15] = -1; m.nodeclass[(size_t)t * 15] = 1 + t % 3; }
  m.classwt = {1.0, 2.5, 1.0 / 3.0}; m.cutoff = {0.5, 0.25, 0.25}; m.orig_labels = {-1, 1, 5}; m.new_labels = {1, 2, 3};
  EXPECT(model_check(m).empty() && !m.has_oob() && !m.has_importance());
  long plain = -1;
  if (argc > 1) { EXPECT(write_forest_model(m, argv[1]).empty()); plain = file_size(argv[1]); }
  const size_t N = 200;
  m.oob_rows = (int64_t)N; m.oob_dim = 3;
  m.outcl.assign(N, 1); m.oob_times.assign(N, 2); m.counttr.assign(3 * N, 0); m.votes.assign(3 * N, 0); m.errtr.assign(9 * 4, 0.125);
  for (size_t i = 0; i < N; ++i) { m.counttr[i] = 2; m.votes[3 * i] = 2; }
  EXPECT(model_check(m).empty() && m.has_oob() && !m.has_importance());
  m.importance.assign(3 * 5, 0.5); m.importanceSD.assign(3 * 4, 0.25);
  EXPECT(model_check(m).empty() && m.has_importance());
  if (argc > 1) {
    EXPECT(write_forest_model(m, argv[1]).empty());
    // outcl, counttr, votes, oob_times take the dense flag (more than 128 elements); importance, importanceSD and errtr do not
    EXPECT(file_size(argv[1]) == plain + (1 + 4 * (long)N) + (1 + 12 * (long)N) + 15 * 8 + 12 * 8 + 36 * 8 + (1 + 12 * (long)N) + (1 + 4 * (long)N));
  }
  m.votes.pop_back();
  EXPECT(!model_check(m).empty());
  m.votes.push_back(0); m.importanceSD.clear();
  EXPECT(!model_check(m).empty());
  m.importance.clear(); m.oob_rows = 0;
  EXPECT(!model_check(m).empty());                      // arrays without their sizes
  if (fails) return 1;
  printf("OK\n");
  return 0;
}
