// cli/train_rf.cpp -- drop-in for ml/rf/main_train_rf.cxx: grows the boundary classifier's forest from feature and label files.
//   train_rf --f feats... --l labels... [--ff fileOfFeatFiles --ll fileOfLabelFiles] [--nt 255] [--mt 0] [--sr 0.7] [--ns 1] [--bal 1]
//            [--seed s] [--maxdepth 0] --m model
// Flags and defaults as :11-15,75-98; several files are concatenated in order (rf_old::readMatrixFromFiles).  Feature files are what
// bc_feat -b writes, label files what bc_label_ri / bc_label_vi write (one label per line).  With --bal the per-class counts and
// weights go to stderr as :57-58 prints them.  The trees are this library's own, not classRF's; --seed and --maxdepth are
// additions.  The model file is the reference's format (ml/rf/ml_rf_model.cxx:378-455): pred_rf and merge_order_bc read it.
#include "common.hpp"

using namespace cli;

// the names in a file of file names (readData(names, file, true), :25-26)
static std::vector<std::string> readNames(const std::string& file) {
  std::ifstream is(file);
  if (!is) perr("Error: cannot open file " + file);
  std::vector<std::string> v;
  std::string s;
  while (is >> s) v.push_back(s);
  return v;
}

// rf_old::readMatrixFromFiles: the rows of every file, in order; *dim = their common length
static std::vector<double> readMatrix(const std::vector<std::string>& files, int64_t* rows, int* dim) {
  std::vector<double> all;
  *rows = 0; *dim = 0;
  for (const std::string& f : files) {
    int64_t n = 0;
    int d = 0;
    const std::vector<double> x = readRows(f, &n, &d);
    if (n == 0) continue;
    if (*rows > 0 && d != *dim) perr("Error: incorrect matrices dimension...");
    *dim = d; *rows += n;
    all.insert(all.end(), x.begin(), x.end());
  }
  return all;
}

int main(int argc, char* argv[]) {
  const std::string usage = "Usage: train_rf --f <feats>... --l <labels>... [--ff <file of feature file names> --ll <file of label file names>] [--nt 255] "
                            "[--mt 0] [--sr 0.7] [--ns 1] [--bal 1] [--seed <s>] [--maxdepth 0] --m <model>   (flags as ml/rf/main_train_rf.cxx:75-98)\n";
  Args a = parse(argc, argv, {}, {"f", "l", "ff", "ll", "nt", "mt", "sr", "ns", "bal", "m", "seed", "maxdepth"}, usage);
  if (!a.has("m") || a.all("m").empty()) { std::cerr << "Error: the option '--m' is required but missing\n" << usage; return EXIT_FAILURE; }
  std::vector<std::string> featFiles = a.all("f"), labelFiles = a.all("l");
  if (a.has("ff") && !a.str("ff").empty()) {
    for (auto& n : readNames(a.str("ff"))) featFiles.push_back(n);
    for (auto& n : readNames(a.str("ll"))) labelFiles.push_back(n);
  }
  int64_t N = 0, Ny = 0;
  int D = 0, Dy = 0;
  const std::vector<double> X = readMatrix(featFiles, &N, &D);
  const std::vector<double> Yd = readMatrix(labelFiles, &Ny, &Dy);
  if (N != Ny || Dy != 1) perr("Error: incorrect matrices dimension...");                                    // :36-37
  std::vector<int32_t> Y((size_t)N);
  for (int64_t i = 0; i < N; ++i) Y[i] = (int32_t)Yd[i];
  glia_hmt_train_opts o;
  glia_hmt_train_opts_default(&o);
  if (a.has("nt")) o.ntree = atoi(a.str("nt").c_str());
  if (a.has("mt")) o.mtry = atoi(a.str("mt").c_str());
  if (a.has("sr")) o.sample_ratio = atof(a.str("sr").c_str());
  if (a.has("ns")) o.nodesize = atoi(a.str("ns").c_str());
  if (a.has("bal")) o.balance = flagOf(a, "bal") ? 1 : 0;
  if (a.has("maxdepth")) o.max_depth = atoi(a.str("maxdepth").c_str());
  if (a.has("seed")) o.seed = strtoull(a.str("seed").c_str(), nullptr, 0);
  if (o.balance) {                                                                                           // :46-60
    std::map<int, long long> count;
    for (int32_t y : Y) ++count[y];
    long long maxcnt = -1;
    for (auto& c : count) if (c.second > maxcnt) maxcnt = c.second;
    for (auto& c : count) std::cerr << "Class " << c.first << ": " << c.second << " [w = " << (double)maxcnt / (double)c.second << "]" << std::endl;
  }
  glia_hmt_ctx* ctx;
  check(glia_hmt_ctx_create(0, nullptr, &ctx));
  glia_hmt_forest_model* model;
  check(glia_hmt_forest_train(ctx, X.data(), N, D, Y.data(), &o, &model));
  check(glia_hmt_forest_model_write(model, a.str("m").c_str()));
  glia_hmt_forest_model_free(model);
  glia_hmt_ctx_destroy(ctx);
  return EXIT_SUCCESS;
}
