// cli/train_rf.cpp -- drop-in for ml/rf/main_train_rf.cxx: grows the boundary classifier's forest from feature and label files.
//   train_rf --f feats... --l labels... [--ff fileOfFeatFiles --ll fileOfLabelFiles] [--nt 255] [--mt 0] [--sr 0.7] [--ns 1] [--bal 1]
//            [--seed s] [--maxdepth 0] [--oob 0] [--imp 0] [--impf file] --m model
// Flags and defaults as :11-15,75-98; several files are concatenated in order (rf_old::readMatrixFromFiles).  Feature files are what
// bc_feat -b writes, label files what bc_label_ri / bc_label_vi write (one label per line).  With --bal the per-class counts and
// weights go to stderr as :57-58 prints them.  The trees are this library's own, not classRF's; --seed and --maxdepth are
// additions, and so are --oob, --imp and --impf (classRF's out-of-bag error and variable importances, ml/rf/ml_rf_train.cxx:112-159, by
// the definition of DESIGN 3.16): with --oob 1 the out-of-bag error of the whole forest and of every class goes to stderr and the
// arrays into the model file's own slots (ml/rf/ml_rf_model.cxx:428-448); --imp 1 does the same for the importances, and --impf writes
// them as text, one row per column: per class, all, Gini, then the standard errors per class and all (%.17g).  Without them the
// file is byte for byte what it was.  The model file is the reference's format (ml/rf/ml_rf_model.cxx:378-455): pred_rf and merge_order_bc read it.
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
                            "[--mt 0] [--sr 0.7] [--ns 1] [--bal 1] [--seed <s>] [--maxdepth 0] [--oob 0] [--imp 0] [--impf <importance table>] --m <model>   "
                            "(flags as ml/rf/main_train_rf.cxx:75-98)\n";
  Args a = parse(argc, argv, {}, {"f", "l", "ff", "ll", "nt", "mt", "sr", "ns", "bal", "m", "seed", "maxdepth", "oob", "imp", "impf"}, usage);
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
  glia_hmt_oob_opts oo;
  glia_hmt_oob_opts_default(&oo);
  if (a.has("oob")) oo.oob = flagOf(a, "oob") ? 1 : 0;
  if (a.has("imp")) oo.importance = flagOf(a, "imp") ? 1 : 0;
  const bool impf = a.has("impf") && !a.str("impf").empty();
  if (impf) oo.importance = 1;
  if (oo.oob || oo.importance) check(glia_hmt_forest_train_oob(ctx, X.data(), N, D, Y.data(), &o, &oo, &model));
  else check(glia_hmt_forest_train(ctx, X.data(), N, D, Y.data(), &o, &model));
  int ntree = 0, nclass = 0;
  check(glia_hmt_forest_model_sizes(model, &ntree, nullptr, &nclass, nullptr));
  if (oo.oob) {                                                                                              // next to the class weights
    std::vector<double> errtr((size_t)ntree * (nclass + 1));
    std::vector<int> labels((size_t)nclass);
    check(glia_hmt_forest_model_oob_arrays(model, nullptr, nullptr, nullptr, nullptr, errtr.data(), nullptr, nullptr, nullptr, nullptr));
    check(glia_hmt_forest_model_arrays(model, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, labels.data(), nullptr));
    const double* last = &errtr[(size_t)(ntree - 1) * (nclass + 1)];
    std::cerr << "OOB error: " << last[0] << std::endl;
    for (int k = 0; k < nclass; ++k) std::cerr << "OOB error of class " << labels[k] << ": " << last[1 + k] << std::endl;
  }
  if (impf) {
    std::vector<double> imp((size_t)D * (nclass + 2)), sd((size_t)D * (nclass + 1));
    check(glia_hmt_forest_model_oob_arrays(model, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, imp.data(), sd.data()));
    FILE* f = fopen(a.str("impf").c_str(), "w");
    if (!f) perr("Error: cannot create file " + a.str("impf"));
    for (int v = 0; v < D; ++v) {
      for (int c = 0; c < nclass + 2; ++c) fprintf(f, "%s%.17g", c ? " " : "", imp[(size_t)v * (nclass + 2) + c]);
      for (int c = 0; c < nclass + 1; ++c) fprintf(f, " %.17g", sd[(size_t)v * (nclass + 1) + c]);
      fprintf(f, "\n");
    }
    if (fclose(f) != 0) perr("Error: cannot write file " + a.str("impf"));
  }
  check(glia_hmt_forest_model_write(model, a.str("m").c_str()));
  glia_hmt_forest_model_free(model);
  glia_hmt_ctx_destroy(ctx);
  return EXIT_SUCCESS;
}
