// cli/pred_rf.cpp -- drop-in for ml/rf/main_pred_rf.cxx: the classifier's value for every row of feature files.
//   pred_rf --m model... [--md d0 d1 thr] --f feats... --l label --p preds...
// File i of --f goes to file i of --p.  Feature files are what bc_feat -b and merge_order_bc -b write: one row per line, values
// separated by blanks (readData, util/text_io.hxx); rows of unequal length are an error, an empty file gives an empty output.
// Predictions are written as writeData(file, preds, "\n", FLT_PREC) does (:37).
#include "common.hpp"

using namespace cli;

int main(int argc, char* argv[]) {
  const std::string usage = "Usage: pred_rf --m <model>... [--md <dim0> <dim1> <threshold>] --f <feats>... --l <label> --p <preds>...   "
                            "(flags as ml/rf/main_pred_rf.cxx:43-60)\n";
  Args a = parse(argc, argv, {}, {"m", "md", "f", "l", "p"}, usage);
  for (const char* req : {"m", "f", "l", "p"})
    if (!a.has(req) || a.all(req).empty()) { std::cerr << "Error: the option '--" << req << "' is required but missing\n" << usage; return EXIT_FAILURE; }
  const auto models = a.all("m"), md = a.all("md"), featFiles = a.all("f"), predFiles = a.all("p");
  if (models.size() != 1 && md.size() != 3) perr("Error: model distributor needs 3 arguments...");           // :21-22
  if (predFiles.size() < featFiles.size()) perr("Error: fewer prediction files than feature files...");
  glia_hmt_ctx* ctx;
  check(glia_hmt_ctx_create(0, nullptr, &ctx));
  std::vector<const char*> paths;
  for (auto& m : models) paths.push_back(m.c_str());
  double dist[3] = {0, 0, 0};
  for (size_t i = 0; i < 3 && i < md.size(); ++i) dist[i] = atof(md[i].c_str());
  glia_hmt_forest* forest;
  check(glia_hmt_forest_load(ctx, (int)models.size(), paths.data(), atoi(a.str("l").c_str()), models.size() == 1 ? nullptr : dist, &forest));
  for (size_t i = 0; i < featFiles.size(); ++i) {
    int64_t rows = 0;
    int dim = 0;
    const std::vector<double> x = readRows(featFiles[i], &rows, &dim);
    std::vector<double> pred((size_t)rows);
    if (rows > 0) check(glia_hmt_forest_predict(ctx, forest, x.data(), rows, dim, pred.data()));
    writeDoubles(predFiles[i], pred.data(), rows, 8);                                                          // FLT_PREC
  }
  glia_hmt_forest_free(forest);
  glia_hmt_ctx_destroy(ctx);
  return EXIT_SUCCESS;
}
