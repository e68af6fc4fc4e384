// cli/pred_mlp.cpp -- drop-in for sshmt/main_pred_mlp.cxx: the MLP classifier's value for every row of feature files.
//   pred_mlp --m model... [--fmm minmax] [--md d0 d1 thr] --f feats... --nn1 N --nn2 N --p preds...
// File i of --f goes to file i of --p.  Feature files are what bc_feat -b writes: one row per line, values separated by blanks
// (readData, util/text_io.hxx); rows of unequal length are an error, an empty file gives an empty output.  Predictions are written as
// writeData(file, preds, "\n") does (:45): no precision argument, so the stream's default of 6 significant digits.
#include "common.hpp"

using namespace cli;

int main(int argc, char* argv[]) {
  const std::string usage = "Usage: pred_mlp --m <model>... [--fmm <minmax>] [--md <dim0> <dim1> <threshold>] --f <feats>... --nn1 <N> --nn2 <N> "
                            "--p <preds>...   (flags as sshmt/main_pred_mlp.cxx:54-71)\n";
  Args a = parse(argc, argv, {}, {"m", "fmm", "md", "f", "nn1", "nn2", "p"}, usage);
  for (const char* req : {"m", "f", "nn1", "nn2", "p"})
    if (!a.has(req) || a.all(req).empty()) { std::cerr << "Error: the option '--" << req << "' is required but missing\n" << usage; return EXIT_FAILURE; }
  const auto models = a.all("m"), md = a.all("md"), featFiles = a.all("f"), predFiles = a.all("p");
  if (models.size() != 1 && md.size() != 3) perr("Error: model distributor needs 3 arguments...");
  if (predFiles.size() < featFiles.size()) perr("Error: fewer prediction files than feature files...");
  glia_hmt_ctx* ctx;
  check(glia_hmt_ctx_create(0, nullptr, &ctx));
  std::vector<const char*> paths;
  for (auto& m : models) paths.push_back(m.c_str());
  double dist[3] = {0, 0, 0};
  for (size_t i = 0; i < 3 && i < md.size(); ++i) dist[i] = atof(md[i].c_str());
  const std::string fmm = a.str("fmm");
  glia_hmt_mlp* mlp;
  check(glia_hmt_mlp_load(ctx, (int)models.size(), paths.data(), atoi(a.str("nn1").c_str()), atoi(a.str("nn2").c_str()),
                          fmm.empty() ? nullptr : fmm.c_str(), models.size() == 1 ? nullptr : dist, &mlp));
  for (size_t i = 0; i < featFiles.size(); ++i) {
    int64_t rows = 0;
    int dim = 0;
    const std::vector<double> x = readRows(featFiles[i], &rows, &dim);
    std::vector<double> pred((size_t)rows);
    if (rows > 0) check(glia_hmt_mlp_predict(ctx, mlp, x.data(), rows, dim, pred.data(), nullptr));
    writeDoubles(predFiles[i], pred.data(), rows);
  }
  glia_hmt_mlp_free(mlp);
  glia_hmt_ctx_destroy(ctx);
  return EXIT_SUCCESS;
}
