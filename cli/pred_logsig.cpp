// cli/pred_logsig.cpp -- drop-in for sshmt/main_pred_logsig.cxx: the logsig classifier's value for every row of feature files.
//   pred_logsig --m model --f feats... --p preds...
// File i of --f goes to file i of --p; a 1 is appended to every row for the bias (:22-23), so the model holds one weight more than a
// row has columns.  Predictions are written as writeData(file, preds, "\n") does (:29): 6 significant digits.
#include "common.hpp"

using namespace cli;

int main(int argc, char* argv[]) {
  const std::string usage = "Usage: pred_logsig --m <model> --f <feats>... --p <preds>...   (flags as sshmt/main_pred_logsig.cxx:38-46)\n";
  Args a = parse(argc, argv, {}, {"m", "f", "p"}, usage);
  for (const char* req : {"m", "f", "p"})
    if (!a.has(req) || a.all(req).empty()) { std::cerr << "Error: the option '--" << req << "' is required but missing\n" << usage; return EXIT_FAILURE; }
  const auto featFiles = a.all("f"), predFiles = a.all("p");
  if (predFiles.size() < featFiles.size()) perr("Error: fewer prediction files than feature files...");
  glia_hmt_ctx* ctx;
  check(glia_hmt_ctx_create(0, nullptr, &ctx));
  const std::string model = a.str("m");
  const char* path = model.c_str();
  glia_hmt_mlp* mlp;
  check(glia_hmt_mlp_load(ctx, 1, &path, 0, 0, nullptr, nullptr, &mlp));
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
