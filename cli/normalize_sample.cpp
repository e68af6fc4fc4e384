// cli/normalize_sample.cpp -- drop-in for gadget/main_normalize_sample.cxx: rescales the columns of feature files to [--min, --max]
// (default [-1, 1]) by per-column minima and maxima, found over all input files (stats::rescale, util/stats.hxx:280-314) or read from
// --im, and writes the table that pred_mlp --fmm, train_mlp --fmm and merge_order_bc --bcfmm take.  Host only: no GPU is touched.
//   normalize_sample --i feats... [--im minmax] [--min lo] [--max hi] [--o out...] [--om minmax_out]
// Rows and the table are written with 8 significant digits (FLT_PREC), as the reference writes them; the table is written only when it
// was found here (no --im).  The value of a column is outputDiff * (f - min) / (max - min + FEPS) + outputMin (util/stats.hxx:272).
#include "common.hpp"

using namespace cli;

int main(int argc, char* argv[]) {
  const std::string usage = "Usage: normalize_sample --i <feats>... [--im <minmax>] [--min <lo>] [--max <hi>] [--o <out>...] [--om <minmax out>]   "
                            "(flags as gadget/main_normalize_sample.cxx:57-68)\n";
  Args a = parse(argc, argv, {}, {"i", "im", "min", "max", "o", "om"}, usage);
  if (!a.has("i") || a.all("i").empty()) { std::cerr << "Error: the option '--i' is required but missing\n" << usage; return EXIT_FAILURE; }
  const auto in = a.all("i"), out = a.all("o");
  if (!out.empty() && out.size() < in.size()) perr("Error: fewer output files than input files...");
  const double lo = atof(a.str("min", "-1.0").c_str()), hi = atof(a.str("max", "1.0").c_str());
  std::vector<std::vector<double>> feats(in.size());
  std::vector<int64_t> rows(in.size());
  int dim = 0;
  for (size_t i = 0; i < in.size(); ++i) {
    int d = 0;
    feats[i] = readRows(in[i], &rows[i], &d);
    if (rows[i] > 0 && dim > 0 && d != dim) perr("Error: invalid data file dimension in " + in[i]);
    if (rows[i] > 0) dim = d;
  }
  if (dim == 0) perr("Error: no rows in the input files...");
  std::vector<double> mn((size_t)dim), mx((size_t)dim);
  if (a.has("im")) {
    int64_t r = 0;
    int d = 0;
    const std::vector<double> t = readRows(a.str("im"), &r, &d);
    if (r < 2 || d < dim) perr("Error: the min/max file needs two rows of at least " + std::to_string(dim) + " values: " + a.str("im"));
    for (int j = 0; j < dim; ++j) { mn[j] = t[j]; mx[j] = t[(size_t)d + j]; }
  } else {
    std::vector<const double*> blocks;
    for (auto& f : feats) blocks.push_back(f.data());
    check(glia_hmt_rows_minmax(blocks.data(), rows.data(), (int)blocks.size(), dim, mn.data(), mx.data()));
  }
  const double diff = hi - lo;
  for (size_t i = 0; i < in.size() && !out.empty(); ++i) {
    std::vector<double>& f = feats[i];
    for (int64_t r = 0; r < rows[i]; ++r)
      for (int j = 0; j < dim; ++j) {
        double& v = f[(size_t)r * dim + j];
        const double num = diff * (v - mn[j]), den = (mx[j] - mn[j]) + 2.22e-16;
        const double q = num / den;
        v = q + lo;
      }
    writeRows(out[i], f.data(), rows[i], dim, 8);
  }
  if (!a.has("im") && a.has("om")) {
    std::vector<double> t(mn);
    t.insert(t.end(), mx.begin(), mx.end());
    writeRows(a.str("om"), t.data(), 2, dim, 8);
  }
  return EXIT_SUCCESS;
}
