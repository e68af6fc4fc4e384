// cli/bc_label_ri.cpp -- drop-in for hmt/main_bc_label_ri.cxx: merge (-1) / split (+1) label of every merge of a GIVEN order
// against one truth volume, by pair F1 (--f1 true, default) or Rand index (--f1 false).
//   bc_label_ri -s seg.mha -o order.txt -t truth.mha [-n mask.mha] [--f1 b] [-g 0|1|2] [-p b] [-w b] [-d mpd] [-l labels.txt]
#include "common.hpp"

using namespace cli;

int main(int argc, char* argv[]) {
  const std::string usage = "Usage: bc_label_ri -s <seg> -o <order> -t <truth> [-n <mask>] [--f1 b] [-g 0|1|2] [-p b] [-w b] [-d mpd] "
                            "[-l <labels>]   (flags as hmt/main_bc_label_ri.cxx:156-182)\n";
  std::vector<std::string> known = {"segImage", "mergeOrder", "truthImage", "maskImage", "f1", "opt", "optSplit", "tweak", "mpd", "bclabel"};
  Args a = parse(argc, argv, {{"s", "segImage"}, {"o", "mergeOrder"}, {"t", "truthImage"}, {"n", "maskImage"}, {"g", "opt"}, {"p", "optSplit"},
                              {"w", "tweak"}, {"d", "mpd"}, {"l", "bclabel"}}, known, usage);
  for (const char* req : {"segImage", "mergeOrder", "truthImage"})
    if (!a.has(req)) { std::cerr << "Error: the option '--" << req << "' is required but missing\n" << usage; perr("Error: unable to parse input arguments"); }
  std::vector<uint32_t> order = readOrder(a.str("mergeOrder"));
  const int64_t n = (int64_t)order.size() / 3;
  Volume seg = readMetaImage(a.str("segImage"), false), truth = readMetaImage(a.str("truthImage"), false);
  if (truth.size() != seg.size()) perr("Error: image sizes do not match...");
  glia_hmt_bc_label_opts o = {a.has("f1") && !flagOf(a, "f1") ? GLIA_HMT_BC_LABEL_RI : GLIA_HMT_BC_LABEL_F1, flagOf(a, "tweak") ? 1 : 0,
                              atof(a.str("mpd", "1.0").c_str()), flagOf(a, "optSplit") ? 1 : 0, atoi(a.str("opt", "0").c_str())};
  glia_hmt_ctx* ctx; glia_hmt_rag* rag;
  check(glia_hmt_ctx_create(0, nullptr, &ctx));
  uint32_t* dLab = upload(seg.u32);
  uint32_t* dTruth = upload(truth.u32);
  float* dZero = upload(std::vector<float>(seg.size(), 0.0f));                  // the map needs an image volume; labels do not read it
  uint32_t* dMask = loadMask(a, "maskImage", seg.size());
  check(glia_hmt_rag_build(ctx, seg.dim, seg.dims, dLab, dMask, /*only_contour=*/0, dZero, nullptr, &rag));
  std::vector<int32_t> labels((size_t)(n ? n : 1));
  const uint32_t* truths[1] = {dTruth};
  check(glia_hmt_bc_label(ctx, rag, truths, 1, order.data(), n, &o, labels.data()));
  if (a.has("bclabel")) {                                                         // :150 writeData(bcLabelFile, bcLabels, "\n")
    std::ofstream os(a.str("bclabel"));
    if (!os) perr("Error: cannot create file " + a.str("bclabel"));
    for (int64_t i = 0; i < n; ++i) os << labels[i] << "\n";
  }
  glia_hmt_rag_free(rag); glia_hmt_ctx_destroy(ctx);
  (void)hipFree(dLab); (void)hipFree(dTruth); (void)hipFree(dZero); if (dMask) (void)hipFree(dMask);
  return EXIT_SUCCESS;
}
