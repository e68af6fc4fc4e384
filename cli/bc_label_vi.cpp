// cli/bc_label_vi.cpp -- drop-in for hmt/main_bc_label_vi.cxx: merge (-1) / split (+1) label of every merge of a GIVEN order by
// variation of information, the majority over one or more truth volumes.
//   bc_label_vi -s seg.mha -o order.txt -t truth1.mha [truth2.mha ...] [-m mask.mha] [-g 0|1|2] -l labels.txt
#include "common.hpp"

using namespace cli;

int main(int argc, char* argv[]) {
  const std::string usage = "Usage: bc_label_vi -s <seg> -o <order> -t <truth> [<truth> ...] [-m <mask>] [-g 0|1|2] -l <labels>   "
                            "(flags as hmt/main_bc_label_vi.cxx:131-152)\n";
  std::vector<std::string> known = {"segImage", "mergeOrder", "truthImage", "maskImage", "opt", "bcLabels"};
  Args a = parse(argc, argv, {{"s", "segImage"}, {"o", "mergeOrder"}, {"t", "truthImage"}, {"m", "maskImage"}, {"g", "opt"}, {"l", "bcLabels"}},
                 known, usage);
  for (const char* req : {"segImage", "mergeOrder", "truthImage", "bcLabels"})
    if (!a.has(req) || a.all(req).empty()) { std::cerr << "Error: the option '--" << req << "' is required but missing\n" << usage; perr("Error: unable to parse input arguments"); }
  std::vector<uint32_t> order = readOrder(a.str("mergeOrder"));
  const int64_t n = (int64_t)order.size() / 3;
  Volume seg = readMetaImage(a.str("segImage"), false);
  std::vector<uint32_t*> dTruth;
  for (const std::string& f : a.all("truthImage")) {
    Volume t = readMetaImage(f, false);
    if (t.size() != seg.size()) perr("Error: image sizes do not match...");
    dTruth.push_back(upload(t.u32));
  }
  glia_hmt_bc_label_opts o = {GLIA_HMT_BC_LABEL_VI, 0, 1.0, 0, atoi(a.str("opt", "0").c_str())};
  glia_hmt_ctx* ctx; glia_hmt_rag* rag;
  check(glia_hmt_ctx_create(0, nullptr, &ctx));
  uint32_t* dLab = upload(seg.u32);
  float* dZero = upload(std::vector<float>(seg.size(), 0.0f));                  // the map needs an image volume; labels do not read it
  uint32_t* dMask = loadMask(a, "maskImage", seg.size());
  check(glia_hmt_rag_build(ctx, seg.dim, seg.dims, dLab, dMask, /*only_contour=*/0, dZero, nullptr, &rag));
  std::vector<int32_t> labels((size_t)(n ? n : 1));
  std::vector<const uint32_t*> truths(dTruth.begin(), dTruth.end());
  check(glia_hmt_bc_label(ctx, rag, truths.data(), (int)truths.size(), order.data(), n, &o, labels.data()));
  {                                                                               // :124 writeData(labelFile, bcLabels, "\n")
    std::ofstream os(a.str("bcLabels"));
    if (!os) perr("Error: cannot create file " + a.str("bcLabels"));
    for (int64_t i = 0; i < n; ++i) os << labels[i] << "\n";
  }
  glia_hmt_rag_free(rag); glia_hmt_ctx_destroy(ctx);
  (void)hipFree(dLab); (void)hipFree(dZero); if (dMask) (void)hipFree(dMask);
  for (uint32_t* d : dTruth) (void)hipFree(d);
  return EXIT_SUCCESS;
}
