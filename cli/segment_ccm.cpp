// cli/segment_ccm.cpp -- drop-in for hmt/main_segment_ccm.cxx: the tree inference of the HMT paper -- node energies from the merge
// probabilities, energy tuples bottom-up, resolution top-down -- and the final label image; -b writes the boundary-confidence image.
//   segment_ccm -s seg.mha -o order.txt -p mergeProbs.txt [-m mask.mha] [-i 0|1] [-r b] [-u b] [-z b] [-f out.mha] [-b bc.mha]
#include "common.hpp"

using namespace cli;

static std::vector<double> readDoubles(const std::string& file) {
  std::ifstream is(file);
  if (!is) perr("Error: cannot open file " + file);
  std::vector<double> v;
  double x;
  while (is >> x) v.push_back(x);
  return v;
}

int main(int argc, char* argv[]) {
  const std::string usage = "Usage: segment_ccm -s <seg> -o <order> -p <mergeProbs> [-m <mask>] [-i b] [-r b] [-u b] [-z b] [-f <finalSeg>] [-b <bcImage>]   "
                            "(flags as hmt/main_segment_ccm.cxx:107-130)\n";
  Args a = parse(argc, argv, {{"s", "segImage"}, {"o", "mergeOrder"}, {"p", "mergeProbs"}, {"m", "maskImage"}, {"i", "ignore"}, {"r", "relabel"},
                              {"u", "write16"}, {"z", "compress"}, {"f", "finalSegImage"}, {"b", "bcImage"}},
                 {"segImage", "mergeOrder", "mergeProbs", "maskImage", "ignore", "relabel", "write16", "compress", "finalSegImage", "bcImage"}, usage);
  for (const char* req : {"segImage", "mergeOrder", "mergeProbs"})
    if (!a.has(req)) { std::cerr << "Error: the option '--" << req << "' is required but missing\n" << usage; return EXIT_FAILURE; }
  const std::vector<uint32_t> order = readOrder(a.str("mergeOrder"));
  const std::vector<double> probs = readDoubles(a.str("mergeProbs"));
  const int64_t n = (int64_t)order.size() / 3, cap = 3 * n + 1;
  if ((int64_t)probs.size() < n) perr("Error: too few merge probabilities...");
  std::vector<uint32_t> lab((size_t)cap);
  std::vector<int32_t> par((size_t)cap), c0((size_t)cap), c1((size_t)cap);
  std::vector<double> em((size_t)cap), es((size_t)cap), Em((size_t)cap), Es((size_t)cap);
  const int64_t nn = glia_hmt_tree_energies(order.data(), n, probs.data(), lab.data(), par.data(), c0.data(), c1.data(), em.data(), es.data(),
                                            Em.data(), Es.data(), cap);                                                  // :37-53
  if (nn < 0) perr(glia_hmt_last_error());
  Volume seg = readMetaImage(a.str("segImage"), false);
  uint32_t* dLab = upload(seg.u32);
  uint32_t* dMask = loadMask(a, "maskImage", seg.size());
  glia_hmt_ctx* ctx;
  check(glia_hmt_ctx_create(0, nullptr, &ctx));
  if (a.has("bcImage")) {                                                                                               // :58-88
    std::vector<double> conf((size_t)(nn ? nn : 1));
    check(glia_hmt_tree_ccm_confidence(par.data(), c0.data(), c1.data(), es.data(), Em.data(), Es.data(), nn, nullptr, nullptr, conf.data()));
    std::vector<float> zeros(seg.size(), 0.0f);
    float* dZ = upload(zeros);                                       // the contour-only map needs an image volume; its values are not used
    float* dOut = upload(zeros);
    glia_hmt_rag* rag;
    check(glia_hmt_rag_build(ctx, seg.dim, seg.dims, dLab, dMask, /*only_contour=*/1, dZ, nullptr, &rag));
    const uint32_t* pl = lab.data(); const int32_t* pp = par.data(); const int32_t* p0 = c0.data(); const double* pq = conf.data();
    check(glia_hmt_boundary_confidence(ctx, rag, 1, &nn, &pl, &pp, &p0, &pq, dOut));
    hipCheck(hipMemcpy(zeros.data(), dOut, zeros.size() * 4, hipMemcpyDeviceToHost));
    writeMetaImageFloat(a.str("bcImage"), seg.dim, seg.dims, zeros, flagOf(a, "compress"));
    glia_hmt_rag_free(rag);
    (void)hipFree(dZ); (void)hipFree(dOut);
  }
  if (a.has("finalSegImage")) {                                                                                         // :90-100
    std::vector<int32_t> picks((size_t)(nn ? nn : 1));
    const int64_t np = glia_hmt_resolve_tree_ccm(c0.data(), c1.data(), Em.data(), Es.data(), nn, picks.data(), nn);
    if (np < 0) perr(glia_hmt_last_error());
    std::vector<uint32_t> src((size_t)(nn ? nn : 1)), dst((size_t)(nn ? nn : 1));
    const int64_t m = glia_hmt_label_transform(lab.data(), c0.data(), c1.data(), nn, picks.data(), np, 1u, src.data(), dst.data(), (int64_t)src.size());
    if (m < 0) perr(glia_hmt_last_error());
    const bool ignore = a.has("ignore") ? flagOf(a, "ignore") : true;                                                   // default true
    check(glia_hmt_transform_image(ctx, dLab, (int64_t)seg.size(), src.data(), dst.data(), m, dMask, ignore ? 1 : 0));  // genFinalSegmentation
    uint32_t nl = 0;
    if (flagOf(a, "relabel")) check(glia_hmt_relabel_image(ctx, dLab, (int64_t)seg.size(), 0, &nl));
    hipCheck(hipMemcpy(seg.u32.data(), dLab, seg.size() * 4, hipMemcpyDeviceToHost));
    writeMetaImage(a.str("finalSegImage"), seg.dim, seg.dims, seg.u32, flagOf(a, "write16"), flagOf(a, "compress"));
  }
  glia_hmt_ctx_destroy(ctx);
  (void)hipFree(dLab);
  if (dMask) (void)hipFree(dMask);
  return EXIT_SUCCESS;
}
