// cli/eval_vi.cpp -- drop-in for gadget/main_eval_vi.cxx: variation of information of proposed label images against reference images.
//   eval_vi -p <res>... -r <ref>... [-m <mask>...] [--exact 1]
// Prints "fs fm fs+fm": false split H(res | ref) and false merge H(ref | res), each the mean over the image pairs (:23-27), over
// the voxels that are not masked out and whose reference label is not 0.  The reference takes log2 of an INTEGER quotient
// (util/image_stats.hxx:153 divides two uints); that is what this tool prints unless --exact 1 asks for the real quotient.
// Masks: none, or one per image -- the reference indexes maskImageFiles[i] for every image once one mask is given (:20), so
// any other number is refused here.
#include "common.hpp"

using namespace cli;

int main(int argc, char* argv[]) {
  const std::string usage = "Usage: eval_vi -p <res>... -r <ref>... [-m <mask>...] [--exact b]   (flags as gadget/main_eval_vi.cxx:36-45)\n";
  Args a = parse(argc, argv, {{"p", "resImage"}, {"r", "refImage"}, {"m", "mask"}}, {"resImage", "refImage", "mask", "exact"}, usage);
  for (const char* req : {"resImage", "refImage"})
    if (!a.has(req)) { std::cerr << "Error: the option '--" << req << "' is required but missing\n" << usage; return EXIT_FAILURE; }
  const size_t nMask = a.all("mask").size();
  if (nMask != 0 && nMask != a.all("resImage").size()) perr("Error: eval_vi takes no mask or one mask per image...");
  EvalInputs in = loadEvalInputs(a);
  glia_hmt_ctx* ctx;
  check(glia_hmt_ctx_create(0, nullptr, &ctx));
  glia_hmt_eval_result r;
  check(glia_hmt_eval(ctx, (int)in.res.size(), in.res.data(), in.ref.data(), in.mask.data(), in.voxels.data(),
                      flagOf(a, "exact") ? GLIA_HMT_VI_EXACT : GLIA_HMT_VI_REFERENCE, &r));
  const double fs = r.false_split, fm = r.false_merge;                                   // :26
  std::cout << fs << " " << fm << " " << fs + fm << std::endl;                           // :27
  glia_hmt_ctx_destroy(ctx);
  return EXIT_SUCCESS;
}
