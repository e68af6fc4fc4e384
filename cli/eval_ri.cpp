// cli/eval_ri.cpp -- drop-in for gadget/main_eval_ri.cxx: Rand scores of proposed label images against reference images.
//   eval_ri -p <res>... -r <ref>... [-m <mask>...] [-a 0|1]
// -a 1 (default), the adapted Rand error: prints "prec rec 1-f" of the pair counts summed over the image pairs (:41-53);
// -a 0, the traditional Rand index: prints "ri" (:55-59).  Masked-out voxels and voxels whose reference label is 0 do not count
// (:38-39); there may be fewer masks than images (:34).  Numbers in the stream's default format, as the reference prints them.
#include "common.hpp"

using namespace cli;

int main(int argc, char* argv[]) {
  const std::string usage = "Usage: eval_ri -p <res>... -r <ref>... [-m <mask>...] [-a b]   (flags as gadget/main_eval_ri.cxx:68-81)\n";
  Args a = parse(argc, argv, {{"p", "resImage"}, {"r", "refImage"}, {"m", "mask"}, {"a", "adapted"}}, {"resImage", "refImage", "mask", "adapted"}, usage);
  for (const char* req : {"resImage", "refImage"})
    if (!a.has(req)) { std::cerr << "Error: the option '--" << req << "' is required but missing\n" << usage; return EXIT_FAILURE; }
  const bool adapted = a.has("adapted") ? flagOf(a, "adapted") : true;
  EvalInputs in = loadEvalInputs(a);
  glia_hmt_ctx* ctx;
  check(glia_hmt_ctx_create(0, nullptr, &ctx));
  glia_hmt_eval_result r;
  check(glia_hmt_eval(ctx, (int)in.res.size(), in.res.data(), in.ref.data(), in.mask.data(), in.voxels.data(), GLIA_HMT_VI_REFERENCE, &r));
  if (adapted) std::cout << r.precision << " " << r.recall << " " << 1.0 - r.f1 << std::endl;      // :48-53
  else std::cout << r.rand_index << std::endl;                                                       // :55-59
  glia_hmt_ctx_destroy(ctx);
  return EXIT_SUCCESS;
}
