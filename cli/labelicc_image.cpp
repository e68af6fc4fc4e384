// cli/labelicc_image.cpp -- drop-in for gadget/main_labelicc_image.cxx: relabels the face-connected components of equal label
// (labelIdentityConnectedComponents, util/image.hxx:331-373: "Used to relabel 3D label sub-volume cut from bigger volume").
//   labelicc_image -i in.mha [-m mask.mha] [-u 0|1] [-z 0|1] -o out.mha
#include "common.hpp"

using namespace cli;

int main(int argc, char* argv[]) {
  const std::string usage = "Usage: labelicc_image -i <image> [-m mask] [-u b] [-z b] -o <out>   (flags as gadget/main_labelicc_image.cxx:31-44)\n";
  Args a = parse(argc, argv, {{"i", "inputImage"}, {"m", "mask"}, {"u", "write16"}, {"z", "compress"}, {"o", "outputImage"}},
                 {"inputImage", "mask", "write16", "compress", "outputImage"}, usage);
  for (const char* req : {"inputImage", "outputImage"})
    if (!a.has(req)) { std::cerr << "Error: the option '--" << req << "' is required but missing\n" << usage; return EXIT_FAILURE; }
  Volume img = readMetaImage(a.str("inputImage"), false);
  uint32_t* dIn = upload(img.u32);
  uint32_t* dMask = loadMask(a, "mask", img.size());                                                             // :11-13
  uint32_t* dOut;
  hipCheck(hipMalloc(&dOut, img.size() * 4));
  glia_hmt_ctx* ctx;
  check(glia_hmt_ctx_create(0, nullptr, &ctx));
  uint32_t n = 0;
  check(glia_hmt_label_components(ctx, img.dim, img.dims, dIn, dMask, GLIA_HMT_CC_IDENTITY, dOut, &n));          // :14-15
  std::vector<uint32_t> out(img.size());
  hipCheck(hipMemcpy(out.data(), dOut, img.size() * 4, hipMemcpyDeviceToHost));
  writeMetaImage(a.str("outputImage"), img.dim, img.dims, out, flagOf(a, "write16"), flagOf(a, "compress"));     // :16-20
  glia_hmt_ctx_destroy(ctx);
  (void)hipFree(dOut); (void)hipFree(dIn);
  if (dMask) (void)hipFree(dMask);
  return EXIT_SUCCESS;
}
