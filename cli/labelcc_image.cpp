// cli/labelcc_image.cpp -- drop-in for gadget/main_labelcc_image.cxx: face-connected components of the non-zero voxels of a label
// image (labelConnectedComponents, util/image.hxx:302-313), with --invert of its zero voxels (main_labelcc_image.cxx:10-18).
//   labelcc_image -i in.mha [-v 0|1] [-r 0|1] [-u 0|1] [-z 0|1] -o out.mha
// (components are numbered in raster order of their first voxel; ITK's own order is not pinned, see include/glia_hmt.h)
#include "common.hpp"

using namespace cli;

int main(int argc, char* argv[]) {
  const std::string usage = "Usage: labelcc_image -i <image> [-v b] [-r b] [-u b] [-z b] -o <out>   (flags as gadget/main_labelcc_image.cxx:34-49)\n";
  Args a = parse(argc, argv, {{"i", "inputImage"}, {"v", "invert"}, {"r", "relabel"}, {"u", "write16"}, {"z", "compress"}, {"o", "outputImage"}},
                 {"inputImage", "invert", "relabel", "write16", "compress", "outputImage"}, usage);
  for (const char* req : {"inputImage", "outputImage"})
    if (!a.has(req)) { std::cerr << "Error: the option '--" << req << "' is required but missing\n" << usage; return EXIT_FAILURE; }
  Volume img = readMetaImage(a.str("inputImage"), false);
  uint32_t* dIn = upload(img.u32);
  uint32_t* dOut;
  hipCheck(hipMalloc(&dOut, img.size() * 4));
  glia_hmt_ctx* ctx;
  check(glia_hmt_ctx_create(0, nullptr, &ctx));
  uint32_t n = 0;
  check(glia_hmt_label_components(ctx, img.dim, img.dims, dIn, nullptr, flagOf(a, "invert") ? GLIA_HMT_CC_BINARY_INVERTED : GLIA_HMT_CC_BINARY,
                                  dOut, &n));                                                                    // :10-19
  if (flagOf(a, "relabel")) check(glia_hmt_relabel_image(ctx, dOut, (int64_t)img.size(), 0, &n));                // :20
  std::vector<uint32_t> out(img.size());
  hipCheck(hipMemcpy(out.data(), dOut, img.size() * 4, hipMemcpyDeviceToHost));
  writeMetaImage(a.str("outputImage"), img.dim, img.dims, out, flagOf(a, "write16"), flagOf(a, "compress"));     // :21-25
  glia_hmt_ctx_destroy(ctx);
  (void)hipFree(dOut); (void)hipFree(dIn);
  return EXIT_SUCCESS;
}
