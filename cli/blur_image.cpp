// cli/blur_image.cpp -- drop-in for gadget/main_blur_image.cxx:106-133: discrete Gaussian smoothing of an image (blurImage,
// util/image.hxx:376-407), the step before `watershed` in the usual recipe.
//   blur_image -i in.mha -s sigma -k kernelWidth [-d dim] [-z 0|1] -o out.mha
// The output pixel type is the input's (MET_UCHAR, MET_USHORT, MET_FLOAT; the other types end as the reference's default branch).
// sigma is taken in voxels: the MetaImage reader of these tools keeps no ElementSpacing, so the spacing counts as 1 (ITK would divide
// the variance by the squared spacing).  The operator is the one include/glia_hmt.h defines, not ITK's last digits.
#include "common.hpp"

using namespace cli;

// ElementType of the file's header alone (readImageInfo of the reference): the pixel type decides how the data is read
static std::string elementType(const std::string& file) {
  std::ifstream is(file, std::ios::binary);
  if (!is) perr("Error: cannot open file " + file);
  std::string line;
  while (std::getline(is, line)) {
    const size_t eq = line.find('=');
    if (eq == std::string::npos) continue;
    const size_t a = line.find_first_not_of(" \t"), b = line.find_last_not_of(" \t\r", eq - 1);
    const std::string k = line.substr(a, b - a + 1);
    if (k == "ElementType") { const size_t v0 = line.find_first_not_of(" \t", eq + 1), v1 = line.find_last_not_of(" \t\r"); return line.substr(v0, v1 - v0 + 1); }
    if (k == "ElementDataFile") break;
  }
  return "";
}

int main(int argc, char* argv[]) {
  const std::string usage = "Usage: blur_image -i <image> -s <sigma> -k <kernelWidth> [-d dim] [-z b] -o <out>   (flags as gadget/main_blur_image.cxx:113-128;"
                            " sigma in voxels: element spacing is not read and counts as 1)\n";
  Args a = parse(argc, argv, {{"i", "inputImage"}, {"s", "sigma"}, {"k", "kernelWidth"}, {"d", "dim"}, {"z", "compress"}, {"o", "outputImage"}},
                 {"inputImage", "sigma", "kernelWidth", "dim", "compress", "outputImage"}, usage);
  for (const char* req : {"inputImage", "sigma", "kernelWidth", "outputImage"})
    if (!a.has(req)) { std::cerr << "Error: the option '--" << req << "' is required but missing\n" << usage; return EXIT_FAILURE; }
  const std::string et = elementType(a.str("inputImage"));
  const int type = et == "MET_FLOAT" ? GLIA_HMT_PIXEL_FLOAT32 : et == "MET_UCHAR" ? GLIA_HMT_PIXEL_UINT8 : et == "MET_USHORT" ? GLIA_HMT_PIXEL_UINT16 : -1;
  if (type < 0) perr("Error: unsupported image pixel type...");                                                   // :100
  const double sigma = atof(a.str("sigma").c_str());
  const int width = atoi(a.str("kernelWidth").c_str()), skip = a.has("dim") ? atoi(a.str("dim").c_str()) : -1;
  // float pixels are read as they are; integer pixels fit a uint32 exactly and are narrowed back to their own type
  Volume img = readMetaImage(a.str("inputImage"), type == GLIA_HMT_PIXEL_FLOAT32);
  const size_t n = img.size(), px = type == GLIA_HMT_PIXEL_FLOAT32 ? 4 : type == GLIA_HMT_PIXEL_UINT8 ? 1 : 2;
  std::vector<char> host(n * px);
  if (type == GLIA_HMT_PIXEL_FLOAT32) memcpy(host.data(), img.f32.data(), n * 4);
  else if (type == GLIA_HMT_PIXEL_UINT8) for (size_t i = 0; i < n; ++i) ((uint8_t*)host.data())[i] = (uint8_t)img.u32[i];
  else for (size_t i = 0; i < n; ++i) ((uint16_t*)host.data())[i] = (uint16_t)img.u32[i];
  const double variance[3] = {sigma * sigma, sigma * sigma, sigma * sigma};                                         // image.hxx:382
  const int blurAxis = skip == 0 ? 1 : 0;                  // any blurred axis: they share one kernel
  {
    // the warning ITK prints when the kernel is cut by the maximum width, with the mass it covers
    double c[GLIA_HMT_BLUR_MAX_WIDTH + 1], covered = 0;
    int radius = 0;
    if (glia_hmt_gaussian_kernel(variance[blurAxis], width, GLIA_HMT_BLUR_MAX_ERROR, c, GLIA_HMT_BLUR_MAX_WIDTH + 1, &radius, &covered) == GLIA_HMT_OK &&
        covered < 1.0 - GLIA_HMT_BLUR_MAX_ERROR)
      std::cerr << "Warning: Gaussian kernel size was truncated to kernelWidth = " << width << ": it covers " << covered << " of the mass (wanted "
                << 1.0 - GLIA_HMT_BLUR_MAX_ERROR << ")" << std::endl;
  }
  char *dIn = upload(host), *dOut;
  hipCheck(hipMalloc(&dOut, host.size()));
  glia_hmt_ctx* ctx;
  check(glia_hmt_ctx_create(0, nullptr, &ctx));
  check(glia_hmt_blur_image(ctx, img.dim, img.dims, type, dIn, variance, width, skip < 0 ? -1 : skip, dOut));     // :14-15
  hipCheck(hipMemcpy(host.data(), dOut, host.size(), hipMemcpyDeviceToHost));
  writeMetaImageBytes(a.str("outputImage"), img.dim, img.dims, et.c_str(), host.data(), host.size(), flagOf(a, "compress"));
  glia_hmt_ctx_destroy(ctx);
  (void)hipFree(dOut); (void)hipFree(dIn);
  return EXIT_SUCCESS;
}
