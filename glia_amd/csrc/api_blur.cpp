// glia_amd/csrc/api_blur.cpp -- C ABI of blur_image (include/glia_hmt.h): the coefficient rule and the host definition
// (gaussian_kernel.hpp) exported, and the device call (blur.hip) behind its argument checks.
#include <cmath>

#include "api_types.hpp"
#include "gaussian_kernel.hpp"

namespace {

static_assert(kBlurMaxRadius == GLIA_HMT_BLUR_MAX_WIDTH, "a radius never exceeds the maximum width");

int blur_bad(const char* what) { set_error(std::string("blur_image: ") + what); return GLIA_HMT_ERR_ARG; }

// what the host and the device call share; every test comes before the first HIP call.  *n: the voxel count
int blur_args(int dim, const int64_t dims[3], int pixel_type, const void* in, const double variance[3], int max_width, int skip_axis, const void* out,
              uint64_t* n) {
  if (!dims || !variance || !in || !out) return blur_bad("dims, variance and the two volumes must not be NULL");
  if (dim != 2 && dim != 3) return blur_bad("dim must be 2 or 3");
  const uint64_t most = 0xFFFFFFFEull;
  *n = 1;
  for (int i = 0; i < dim; ++i) {
    if (dims[i] <= 0) return blur_bad("extents must be positive");
    if ((uint64_t)dims[i] > most / *n) return blur_bad("between 1 and 2^32 - 2 voxels");
    *n *= (uint64_t)dims[i];
  }
  if (pixel_type != GLIA_HMT_PIXEL_FLOAT32 && pixel_type != GLIA_HMT_PIXEL_UINT8 && pixel_type != GLIA_HMT_PIXEL_UINT16)
    return blur_bad("pixel_type must be GLIA_HMT_PIXEL_FLOAT32, _UINT8 or _UINT16");
  if (skip_axis < -1 || skip_axis >= dim) return blur_bad("skip_axis must be -1 or an axis of the image");
  if (max_width < 1 || max_width > GLIA_HMT_BLUR_MAX_WIDTH) return blur_bad("max_width must be between 1 and 128");
  for (int a = 0; a < dim; ++a)
    if (a != skip_axis && !(std::isfinite(variance[a]) && variance[a] > 0.0 && variance[a] <= GLIA_HMT_BLUR_MAX_VARIANCE))
      return blur_bad("the variance of a blurred axis must be finite, positive and at most 256");
  if (in == out) return blur_bad("the volume cannot be blurred in place");
  return GLIA_HMT_OK;
}

}  // namespace

extern "C" {

int glia_hmt_gaussian_kernel(double variance, int max_width, double max_error, double* coeffs, int capacity, int* radius, double* covered) {
  auto bad = [](const char* what) { set_error(std::string("gaussian_kernel: ") + what); return GLIA_HMT_ERR_ARG; };
  if (!coeffs || !radius) return bad("coeffs and radius must not be NULL");
  if (!(std::isfinite(variance) && variance > 0.0 && variance <= GLIA_HMT_BLUR_MAX_VARIANCE)) return bad("the variance must be finite, positive and at most 256");
  if (max_width < 1 || max_width > GLIA_HMT_BLUR_MAX_WIDTH) return bad("max_width must be between 1 and 128");
  if (!(max_error > 0.0 && max_error < 1.0)) return bad("max_error must lie in (0, 1)");
  const GaussianKernel g = gaussian_kernel(variance, max_width, max_error);
  *radius = g.radius;
  if (covered) *covered = g.covered;
  if (capacity < g.radius + 1) { set_error("gaussian_kernel: " + std::to_string(g.radius + 1) + " coefficients, capacity " + std::to_string(capacity)); return GLIA_HMT_ERR_CAPACITY; }
  std::copy(g.c.begin(), g.c.end(), coeffs);
  return GLIA_HMT_OK;
}

int glia_hmt_blur_image_host(int dim, const int64_t dims[3], int pixel_type, const void* h_in, const double variance[3], int max_width, int skip_axis,
                             void* h_out) {
  uint64_t n = 0;
  if (int rc = blur_args(dim, dims, pixel_type, h_in, variance, max_width, skip_axis, h_out, &n)) return rc;
  if (pixel_type == GLIA_HMT_PIXEL_UINT8) blur_image_host(dim, dims, (const uint8_t*)h_in, variance, max_width, skip_axis, (uint8_t*)h_out);
  else if (pixel_type == GLIA_HMT_PIXEL_UINT16) blur_image_host(dim, dims, (const uint16_t*)h_in, variance, max_width, skip_axis, (uint16_t*)h_out);
  else blur_image_host(dim, dims, (const float*)h_in, variance, max_width, skip_axis, (float*)h_out);
  return GLIA_HMT_OK;
}

int glia_hmt_blur_image(glia_hmt_ctx* c, int dim, const int64_t dims[3], int pixel_type, const void* d_in, const double variance[3], int max_width,
                        int skip_axis, void* d_out) {
  if (!c) return blur_bad("ctx must not be NULL");
  uint64_t n = 0;
  if (int rc = blur_args(dim, dims, pixel_type, d_in, variance, max_width, skip_axis, d_out, &n)) return rc;
  int route = GLIA_HMT_BLUR_ROUTE_PASSES;
  std::string v;
  if (option("GLIA_HMT_BLUR", &v) && v != "passes") {
    if (v != "march") return blur_bad(("GLIA_HMT_BLUR must be passes or march, not '" + v + "'").c_str());
    route = GLIA_HMT_BLUR_ROUTE_MARCH;
  }
  GaussianKernel kernels[3];
  const GaussianKernel* taps[3] = {nullptr, nullptr, nullptr};
  for (int a = 0; a < dim; ++a)
    if (a != skip_axis) { kernels[a] = gaussian_kernel(variance[a], max_width, GLIA_HMT_BLUR_MAX_ERROR); taps[a] = &kernels[a]; }
  GLIA_HIP_TRY(hipSetDevice(c->device));
  return blur_image_device(dim, dims, pixel_type, d_in, taps, route, d_out, c->stream, &c->blur_ms, &c->blur_route);
}

int glia_hmt_blur_limits(int* tile_x, int* tile_y, int* max_march_radius, int* max_radius) {
  if (tile_x) *tile_x = kBlurTileX;
  if (tile_y) *tile_y = kBlurTileY;
  if (max_march_radius) *max_march_radius = kBlurMarchRadius;
  if (max_radius) *max_radius = kBlurMaxRadius;
  return GLIA_HMT_OK;
}

int glia_hmt_last_blur_timing(const glia_hmt_ctx* c, double* ms, int* route_used) {
  if (!c) { set_error("last_blur_timing: ctx must not be NULL"); return GLIA_HMT_ERR_ARG; }
  if (ms) *ms = c->blur_ms;
  if (route_used) *route_used = c->blur_route;
  return GLIA_HMT_OK;
}

}  // extern "C"
