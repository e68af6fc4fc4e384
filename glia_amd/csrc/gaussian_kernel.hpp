// glia_amd/csrc/gaussian_kernel.hpp -- the discrete Gaussian of blur_image on the host: the coefficients of one axis
// and the definition of the whole operator as plain C++.  Host only, no HIP, no library: cli/gaussian_kernel_check.cpp builds on it
// alone; api_blur.cpp exports it (glia_hmt_gaussian_kernel, glia_hmt_blur_image_host) and hands the coefficients to the kernels.
//
// Reference: blurImage (util/image.hxx:376-407) = itk::DiscreteGaussianImageFilter(variance = sigma^2, MaximumKernelWidth), whose
// coefficients come from itk::GaussianOperator: T(n) = exp(-t) I_n(t), accumulated until they cover 1 - MaximumError, cut at the
// maximum width, normalised.  ITK is absent, so the rule below is this project's statement of it: the truncation is ITK's as
// understood (unpinned), the Bessel values are exact to rounding where ITK's are polynomial fits good to about 1e-7.
//
// Every product, quotient and sum is rounded on its own (-ffp-contract=off where this header is compiled).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define GLIA_BLUR_HD __host__ __device__
#else
#define GLIA_BLUR_HD
#endif

namespace glia {

constexpr int kBlurMaxRadius = 128;          // = the largest accepted max_width
constexpr double kBlurMaxVariance = 256.0;
constexpr double kBlurMaxError = 0.01;       // ITK's default MaximumError, what the tools pass

// T(n) = exp(-t) I_n(t): the power series of the modified Bessel function of the first kind in double, operation for operation as
// DESIGN 3.18 lists them (no pow; the one exp is the host's)
inline double discrete_gaussian(int n, double t) {
  const double h = t / 2;
  double term = 1;
  for (int j = 1; j <= n; ++j) term = term * h / j;
  const double hh = h * h;
  double s = 0;
  long long k = 0;
  do {
    s += term;
    k += 1;
    term = term * hh / (double)(k * (k + n));
  } while (!(term < s * 0x1p-60));
  return std::exp(-t) * s;
}

struct GaussianKernel {
  std::vector<double> c;     // one-sided, c[0..radius], normalised by `covered`
  int radius = 0;
  double covered = 0;        // c0 + 2 (c1 + ... + c_radius) before the division: 1 - covered is what the truncation left out
};

// the truncation of itk::GaussianOperator::GenerateCoefficients; variance > 0, max_width >= 1, 0 < max_error < 1 (the caller checks)
inline GaussianKernel gaussian_kernel(double variance, int max_width, double max_error) {
  GaussianKernel g;
  g.c.push_back(discrete_gaussian(0, variance));
  g.c.push_back(discrete_gaussian(1, variance));
  double sum = g.c[0] + 2.0 * g.c[1];
  for (int i = 2; sum < 1.0 - max_error; ++i) {
    const double ti = discrete_gaussian(i, variance);
    g.c.push_back(ti);
    sum += 2.0 * ti;
    if (ti <= 0.0) break;
    if ((int)g.c.size() > max_width) break;
  }
  g.radius = (int)g.c.size() - 1;
  g.covered = sum;
  for (double& v : g.c) v = v / sum;
  return g;
}

// One axis pass, float32 -> float32: out[p] = f32(sum_{o = -r..+r} c[|o|] * (double)in[clamp(p + o e_axis)]), o ascending, the
// accumulator starting at +0.0, coordinates clamped into the volume (zero-flux Neumann).  dims[3] with 1 for an absent axis.
inline void blur_axis_pass_host(const int64_t dims[3], int axis, const GaussianKernel& g, const float* in, float* out) {
  const int64_t nx = dims[0], ny = dims[1], nz = dims[2];
  const int64_t stride = axis == 0 ? 1 : axis == 1 ? nx : nx * ny, extent = dims[axis];
  for (int64_t z = 0; z < nz; ++z)
    for (int64_t y = 0; y < ny; ++y)
      for (int64_t x = 0; x < nx; ++x) {
        const int64_t p = (z * ny + y) * nx + x, at = axis == 0 ? x : axis == 1 ? y : z;
        double acc = 0.0;
        for (int o = -g.radius; o <= g.radius; ++o) {
          int64_t q = at + o;
          q = q < 0 ? 0 : q > extent - 1 ? extent - 1 : q;
          acc = acc + g.c[(size_t)(o < 0 ? -o : o)] * (double)in[p + (q - at) * stride];
        }
        out[p] = (float)acc;
      }
}

// the cast back to an integer pixel type after the last pass: clamped to the type's range, truncated toward zero
template <typename T> GLIA_BLUR_HD inline T blur_to_integer(float v) {
  const float top = sizeof(T) == 1 ? 255.0f : 65535.0f;
  if (!(v > 0.0f)) return (T)0;
  return v >= top ? (T)top : (T)v;
}
template <> GLIA_BLUR_HD inline float blur_to_integer<float>(float v) { return v; }   // float32 pixels: no cast

// The whole operator: x, then y, then z; variance[a] is read for the axes that are blurred (a < dim, a != skip_axis).  Integer pixels
// go to float32 (exact), through the same passes, and back by blur_to_integer; with no axis blurred the output is the input.
template <typename T> inline void blur_image_host(int dim, const int64_t dims_in[3], const T* in, const double variance[3], int max_width,
                                                  int skip_axis, T* out) {
  const int64_t dims[3] = {dims_in[0], dims_in[1], dim == 3 ? dims_in[2] : 1};
  const size_t n = (size_t)(dims[0] * dims[1] * dims[2]);
  std::vector<float> a(n), b(n);
  for (size_t i = 0; i < n; ++i) a[i] = (float)in[i];
  int passes = 0;
  for (int axis = 0; axis < dim; ++axis) {
    if (axis == skip_axis) continue;
    blur_axis_pass_host(dims, axis, gaussian_kernel(variance[axis], max_width, kBlurMaxError), a.data(), b.data());
    a.swap(b);
    ++passes;
  }
  if (!passes) { memcpy(out, in, n * sizeof(T)); return; }
  for (size_t i = 0; i < n; ++i) out[i] = blur_to_integer<T>(a[i]);
}

}  // namespace glia
