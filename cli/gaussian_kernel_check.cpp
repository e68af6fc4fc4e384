// cli/gaussian_kernel_check.cpp -- the discrete Gaussian and the host definition of blur_image alone, without the library and without a
// GPU: glia_amd/csrc/gaussian_kernel.hpp on the known radii of DESIGN 3.18, and on tiny volumes whose extents (1, 2, 3) lie below the
// radius, where every clamped tap has to stay inside the buffer.
//   gaussian_kernel_check     prints the kernels, checks, prints OK
// Built plainly by cli/Makefile; `make gaussian_kernel_check_san` builds it with -fsanitize=address,undefined for a run on the CPU.
#include <cstdio>

#include "../glia_amd/csrc/gaussian_kernel.hpp"

using namespace glia;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "gaussian_kernel_check: line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

template <typename T> static std::vector<T> blur(int dim, std::vector<int64_t> dims, const std::vector<T>& in, double t, int width, int skip) {
  dims.resize(3, 1);
  const double var[3] = {t, t, t};
  std::vector<T> out(in.size());
  blur_image_host(dim, dims.data(), in.data(), var, width, skip, out.data());
  return out;
}

int main() {
  const struct { double t; int width, radius; } known[] = {{1, 3, 3}, {1, 32, 3}, {4, 32, 5}, {0.25, 32, 2}, {0.01, 32, 1}, {9, 5, 5}, {64, 32, 21}, {100, 64, 26}};
  for (const auto& k : known) {
    const GaussianKernel g = gaussian_kernel(k.t, k.width, kBlurMaxError);
    printf("t = %g, max_width = %d: radius %d, covered %.17g\n ", k.t, k.width, g.radius, g.covered);
    double sum = g.c[0];
    for (int i = 0; i <= g.radius; ++i) { printf(" %.17g", g.c[(size_t)i]); if (i) sum += 2.0 * g.c[(size_t)i]; }
    printf("\n");
    EXPECT(g.radius == k.radius && (int)g.c.size() == g.radius + 1);
    EXPECT(std::fabs(sum - 1.0) < 1e-14);
    for (int i = 1; i <= g.radius; ++i) EXPECT(g.c[(size_t)i] > 0.0 && g.c[(size_t)i] < g.c[(size_t)i - 1]);
  }
  EXPECT(std::fabs(gaussian_kernel(1, 32, kBlurMaxError).covered - 0.99777) < 1e-5);
  EXPECT(std::fabs(gaussian_kernel(9, 5, kBlurMaxError).covered - 0.9339) < 1e-4);
  EXPECT(gaussian_kernel(256, 128, kBlurMaxError).radius <= 128 && gaussian_kernel(1e-300, 1, kBlurMaxError).radius == 1);

  // tiny volumes against radius 5 (t = 9 cut at width 5): extents 1, 2 and 3 on every axis, in 3D and 2D, every skip
  const int64_t shapes[][3] = {{1, 1, 1}, {2, 1, 3}, {3, 2, 1}, {1, 3, 2}, {2, 3, 2}, {3, 3, 3}, {7, 2, 1}};
  for (const auto& s : shapes)
    for (int dim = 2; dim <= 3; ++dim)
      for (int skip = -1; skip < dim; ++skip) {
        const size_t n = (size_t)(s[0] * s[1] * (dim == 3 ? s[2] : 1));
        std::vector<float> f(n);
        std::vector<uint8_t> b(n);
        std::vector<uint16_t> w(n);
        for (size_t i = 0; i < n; ++i) { f[i] = (float)(i % 5) * 0.25f; b[i] = (uint8_t)(i * 37); w[i] = (uint16_t)(i % 2 ? 65535 : 0); }
        const std::vector<float> of = blur(dim, {s[0], s[1], s[2]}, f, 9, 5, skip);
        const std::vector<uint8_t> ob = blur(dim, {s[0], s[1], s[2]}, b, 9, 5, skip);
        const std::vector<uint16_t> ow = blur(dim, {s[0], s[1], s[2]}, w, 9, 5, skip);
        for (size_t i = 0; i < n; ++i) EXPECT(of[i] >= 0.0f && of[i] <= 1.0f + 1e-6f);      // a weighted mean of values in [0, 1]
        if (n == 1) EXPECT(ob[0] == b[0] && ow[0] == w[0]);
      }
  // a constant stays the constant: the coefficients sum to 1 within rounding, 0.5 is a power of two
  {
    const std::vector<float> c(3 * 2 * 2, 0.5f);
    for (float v : blur(3, {3, 2, 2}, c, 1, 3, -1)) EXPECT(std::fabs(v - 0.5f) <= 3 * 0x1p-25f);
  }
  // the slice-wise mode in 2D blurs lines: an impulse in a 3 x 1 image with y left alone
  {
    const std::vector<float> line = {0.f, 1.f, 0.f};
    const std::vector<float> o = blur(2, {3, 1}, line, 1, 3, 1);     // 3 x 1, y skipped: a 1D blur along x
    const GaussianKernel g = gaussian_kernel(1, 3, kBlurMaxError);
    EXPECT(o[1] == (float)(0.0 + g.c[3] * 0.0 + g.c[2] * 0.0 + g.c[1] * 0.0 + g.c[0] * 1.0 + g.c[1] * 0.0 + g.c[2] * 0.0 + g.c[3] * 0.0));
    EXPECT(o[0] == o[2]);
  }
  // the integer cast truncates and clamps
  EXPECT(blur_to_integer<uint8_t>(7.75f) == 7 && blur_to_integer<uint8_t>(255.5f) == 255 && blur_to_integer<uint8_t>(-0.5f) == 0);
  EXPECT(blur_to_integer<uint16_t>(65534.996f) == 65534 && blur_to_integer<uint16_t>(70000.0f) == 65535 && blur_to_integer<uint16_t>(0.99f) == 0);
  if (fails) { fprintf(stderr, "gaussian_kernel_check: %d check(s) failed\n", fails); return 1; }
  printf("OK\n");
  return 0;
}
