// cli/libm_exp_check.cpp -- the restatements of glibc's exp (glia_amd/csrc/glibc_math.hpp: exp_sse2, exp_fma) and the sigmoid built on
// them, alone: the header compiled by the host compiler, against THIS host's std::exp, without the library and without a GPU.
//   libm_exp_check      prints which build of exp this host runs and OK, exits 0; or names the failed lines and exits 1
// One of the two restatements must give std::exp bit for bit over the whole range (sampled, plus the special values), the sigmoid of
// that variant must give 1.0 / (1.0 + std::exp(-h)), and the other variant must differ on one of the probe arguments.
// Built plainly by cli/Makefile; `make libm_exp_check_san` builds it with -fsanitize=address,undefined for a run on the CPU.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#define __host__
#define __device__
#define __forceinline__ inline
#include "../glia_amd/csrc/glibc_math.hpp"

using namespace glia;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "libm_exp_check: line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static bool same_bits(double a, double b) { return (a != a && b != b) || memcmp(&a, &b, sizeof(a)) == 0; }
static uint64_t rng_state = 0x243F6A8885A308D3ull;
static double uniform(double lo, double hi) {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return lo + (hi - lo) * ((double)(rng_state >> 11) / 9007199254740992.0);
}
static double host_exp(double x) { volatile double v = x; return std::exp(v); }
static double host_sigmoid(double h) { volatile double v = -h; return 1.0 / (1.0 + std::exp(v)); }

int main() {
  const double inf = std::numeric_limits<double>::infinity();
  const double probe[3] = {0x1.abe9a7aa19388p-1, 0x1.2993abd96c7dp+4, -0x1.31e0da89a5188p-2};
  std::vector<double> xs = {0.0, -0.0, 5e-324, -5e-324, 1e-310, 0x1p-54, -0x1p-54, 0x1p-55, 512.0, -512.0, 709.782712893384, 709.7827128933841,
                            1024.0, -1024.0, 1e308, -1e308, inf, -inf, std::nan(""), -708.4, -745.13321910194122, -745.2, -1023.9};
  for (double p : probe) xs.push_back(p);
  for (int i = 0; i < 400000; ++i) {
    xs.push_back(uniform(-1100.0, 1100.0)); xs.push_back(uniform(-50.0, 50.0)); xs.push_back(uniform(500.0, 720.0)); xs.push_back(-uniform(500.0, 720.0));
    xs.push_back(-uniform(700.0, 760.0));      // results in the subnormal range
  }
  long bad[2] = {0, 0}, bad_sig[2] = {0, 0};
  for (double x : xs) {
    const double h = host_exp(x), s = host_sigmoid(x);
    if (!same_bits(glibc::exp_sse2(x), h)) ++bad[0];
    if (!same_bits(glibc::exp_fma(x), h)) ++bad[1];
    if (!same_bits(glibc::sigmoid(x, 1), s)) ++bad_sig[0];
    if (!same_bits(glibc::sigmoid(x, 2), s)) ++bad_sig[1];
    EXPECT(same_bits(glibc::sigmoid(x, 0), s));      // variant 0 is the libm of whoever runs it: here, the host's
  }
  const int v = bad[1] == 0 ? 2 : bad[0] == 0 ? 1 : 0;
  printf("libm_exp_check: %zu arguments; exp differs from this host's on %ld (non-FMA restatement) / %ld (FMA restatement), the sigmoid on %ld / %ld\n",
         xs.size(), bad[0], bad[1], bad_sig[0], bad_sig[1]);
  EXPECT(v != 0);
  if (v) {
    EXPECT(bad_sig[v - 1] == 0);
    EXPECT(bad[2 - v] > 0);                          // the two builds are different functions ...
    bool told_apart = false;                         // ... and the probe arguments show it
    for (double p : probe) told_apart = told_apart || !same_bits(v == 2 ? glibc::exp_sse2(p) : glibc::exp_fma(p), host_exp(p));
    EXPECT(told_apart);
  }
  // the ends of the range, whatever the build
  for (int w = 1; w <= 2; ++w) {
    EXPECT(glibc::sigmoid(512.0, w) == 1.0 && glibc::sigmoid(inf, w) == 1.0 && glibc::sigmoid(-inf, w) == 0.0 && glibc::sigmoid(-1e308, w) == 0.0);
    EXPECT(glibc::sigmoid(0.0, w) == 0.5 && glibc::sigmoid(std::nan(""), w) != glibc::sigmoid(std::nan(""), w));
  }
  EXPECT(glibc::exp_sse2(inf) == inf && glibc::exp_fma(-inf) == 0.0 && glibc::exp_sse2(710.0) == inf && glibc::exp_fma(-746.0) == 0.0);
  if (fails) return 1;
  printf("libm_exp_check: host exp = variant %d (%s)\nlibm_exp_check: OK\n", v, v == 2 ? "FMA build" : "non-FMA build");
  return 0;
}
