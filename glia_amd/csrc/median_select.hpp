// glia_amd/csrc/median_select.hpp -- an order statistic of a multiset given as SIGNED SORTED RUNS of f32 values, without
// materialising it: the set holds every element of the runs with sign +1, minus (as a multiset difference) every element of the runs
// with sign -1, which must be present in it.  That is how the median layout (GLIA_USE_MEDIAN_AS_FEATS, type/feat.hxx:677-722) sees the
// voxel sets of an edge once every leaf's values and every directed pair's boundary values are sorted: P(u + v) = two runs, B(u) =
// the runs leaving u, B(u + v) = B(u) + B(v) - (u -> v) - (v -> u).  stats::amedian (util/stats.hxx:83-91) is the element at rank n / 2.
//
// The selection bisects on the order-preserving 32-bit image of the value: the answer is the smallest key x with
// #{elements <= x} > rank, i.e. sorted[rank] of the materialised set, bit for bit.  The order is the one of the keys, which is the
// order the radix sort leaves the runs in (-0.0 sorts below +0.0, as in median_feats.hip).  Exactly 32 rounds, each one binary search
// per run.  Plain C++ as well as HIP: cli/median_select_check.cpp runs it on the host against std::nth_element.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GLIA_HD __host__ __device__
#else
#define GLIA_HD
#endif

namespace glia {

GLIA_HD inline uint32_t float_ord(float f) {
  uint32_t u = __builtin_bit_cast(uint32_t, f);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
GLIA_HD inline float ord_float(uint32_t o) {
  uint32_t u = o ^ ((o >> 31) ? 0x80000000u : 0xFFFFFFFFu);
  return __builtin_bit_cast(float, u);
}

struct SignedRun { const float* v; unsigned long long n; int sign; };      // sorted ascending by float_ord; sign +1 or -1

// elements of a sorted run whose key is <= key
GLIA_HD inline unsigned long long run_count_le(const float* v, unsigned long long n, uint32_t key) {
  unsigned long long lo = 0, hi = n;
  while (lo < hi) {
    const unsigned long long mid = lo + ((hi - lo) >> 1);
    if (float_ord(v[mid]) <= key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// The element at `rank` (0-based, 0 <= rank < size of the set).  Runs: count() = runs THIS caller looks at, get(i) = SignedRun.
// Sum: the total of one signed count per cooperating caller -- the identity when one caller holds every run (host, one thread), a
// wave reduction when the runs of a set are dealt out to the lanes of a wave (all lanes must then call with the same rank; the
// round count does not depend on the data, so they stay convergent).
template <class Runs, class Sum>
GLIA_HD inline float median_select(const Runs& runs, long long rank, Sum sum) {
  uint32_t lo = 0, hi = 0xFFFFFFFFu;
  const int mine = runs.count();
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    long long c = 0;
    for (int i = 0; i < mine; ++i) {
      const SignedRun r = runs.get(i);
      const long long k = (long long)run_count_le(r.v, r.n, mid);
      c += r.sign < 0 ? -k : k;
    }
    if (sum(c) > rank) hi = mid; else lo = mid + 1;
  }
  return ord_float(lo);
}

struct SelectAlone { GLIA_HD long long operator()(long long c) const { return c; } };
// every run in one array
struct RunList {
  const SignedRun* r; int n;
  GLIA_HD int count() const { return n; }
  GLIA_HD SignedRun get(int i) const { return r[i]; }
};

}  // namespace glia
