// glia_amd/csrc/median_runs.hpp -- value runs of the median layout (GLIA_USE_MEDIAN_AS_FEATS), shared by median_feats.hip (a given
// merge order) and median_init.hip (the initial edges): the voxel values of an image grouped by leaf, its boundary-voxel values grouped
// by directed leaf pair.  The kernels sit in an unnamed namespace: each of the two files gets its own instance.
#pragma once
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "greedy_common.hpp"

namespace glia {
namespace {

__global__ void mf_gather_u32(const uint32_t* rec, long long n, int words, int word, uint32_t* out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = rec[(size_t)i * words + word];
}

// voxel values grouped by leaf: dst = leaf_off[leaf] + running count (the order inside a leaf does not matter: the sets are sorted)
__global__ void mf_scatter_regions(VolumeRef vol, const float* img, const uint32_t* rlabel, uint32_t R, const unsigned long long* leaf_off, uint32_t* cursor, float* out) {
  const long long N = vol.nx * vol.ny * vol.nz;
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= N) return;
  const uint32_t t = vol.lab[p];
  if (t == kMaskedLabel) return;                          // masked-out centre (point-map mode: util/struct.hxx:86-91)
  const uint32_t leaf = find_label(rlabel, R, t);
  if (leaf >= R || rlabel[leaf] != t) return;
  out[leaf_off[leaf] + atomicAdd(&cursor[leaf], 1u)] = img[p];
}

// boundary-voxel values grouped by directed pair, the neighbour rule of type/neighbor.hxx:109-126 (masked-out neighbours are invalid)
__global__ void mf_scatter_pairs(VolumeRef vol, const float* img, const uint32_t* pa, const uint32_t* pb, long long P, const unsigned long long* off, uint32_t* cursor,
                                 float* out) {
  const long long N = vol.nx * vol.ny * vol.nz;
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= N) return;
  const long long x = p % vol.nx, y = (p / vol.nx) % vol.ny, z = p / (vol.nx * vol.ny);
  const uint32_t t = vol.lab[p];
  if (t == kMaskedLabel) return;
  uint32_t nb = t;
  const long long sy = vol.nx, sz = vol.nx * vol.ny;
  const uint32_t* L = vol.lab_nb;
  do {
    uint32_t q;
    if (x > 0 && (q = L[p - 1]) != t && q != kMaskedLabel) { nb = q; break; }
    if (x + 1 < vol.nx && (q = L[p + 1]) != t && q != kMaskedLabel) { nb = q; break; }
    if (y > 0 && (q = L[p - sy]) != t && q != kMaskedLabel) { nb = q; break; }
    if (y + 1 < vol.ny && (q = L[p + sy]) != t && q != kMaskedLabel) { nb = q; break; }
    if (vol.dim == 3) {
      if (z > 0 && (q = L[p - sz]) != t && q != kMaskedLabel) { nb = q; break; }
      if (z + 1 < vol.nz && (q = L[p + sz]) != t && q != kMaskedLabel) { nb = q; break; }
    }
  } while (false);
  if (nb == t) return;
  const long long i = find_pair(pa, pb, P, t, nb);
  if (i < 0) return;
  out[off[i] + atomicAdd(&cursor[i], 1u)] = img[p];
}

}  // namespace
}  // namespace glia
