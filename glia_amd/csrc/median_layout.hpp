// glia_amd/csrc/median_layout.hpp -- the column walk of GLIA_USE_MEDIAN_AS_FEATS (type/feat.hxx:677-722, 772-808; hmt/bc_feat.hxx:
// 252-268), stated once for the host route (glia_hmt_bc_feat, api_loops.cpp) and the device kernel (bc_init_score_median, greedy_bc.hip).
// One more column per real-feature block: ImageRealFeats = [histogram] entropy | MEDIAN mean std | min max with mean and standard
// deviation taken from the value vector, ImageDiffFeats = l1 x2 |d entropy| |d MEDIAN| |d mean| |d std| |d min| |d max|; the simple
// selection carries the shared boundary's median beside its mean.
#pragma once
#include "bc_features.hpp"

namespace glia {

// columns the layout adds to a vector of c.fdim columns
__host__ __device__ inline int median_extra_cols(const BcCfg& c) { return c.use_simple ? c.n_boundary : 4 * c.n_region + 4 * c.n_boundary; }

// in: the finished statistics-based vector (c.fdim columns, x1 / x2 as the feature code ordered them); out: the median layout
// (c.fdim + median_extra_cols(c) columns, must not overlap in).  rs(blk, i, q) / bs(blk, i, q): statistic q = median | mean | stddev
// of region-list / boundary-list image i over block blk = x1 | x2 | the merged region (| 3: the shared boundary, bs only).
// Returns the columns written, or -1 when the walk does not end at both vectors' ends (a layout error, never expected).
template <class RS, class BS>
__host__ __device__ inline int median_splice(const BcCfg& c, const double* in, double* out, RS rs, BS bs) {
  const int nr = c.n_region, nl = c.n_rlabel, nb = c.n_boundary, T = c.T, D = c.D;
  auto hb = [&](int kind, int i) { return c.use_hist ? c.cbins[kind == 0 ? c.rc[i] : kind == 1 ? c.lc[i] : c.bc[i]] : 0; };
  int p = 0, k = 0;
  if (c.use_simple) {                                         // hmt/bc_feat.hxx:247-279
    for (int q = 0; q < 5; ++q) out[k++] = in[p++];
    for (int j = 0; j < nb; ++j) { out[k++] = bs(3, j, 1); out[k++] = bs(3, j, 0); ++p; }
    for (int j = 0; j < nr; ++j) { out[k++] = __builtin_fabs(rs(0, j, 1) - rs(1, j, 1)); out[k++] = in[p + 1]; out[k++] = in[p + 2]; out[k++] = in[p + 3]; p += 4; }
    for (int j = 0; j < 2 * nl; ++j) out[k++] = in[p++];
  } else {
    for (int q = 0; q < 11 + 4 * T; ++q) out[k++] = in[p++];
    for (int j = 0; j < nr; ++j) {                               // feat.hxx:782-808: l1, x2, |d entropy|, |d median|, |d mean|, |d std|, |d min|, |d max|
      out[k++] = in[p]; out[k++] = in[p + 1]; out[k++] = in[p + 2];
      out[k++] = __builtin_fabs(rs(0, j, 0) - rs(1, j, 0)); out[k++] = __builtin_fabs(rs(0, j, 1) - rs(1, j, 1)); out[k++] = __builtin_fabs(rs(0, j, 2) - rs(1, j, 2));
      out[k++] = in[p + 5]; out[k++] = in[p + 6];
      p += 7;
    }
    for (int q = 0; q < 3 * nl; ++q) out[k++] = in[p++];
    auto real_block = [&](int h, double med, double mean, double sd) {     // [histogram] entropy | median mean std | min max
      for (int q = 0; q < h + 1; ++q) out[k++] = in[p++];
      out[k++] = med; out[k++] = mean; out[k++] = sd;
      out[k++] = in[p + 2]; out[k++] = in[p + 3];
      p += 4;
    };
    for (int j = 0; j < nb; ++j) real_block(hb(2, j), bs(3, j, 0), bs(3, j, 1), bs(3, j, 2));
    for (int blk = 0; blk < 3; ++blk) {
      for (int q = 0; q < 4 + D + 2 * T; ++q) out[k++] = in[p++];
      for (int j = 0; j < nr; ++j) real_block(hb(0, j), rs(blk, j, 0), rs(blk, j, 1), rs(blk, j, 2));
      for (int j = 0; j < nl; ++j) for (int q = 0; q < hb(1, j) + 1; ++q) out[k++] = in[p++];
      for (int j = 0; j < nb; ++j) real_block(hb(2, j), bs(blk, j, 0), bs(blk, j, 1), bs(blk, j, 2));
    }
  }
  return (p == c.fdim && k == c.fdim + median_extra_cols(c)) ? k : -1;
}

}  // namespace glia
