// glia_amd/csrc/eval.cpp -- the numbers of eval_ri and eval_vi (gadget/main_eval_ri.cxx, gadget/main_eval_vi.cxx) from contingency tables.
//
// The device counts c(a, b), the voxels with proposed label a and reference label b that the caller's filter keeps
// (label_overlap.hip).  Everything below is host code with no HIP call: it includes nothing of the runtime, so it also builds with a
// plain host compiler.  Per table, with n_a = sum_b c(a, b), n_b = sum_a c(a, b), n = sum c:
//   stats::pairStats (util/stats.hxx:189-229)    TP = sum c (c - 1) / 2                       :205
//                                                nPair = n (n - 1) / 2                        :207
//                                                key1 = sum_b n_b (n_b - 1) / 2               :209-216
//                                                key0 = sum_a n_a (n_a - 1) / 2               :217-224
//                                                TN = nPair - key1 + TP - key0, FP = key0 - TP, FN = key1 - TP      :225-228
//   stats::centropy (util/image_stats.hxx:122-158), image0 = the conditioning image:
//                                                H(a | b) = sum c(a, b) log2(n_b / c(a, b)) / n     :148-157
// eval_ri adds the four counts of all image pairs and then takes the ratios (main_eval_ri.cxx:41-59); eval_vi takes stats::mean of
// the per-pair entropies (main_eval_vi.cxx:23-27; util/stats.hxx:38-58).
//
// The quotient of :153 is `up.second / bp.second` on two `uint`s: an integer division.  kReference restates that; kExact divides
// in double.  Sums run in entry order; the reference's run in unordered_map order, so its own last bits are not pinned.
// Integers are exact (128 bits: a table's n (n - 1) / 2 stays below 2^63 for n < 2^32, and the sums over tables fit).  A count
// above 2^53 converted to double rounds to nearest; the reference converts Boost's int512_t, whose rounding is not pinned.
#include <cmath>
#include <cstdint>
#include <string>
#include <unordered_map>

#include "../../include/glia_hmt.h"

namespace glia {

void set_error(const std::string& msg);                              // api.cpp

namespace {

constexpr double kFEPS = 2.22e-16;                                   // glia_base.hxx:57
inline bool isfeq(double a, double b) { return std::fabs(a - b) < kFEPS; }   // glia_base.hxx:71-72
inline double sdivide(double lhs, double rhs, double dummy) { return std::fabs(rhs) >= kFEPS ? lhs / rhs : dummy; }   // glia_base.hxx:77-78
typedef unsigned __int128 U128;

inline U128 pairs_of(U128 n) { return n ? n * (n - 1) / 2 : 0; }
inline void split(U128 v, uint64_t* lo, uint64_t* hi) { *lo = (uint64_t)v; *hi = (uint64_t)(v >> 64); }

}  // namespace

int overlap_scores(const glia_hmt_overlap_entry* const* tables, const int64_t* n_entries, int n_tables, int vi_mode, glia_hmt_eval_result* out) {
  U128 TP = 0, TN = 0, FP = 0, FN = 0;
  double fs_sum = 0.0, fm_sum = 0.0;                                 // stats::sum: from 0.0, in image order (util/stats.hxx:38-44)
  for (int t = 0; t < n_tables; ++t) {
    const glia_hmt_overlap_entry* e = tables[t];
    const int64_t E = n_entries[t];
    std::unordered_map<uint32_t, U128> na, nb;
    na.reserve((size_t)E); nb.reserve((size_t)E);
    U128 n = 0, tp = 0;
    for (int64_t i = 0; i < E; ++i) {
      if (e[i].count == 0) { set_error("eval: table " + std::to_string(t) + " entry " + std::to_string(i) + " has count 0"); return GLIA_HMT_ERR_ARG; }
      const U128 c = e[i].count;
      n += c; tp += pairs_of(c);
      na[e[i].a] += c; nb[e[i].b] += c;
    }
    U128 key0 = 0, key1 = 0;
    for (const auto& p : na) key0 += pairs_of(p.second);
    for (const auto& p : nb) key1 += pairs_of(p.second);
    TP += tp;
    TN += pairs_of(n) - key1 + tp - key0;
    FP += key0 - tp;
    FN += key1 - tp;
    // centropy(ref, res, mask, {BG_VAL}, {}) = H(a | b), centropy(res, ref, mask, {}, {BG_VAL}) = H(b | a) (main_eval_vi.cxx:23-24)
    double fs = 0.0, fm = 0.0;
    for (int64_t i = 0; i < E; ++i) {
      const uint64_t c = e[i].count, mb = (uint64_t)nb[e[i].b], ma = (uint64_t)na[e[i].a];
      if (vi_mode == GLIA_HMT_VI_REFERENCE) {
        fs += (double)c * std::log2((double)(mb / c));
        fm += (double)c * std::log2((double)(ma / c));
      } else {
        fs += (double)c * std::log2((double)mb / (double)c);
        fm += (double)c * std::log2((double)ma / (double)c);
      }
    }
    fs_sum += fs / (double)n;                                        // `ret / n`: 0.0 / 0 = NaN when no voxel is selected (:157)
    fm_sum += fm / (double)n;
  }
  split(TP, &out->tp_lo, &out->tp_hi); split(TN, &out->tn_lo, &out->tn_hi);
  split(FP, &out->fp_lo, &out->fp_hi); split(FN, &out->fn_lo, &out->fn_hi);
  double den = (double)(TP + FP);                                    // stats::precision (util/stats.hxx:243-248)
  out->precision = (double)TP / (!isfeq(den, 0.0) ? den : (den + kFEPS));
  den = (double)(TP + FN);                                           // stats::recall (:251-256)
  out->recall = (double)TP / (!isfeq(den, 0.0) ? den : (den + kFEPS));
  out->f1 = 2.0 * out->precision * out->recall / (out->precision + out->recall);     // stats::f1 (:259-261): 0 / 0 = NaN
  const double num = (double)(TP + TN);                              // stats::randIndex (:232-240)
  den = (double)(FP + FN);
  den += num;
  out->rand_index = num / (!isfeq(den, 0.0) ? den : (den + kFEPS));
  out->false_split = sdivide(fs_sum, (double)n_tables, 0.0);         // stats::mean (:56-58)
  out->false_merge = sdivide(fm_sum, (double)n_tables, 0.0);
  return GLIA_HMT_OK;
}

}  // namespace glia

extern "C" int glia_hmt_overlap_scores(const glia_hmt_overlap_entry* const* h_tables, const int64_t* n_entries, int n_tables, int vi_mode,
                                       glia_hmt_eval_result* out) {
  auto bad = [](const std::string& what) { glia::set_error("eval: " + what); return GLIA_HMT_ERR_ARG; };
  if (!h_tables || !n_entries || !out) return bad("the tables, their lengths and out must not be NULL");
  if (n_tables < 1) return bad("at least one table");
  if (vi_mode != GLIA_HMT_VI_REFERENCE && vi_mode != GLIA_HMT_VI_EXACT) return bad("vi_mode must be GLIA_HMT_VI_REFERENCE or GLIA_HMT_VI_EXACT");
  for (int t = 0; t < n_tables; ++t) {
    if (n_entries[t] < 0) return bad("negative length of table " + std::to_string(t));
    if (n_entries[t] > 0 && !h_tables[t]) return bad("table " + std::to_string(t) + " is NULL");
  }
  return glia::overlap_scores(h_tables, n_entries, n_tables, vi_mode, out);
}
