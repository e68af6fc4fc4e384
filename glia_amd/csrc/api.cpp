// glia_amd/csrc/api.cpp -- C ABI of libglia_hmt.so (see include/glia_hmt.h for the reference operators each entry point replaces):
// errors, options, the libm probe, the context and the small entry points.  The region-map handle is api_rag.cpp, the entry points
// that run a loop or consume a merge order are api_loops.cpp.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <unordered_map>

#include "rmap_order.hpp"
#include "api_types.hpp"

namespace glia {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }

// ---- options ------------------------------------------------------------------------------------------------------------
// Tuning and test switches of the loops (which queue, window size, baseline interval, helper count, instance tier ...).  One
// process-wide table, set through glia_hmt_set_option(); it starts from the environment variables of the same names, read ONCE
// when the table is first used -- no entry point calls getenv() per call.
static const char* const kOptionKeys[] = {"GLIA_HMT_PB_WINDOW", "GLIA_HMT_PB_BATCH", "GLIA_HMT_WINCAP", "GLIA_HMT_REBASE", "GLIA_HMT_HORIZON",
                                          "GLIA_HMT_FORCE_TREE", "GLIA_HMT_HELPERS", "GLIA_HMT_TRACE", "GLIA_HMT_LIBM", "GLIA_HMT_BC_NOCOMMON",
                                          "GLIA_HMT_BC_GENERIC", "GLIA_HMT_DEBUG", "GLIA_HMT_MAXITERS", "GLIA_HMT_MINCAP", "GLIA_HMT_MEDIAN_BATCH", "GLIA_HMT_BCFEAT", "GLIA_HMT_CC",
                                          "GLIA_HMT_TRAIN_TREES", "GLIA_HMT_BASELINE_AUDIT", "GLIA_HMT_COLLECT_LANES", "GLIA_HMT_REBASE_END", "GLIA_HMT_BATCH", "GLIA_HMT_BLUR"};
static std::mutex g_opt_mu;
static std::unordered_map<std::string, std::string> g_opt;
static bool g_opt_init = false;
static void opt_init_locked() {
  if (g_opt_init) return;
  for (const char* k : kOptionKeys) if (const char* e = getenv(k)) g_opt[k] = e;
  g_opt_init = true;
}
static bool opt_known(const char* key) { for (const char* k : kOptionKeys) if (!strcmp(k, key)) return true; return false; }
bool option(const char* key, std::string* value) {
  std::lock_guard<std::mutex> lock(g_opt_mu);
  opt_init_locked();
  auto it = g_opt.find(key);
  if (it == g_opt.end()) return false;
  if (value) *value = it->second;
  return true;
}
int set_option(const char* key, const char* value) {
  if (!key || !opt_known(key)) { set_error(std::string("set_option: unknown option ") + (key ? key : "(null)")); return GLIA_HMT_ERR_ARG; }
  std::lock_guard<std::mutex> lock(g_opt_mu);
  opt_init_locked();
  if (value) g_opt[key] = value; else g_opt.erase(key);
  return GLIA_HMT_OK;
}

float ceil_f32(double d) {   // smallest float >= d
  if (std::isinf(d) || std::isnan(d)) return (float)d;
  float f = (float)d;
  if ((double)f < d) f = std::nextafterf(f, std::numeric_limits<float>::infinity());
  return f;
}
static float floor_f32(double d) {  // largest float <= d
  if (std::isinf(d) || std::isnan(d)) return (float)d;
  float f = (float)d;
  if ((double)f > d) f = std::nextafterf(f, -std::numeric_limits<float>::infinity());
  return f;
}
uint32_t next_pow2(uint64_t v) {
  uint64_t p = 1;
  while (p < v) p <<= 1;
  return (uint32_t)std::min<uint64_t>(p, 1ull << 31);
}

// util/image_stats.hxx:17-22: bounds[0] = interval (range.first ignored), bounds[i] = bounds[i-1] + interval
HistSpec make_hist_spec(int bins, double lo, double hi) {
  HistSpec h;
  h.bins = bins;
  double interval = (hi - lo) / bins;
  double b = 0.0;
  for (int i = 0; i < GLIA_HMT_MAX_BINS; ++i) {
    if (i < bins) { b = (i == 0) ? interval : b + interval; h.fb[i] = ceil_f32(b); }
    else h.fb[i] = std::numeric_limits<float>::infinity();
  }
  h.lo_f = floor_f32(lo);
  h.hi_f = ceil_f32(hi);
  return h;
}

// Which restatement of glibc's log2 / log reproduces THIS host's libm bit for bit (the reference calls std::log2 in
// stats::entropy, util/stats.hxx:150, and std::log in slog, glia_base.hxx:80-81; the device must return the same bits).
// Probe vector: histogram fractions c/n, values around 1 (the near-one branch), and a sweep over exponents.
static LibmSel probe_host_libm() {
  std::vector<double> xs;
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
  for (int i = 0; i < 6000; ++i) { const uint64_t n = 1 + next() % 100000, c = 1 + next() % n; xs.push_back((double)c / (double)n); }
  for (int i = 0; i < 3000; ++i) xs.push_back(1.0 + ((double)(int64_t)(next() % 2000001) - 1000000.0) * 1e-7);
  for (int i = 0; i < 3000; ++i) xs.push_back(std::ldexp(1.0 + (double)(next() >> 12) * 0x1p-52, (int)(next() % 120) - 60));
  for (int e = -1074; e < 1024; e += 37) xs.push_back(std::ldexp(1.0, e));
  LibmSel sel = {kLibmDevice, kLibmDevice, kLibmDevice, kLibmDevice};
  bool l2 = true, ls = true, lf = true, ps = true, pf = true, es = true, ef = true;
  for (double x : xs) {
    volatile double vx = x;
    const double h2 = std::log2(vx), h1 = std::log(vx);
    l2 = l2 && glibc::as_u64(h2) == glibc::as_u64(glibc::log2_sse2(x));
    ls = ls && glibc::as_u64(h1) == glibc::as_u64(glibc::log_sse2(x));
    lf = lf && glibc::as_u64(h1) == glibc::as_u64(glibc::log_fma(x));
  }
  // std::pow(perim, 1.5) of the compactness feature (type/feat.hxx:78-79): integer perimeters, small and large
  for (int i = 0; i < 12000; ++i) {
    const double x = i < 4000 ? (double)(i + 1) : (double)(1 + next() % (i < 8000 ? (1ull << 24) : (1ull << 40)));
    volatile double vx = x, vy = 1.5;
    const uint64_t h = glibc::as_u64(std::pow(vx, vy));
    ps = ps && h == glibc::as_u64(glibc::pow_sse2(x, 1.5));
    pf = pf && h == glibc::as_u64(glibc::pow_fma(x, 1.5));
  }
  // std::exp of the MLP's sigmoid (alg/nn.hxx; mlp_model.hpp): logits and their negatives over the range a sigmoid resolves, the
  // special-cased range beyond 512, and three arguments on which the two builds are known to differ
  {
    std::vector<double> es_x = {0x1.abe9a7aa19388p-1, 0x1.2993abd96c7dp+4, -0x1.31e0da89a5188p-2, 0.0, -0.0, 0x1p-54, -0x1p-55, 512.0, -512.0,
                                709.782712893384, 710.0, -745.2, -1024.0, 1e308};
    for (int i = 0; i < 6000; ++i) es_x.push_back(((double)(int64_t)(next() % 100000001) - 50000000.0) * 1e-6);      // [-50, 50]
    for (int i = 0; i < 3000; ++i) es_x.push_back(((double)(int64_t)(next() % 2000001) - 1000000.0) * 1e-3);         // [-1000, 1000]
    for (int i = 0; i < 3000; ++i) es_x.push_back((i & 1 ? -1.0 : 1.0) * (500.0 + (double)(next() % 2200001) * 1e-4)); // +-[500, 720]
    for (double x : es_x) {
      volatile double vx = x;
      const uint64_t h = glibc::as_u64(std::exp(vx));
      es = es && h == glibc::as_u64(glibc::exp_sse2(x));
      ef = ef && h == glibc::as_u64(glibc::exp_fma(x));
    }
  }
  if (ef) sel.exp_variant = kLibmFma; else if (es) sel.exp_variant = kLibmSse2;
  if (l2) sel.log2_variant = kLibmSse2;
  if (lf) sel.log_variant = kLibmFma; else if (ls) sel.log_variant = kLibmSse2;
  if (pf) sel.pow_variant = kLibmFma; else if (ps) sel.pow_variant = kLibmSse2;
  return sel;
}
// What a context uses: the probe's answer (taken once per process), unless GLIA_HMT_LIBM = device | sse2 | fma overrides the choice
// (tests).  The override is read at EVERY context creation and probe call, not only at the process's first: a test makes a context
// for each family in one process.
static LibmSel host_libm() {
  static const LibmSel probed = probe_host_libm();
  LibmSel sel = probed;
  std::string ov;
  if (option("GLIA_HMT_LIBM", &ov)) {
    const char* e = ov.c_str();
    const int v = !strcmp(e, "sse2") ? kLibmSse2 : !strcmp(e, "fma") ? kLibmFma : kLibmDevice;
    sel.log_variant = v; sel.log2_variant = v == kLibmFma ? kLibmSse2 : v; sel.pow_variant = v; sel.exp_variant = v;
  }
  return sel;
}

}  // namespace glia

static std::atomic<int> g_live_contexts{0};

extern "C" {

const char* glia_hmt_last_error(void) { return g_err.c_str(); }
const char* glia_hmt_version(void) { return "glia_hmt 0.1 (gfx950)"; }

int glia_hmt_ctx_create(int device, void* hip_stream, glia_hmt_ctx** out) {
  if (!out) { set_error("ctx_create: out is NULL"); return GLIA_HMT_ERR_ARG; }
  int n = 0;
  GLIA_HIP_TRY(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) { set_error("ctx_create: no such HIP device"); return GLIA_HMT_ERR_ARG; }
  GLIA_HIP_TRY(hipSetDevice(device));
  glia_hmt_ctx* c = new glia_hmt_ctx;
  c->device = device;
  ++g_live_contexts;
  const int rc = [&]() -> int {
    if (hip_stream) c->stream = (hipStream_t)hip_stream;
    else { GLIA_HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->own_stream = true; }
    GLIA_HIP_TRY(hipMalloc(&c->flags, 256));      // 8 status words + profiling counters of the accumulation pass (profiling builds)
    GLIA_HIP_TRY(hipMemsetAsync(c->flags, 0, 256, c->stream));
    GLIA_HIP_TRY(hipEventCreate(&c->ev0));
    GLIA_HIP_TRY(hipEventCreate(&c->ev1));
    return GLIA_HMT_OK;
  }();
  if (rc) { glia_hmt_ctx_destroy(c); return rc; }      // (destroys what exists: every member starts out null)
  const LibmSel sel = host_libm();
  c->libm = sel;
  *out = c;
  // The call succeeds either way; a host libm none of the restatements reproduces is reported through glia_hmt_last_error()
  // (and glia_hmt_ctx_libm_status): entropy, --logs and compactness columns are then within 1 ulp of the host's, not pinned.
  if (sel.log2_variant == 0 || sel.log_variant == 0 || sel.pow_variant == 0)
    set_error(std::string("warning: the host libm's ") + (sel.log2_variant == 0 ? "log2 " : "") + (sel.log_variant == 0 ? "log " : "") +
              (sel.pow_variant == 0 ? "pow " : "") + "is not reproduced bit for bit by a restatement (glibc 2.35 FMA / non-FMA builds): "
              "the entropy / log / compactness feature columns are within 1 ulp of this host's values, unpinned; equal classifier scores may order differently");
  return GLIA_HMT_OK;
}

int glia_hmt_ctx_libm(const glia_hmt_ctx* c, int* log2_variant, int* log_variant) {
  if (!c) return GLIA_HMT_ERR_ARG;
  if (log2_variant) *log2_variant = c->libm.log2_variant;
  if (log_variant) *log_variant = c->libm.log_variant;
  return GLIA_HMT_OK;
}

int glia_hmt_ctx_libm_status(const glia_hmt_ctx* c) {
  if (!c) return GLIA_HMT_ERR_ARG;
  return (c->libm.log2_variant != 0 && c->libm.log_variant != 0 && c->libm.pow_variant != 0) ? 1 : 0;
}

int glia_hmt_ctx_libm_pow(const glia_hmt_ctx* c, int* pow_variant) {
  if (!c || !pow_variant) return GLIA_HMT_ERR_ARG;
  *pow_variant = c->libm.pow_variant;
  return GLIA_HMT_OK;
}

int glia_hmt_ctx_libm_exp(const glia_hmt_ctx* c, int* exp_variant) {
  if (!c || !exp_variant) return GLIA_HMT_ERR_ARG;
  *exp_variant = c->libm.exp_variant;
  return GLIA_HMT_OK;
}

int glia_hmt_host_libm_probe_exp(int* exp_variant) {
  if (!exp_variant) return GLIA_HMT_ERR_ARG;
  *exp_variant = host_libm().exp_variant;
  return GLIA_HMT_OK;
}

int glia_hmt_host_libm_probe_pow(int* pow_variant) {
  if (!pow_variant) return GLIA_HMT_ERR_ARG;
  *pow_variant = host_libm().pow_variant;
  return GLIA_HMT_OK;
}

int glia_hmt_host_rmap_ranks(const uint32_t* labels, const int64_t* first_voxel, int64_t n, int mode, uint32_t* rank) {
  if (!labels || !first_voxel || !rank || n < 0 || mode < 0 || mode > 2) { set_error("host_rmap_ranks: invalid argument"); return GLIA_HMT_ERR_ARG; }
  std::vector<uint32_t> lab(labels, labels + n), out;
  std::vector<long long> first(first_voxel, first_voxel + n);
  for (int64_t i = 1; i < n; ++i) if (lab[i] <= lab[i - 1]) { set_error("host_rmap_ranks: labels must be ascending"); return GLIA_HMT_ERR_ARG; }
  rmap_ranks(lab, first, &out, mode);
  std::copy(out.begin(), out.end(), rank);
  return GLIA_HMT_OK;
}

int glia_hmt_host_libm_probe(int* log2_variant, int* log_variant) {
  const LibmSel sel = host_libm();
  if (log2_variant) *log2_variant = sel.log2_variant;
  if (log_variant) *log_variant = sel.log_variant;
  return GLIA_HMT_OK;
}

int glia_hmt_host_libm_eval(int function, int variant, const double* h_in, double* h_out, int64_t n) {
  if (!h_in || !h_out || n < 0 || function < 0 || function > 4 || (variant != kLibmSse2 && variant != kLibmFma)) {
    set_error("host_libm_eval: invalid argument");
    return GLIA_HMT_ERR_ARG;
  }
  for (int64_t i = 0; i < n; ++i) {
    const double x = h_in[i];
    if (function == 3) h_out[i] = variant == kLibmFma ? glibc::exp_fma(x) : glibc::exp_sse2(x);
    else if (function == 4) h_out[i] = glibc::sigmoid(x, variant);
    else if (function == 2) h_out[i] = !glibc::pow_in_domain(x, 1.5) ? std::pow(x, 1.5) : variant == kLibmFma ? glibc::pow_fma(x, 1.5) : glibc::pow_sse2(x, 1.5);
    else h_out[i] = function == 0 ? glibc::log2_sse2(x) : variant == kLibmFma ? glibc::log_fma(x) : glibc::log_sse2(x);
  }
  return GLIA_HMT_OK;
}

int glia_hmt_libm_eval(glia_hmt_ctx* c, int function, int variant, const double* d_in, double* d_out, int64_t n) {
  if (!c || !d_in || !d_out || n < 0 || function < 0 || function > 4) { set_error("libm_eval: invalid argument"); return GLIA_HMT_ERR_ARG; }
  GLIA_HIP_TRY(hipSetDevice(c->device));
  return launch_libm_eval(function, variant, d_in, d_out, n, c->stream);
}

unsigned long long glia_hmt_release_cached_memory(void) { return (unsigned long long)glia::BlockCache::get().trim(); }
unsigned long long glia_hmt_internal_errors(void) { return glia::internal_errors(); }
int glia_hmt_set_option(const char* key, const char* value) { return glia::set_option(key, value); }
int glia_hmt_check_merge_order(const uint32_t* h_order, int64_t n_merges, int64_t n_regions, int64_t* first_bad) {
  if ((!h_order && n_merges) || n_merges < 0 || n_regions < 0 || n_regions > 0x7FFFFFFFll) { set_error("check_merge_order: invalid argument"); return GLIA_HMT_ERR_ARG; }
  int64_t bad = -1;
  if (glia::merge_order_is_consistent(h_order, n_merges, (uint32_t)n_regions, &bad)) { if (first_bad) *first_bad = -1; return GLIA_HMT_OK; }
  if (first_bad) *first_bad = bad;
  set_error("check_merge_order: merge " + std::to_string(bad) + " joins a region that does not exist (any more) or creates the wrong one");
  return GLIA_HMT_ERR_ARG;
}

void glia_hmt_ctx_destroy(glia_hmt_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  (void)free_tables(c);
  if (c->flags) (void)hipFree(c->flags);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->own_stream) (void)hipStreamDestroy(c->stream);
  delete c;
  if (--g_live_contexts <= 0) (void)glia::BlockCache::get().trim();      // nobody left to reuse the parked blocks
}

int glia_hmt_ctx_sync(glia_hmt_ctx* c) {
  if (!c) return GLIA_HMT_ERR_ARG;
  GLIA_HIP_TRY(hipStreamSynchronize(c->stream));
  return GLIA_HMT_OK;
}

int glia_hmt_ctx_set_table_hint(glia_hmt_ctx* c, int64_t expected_regions, int64_t expected_pairs) {
  if (!c) return GLIA_HMT_ERR_ARG;
  c->hint_rcap = expected_regions > 0 ? next_pow2((uint64_t)expected_regions * 2) : 0;
  c->hint_pcap = expected_pairs > 0 ? next_pow2((uint64_t)expected_pairs * 2) : 0;
  return GLIA_HMT_OK;
}

int glia_hmt_synth(glia_hmt_ctx* c, int dim, const int64_t dims[3], int S, int G, uint64_t seed, int variant,
                   uint32_t* d_labels, float* d_pb) {
  if (!c || !dims || !d_labels || !d_pb || (dim != 2 && dim != 3) || S <= 0 || G <= 0) {
    set_error("synth: invalid argument");
    return GLIA_HMT_ERR_ARG;
  }
  GLIA_HIP_TRY(hipSetDevice(c->device));
  int64_t N = dims[0] * dims[1] * (dim == 3 ? dims[2] : 1);
  OwnedArrays own;
  uint32_t* d_truth = nullptr;
  int rc = own.alloc(&d_truth, (size_t)N);
  if (rc == GLIA_HMT_OK) rc = launch_synth(dim, dims, S, G, seed, variant, d_labels, d_truth, d_pb, c->stream);
  if (rc == GLIA_HMT_OK) GLIA_HIP_TRY(hipStreamSynchronize(c->stream));
  return rc;
}

int glia_hmt_watershed(glia_hmt_ctx* c, int dim, const int64_t dims[3], const float* d_image, double level, uint32_t* d_labels, uint32_t* n_labels,
                       int* sweeps) {
  if (!c || !dims || !d_image || !d_labels || (dim != 2 && dim != 3) || !(level >= 0.0)) { set_error("watershed: invalid argument"); return GLIA_HMT_ERR_ARG; }
  GLIA_HIP_TRY(hipSetDevice(c->device));
  return watershed_labels(dim, dims, d_image, level, d_labels, n_labels, sweeps, c->stream);
}

// labelIdentityConnectedComponents / labelConnectedComponents (util/image.hxx:331-373, :302-313); every test below comes before the
// first HIP call
int glia_hmt_label_components(glia_hmt_ctx* c, int dim, const int64_t dims[3], const uint32_t* d_labels_in, const uint32_t* d_mask, int mode,
                              uint32_t* d_labels_out, uint32_t* n_components) {
  auto bad = [](const char* what) { set_error(std::string("label_components: ") + what); return GLIA_HMT_ERR_ARG; };
  if (!c || !dims || !d_labels_in || !d_labels_out || !n_components) return bad("ctx, dims, the two volumes and n_components must not be NULL");
  if (dim != 2 && dim != 3) return bad("dim must be 2 or 3");
  const uint64_t most = 0xFFFFFFFEull;                 // 2^32 - 2: 32-bit voxel indices and one free value
  uint64_t n = 1;
  for (int i = 0; i < dim; ++i) {
    if (dims[i] <= 0) return bad("extents must be positive");
    if ((uint64_t)dims[i] > most / n) return bad("between 1 and 2^32 - 2 voxels");
    n *= (uint64_t)dims[i];
  }
  if (mode < GLIA_HMT_CC_IDENTITY || mode > GLIA_HMT_CC_BINARY_INVERTED) return bad("mode must be 0 (identity), 1 (binary) or 2 (binary, inverted)");
  if (d_labels_out == d_labels_in) return bad("the volume cannot be labelled in place");
  int route = GLIA_HMT_CC_ROUTE_TILED;
  std::string v;
  if (option("GLIA_HMT_CC", &v) && v != "tiled") {
    if (v != "global") return bad(("GLIA_HMT_CC must be tiled or global, not '" + v + "'").c_str());
    route = GLIA_HMT_CC_ROUTE_GLOBAL;
  }
  GLIA_HIP_TRY(hipSetDevice(c->device));
  return label_components(dim, dims, d_labels_in, d_mask, mode, route, d_labels_out, n_components, c->stream);
}

// the shared table of stats::pairStats / centropy / getOverlap on images (util/image_stats.hxx:122-158,248-273,308-335); every test
// comes before the first HIP call
static int overlap_args(const char* who, const glia_hmt_ctx* c, const uint32_t* d_a, const uint32_t* d_b, int64_t n_voxels) {
  auto bad = [&](const char* what) { set_error(std::string(who) + ": " + what); return GLIA_HMT_ERR_ARG; };
  if (!c) return bad("ctx must not be NULL");
  if (!d_a || !d_b) return bad("the two label volumes must not be NULL");
  if (n_voxels < 1 || (uint64_t)n_voxels > 0xFFFFFFFEull) return bad("between 1 and 2^32 - 2 voxels");
  return GLIA_HMT_OK;
}

int glia_hmt_label_overlap(glia_hmt_ctx* c, const uint32_t* d_a, const uint32_t* d_b, const uint32_t* d_mask, int64_t n_voxels, int flags,
                           glia_hmt_overlap_entry* h_entries, int64_t capacity, int64_t* n_entries) {
  auto bad = [](const char* what) { set_error(std::string("label_overlap: ") + what); return GLIA_HMT_ERR_ARG; };
  if (int rc = overlap_args("label_overlap", c, d_a, d_b, n_voxels)) return rc;
  if (!n_entries) return bad("n_entries must not be NULL");
  if (capacity < 0 || (capacity > 0 && !h_entries)) return bad("h_entries must hold `capacity` >= 0 entries");
  if (flags & ~(GLIA_HMT_OVERLAP_DROP_ZERO_A | GLIA_HMT_OVERLAP_DROP_ZERO_B)) return bad("unknown flag bits");
  GLIA_HIP_TRY(hipSetDevice(c->device));
  std::vector<glia_hmt_overlap_entry> table;
  OverlapPass pass;
  if (int rc = label_overlap(d_a, d_b, d_mask, (unsigned long long)n_voxels, flags, c->stream, &table, &pass)) return rc;
  c->evt = glia_hmt_eval_timing{pass.ms, (int64_t)table.size(), pass.repeats};
  *n_entries = (int64_t)table.size();
  if ((int64_t)table.size() > capacity) { set_error("label_overlap: " + std::to_string(table.size()) + " entries, capacity " + std::to_string(capacity)); return GLIA_HMT_ERR_CAPACITY; }
  std::copy(table.begin(), table.end(), h_entries);
  return GLIA_HMT_OK;
}

// operation() of gadget/main_eval_ri.cxx:9-61 and gadget/main_eval_vi.cxx:7-29: excluded0 = {}, excluded1 = {BG_VAL}
int glia_hmt_eval(glia_hmt_ctx* c, int n_images, const uint32_t* const* d_res, const uint32_t* const* d_ref, const uint32_t* const* d_mask,
                  const int64_t* n_voxels, int vi_mode, glia_hmt_eval_result* out) {
  auto bad = [](const char* what) { set_error(std::string("eval: ") + what); return GLIA_HMT_ERR_ARG; };
  if (!c) return bad("ctx must not be NULL");
  if (n_images < 1) return bad("at least one image pair");
  if (!d_res || !d_ref || !n_voxels || !out) return bad("d_res, d_ref, n_voxels and out must not be NULL");
  if (vi_mode != GLIA_HMT_VI_REFERENCE && vi_mode != GLIA_HMT_VI_EXACT) return bad("vi_mode must be GLIA_HMT_VI_REFERENCE or GLIA_HMT_VI_EXACT");
  for (int i = 0; i < n_images; ++i) if (int rc = overlap_args("eval", c, d_res[i], d_ref[i], n_voxels[i])) return rc;
  GLIA_HIP_TRY(hipSetDevice(c->device));
  std::vector<std::vector<glia_hmt_overlap_entry>> tables((size_t)n_images);
  std::vector<const glia_hmt_overlap_entry*> ptr((size_t)n_images);
  std::vector<int64_t> len((size_t)n_images);
  glia_hmt_eval_timing t = {0, 0, 0};
  for (int i = 0; i < n_images; ++i) {
    OverlapPass pass;
    if (int rc = label_overlap(d_res[i], d_ref[i], d_mask ? d_mask[i] : nullptr, (unsigned long long)n_voxels[i], GLIA_HMT_OVERLAP_DROP_ZERO_B, c->stream,
                               &tables[i], &pass)) return rc;
    t.ms_count += pass.ms; t.entries += (int64_t)tables[i].size(); t.repeats += pass.repeats;
    ptr[i] = tables[i].data(); len[i] = (int64_t)tables[i].size();
  }
  c->evt = t;
  return overlap_scores(ptr.data(), len.data(), n_images, vi_mode, out);
}

int glia_hmt_last_eval_timing(const glia_hmt_ctx* c, glia_hmt_eval_timing* out) {
  if (!c || !out) { set_error("last_eval_timing: invalid argument"); return GLIA_HMT_ERR_ARG; }
  *out = c->evt;
  return GLIA_HMT_OK;
}

// hmt::genTree (hmt/tree_build.hxx:12-38): order -> array tree, children before parents
int64_t glia_hmt_transform_keys(const uint32_t* h_order, int64_t n_merges, uint32_t* h_src, uint32_t* h_dst, int64_t capacity) {
  if (!h_order || !h_src || !h_dst || n_merges < 0) { set_error("transform_keys: invalid argument"); return GLIA_HMT_ERR_ARG; }
  std::vector<uint32_t> s, d;
  int rc = transform_keys(h_order, n_merges, &s, &d);
  if (rc) return rc;
  if ((int64_t)s.size() > capacity) { set_error("transform_keys: output capacity too small"); return GLIA_HMT_ERR_CAPACITY; }
  std::copy(s.begin(), s.end(), h_src);
  std::copy(d.begin(), d.end(), h_dst);
  return (int64_t)s.size();
}

int glia_hmt_transform_image(glia_hmt_ctx* c, uint32_t* d_labels, int64_t n_voxels, const uint32_t* h_src, const uint32_t* h_dst,
                             int64_t n_map, const uint32_t* d_mask, int fill_missing) {
  if (!c || !d_labels || n_voxels < 0 || n_map < 0 || (n_map && (!h_src || !h_dst))) { set_error("transform_image: invalid argument"); return GLIA_HMT_ERR_ARG; }
  GLIA_HIP_TRY(hipSetDevice(c->device));
  return transform_image(d_labels, n_voxels, h_src, h_dst, n_map, d_mask, fill_missing, c->stream, &c->transform_ms);
}

int glia_hmt_relabel_image(glia_hmt_ctx* c, uint32_t* d_labels, int64_t n_voxels, int64_t min_size, uint32_t* n_labels) {
  if (!c || !d_labels || n_voxels < 0 || !n_labels) { set_error("relabel_image: invalid argument"); return GLIA_HMT_ERR_ARG; }
  GLIA_HIP_TRY(hipSetDevice(c->device));
  return relabel_image(d_labels, n_voxels, min_size, n_labels, c->stream);
}

double glia_hmt_last_transform_ms(const glia_hmt_ctx* c) { return c ? c->transform_ms : 0.0; }

int64_t glia_hmt_gen_tree(const uint32_t* h_order, int64_t n_merges, uint32_t* node_label, int32_t* parent, int32_t* child0,
                          int32_t* child1, int64_t capacity) {
  if (!h_order || !node_label || !parent || !child0 || !child1 || n_merges < 0) { set_error("gen_tree: invalid argument"); return GLIA_HMT_ERR_ARG; }
  return gen_tree(h_order, n_merges, node_label, parent, child0, child1, capacity);
}

}  // extern "C"
