// glia_amd/csrc/api_rag.cpp -- C ABI: the region-map handle (build, merge, copy, export, free) -- everything that owns a RagArrays.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "api_types.hpp"

int free_tables(glia_hmt_ctx* c) {
  for (void* p : {(void*)c->rkeys, (void*)c->rrec, (void*)c->pkeys, (void*)c->prec}) if (p) GLIA_HIP_TRY(hipFree(p));
  c->rkeys = nullptr; c->rrec = nullptr; c->pkeys = nullptr; c->prec = nullptr;
  c->rcap = c->pcap = 0;
  return GLIA_HMT_OK;
}

static int clear_tables(glia_hmt_ctx* c) {
  GLIA_HIP_TRY(hipMemsetAsync(c->rkeys, 0, sizeof(uint32_t) * (size_t)c->rcap, c->stream));
  GLIA_HIP_TRY(hipMemsetAsync(c->rrec, 0, sizeof(uint32_t) * kRegionWords * (size_t)c->rcap, c->stream));
  GLIA_HIP_TRY(hipMemsetAsync(c->pkeys, 0, sizeof(unsigned long long) * (size_t)c->pcap, c->stream));
  GLIA_HIP_TRY(hipMemsetAsync(c->prec, 0, sizeof(uint32_t) * kPairWords * (size_t)c->pcap, c->stream));
  return GLIA_HMT_OK;
}

static int ensure_tables(glia_hmt_ctx* c, uint32_t rcap, uint32_t pcap) {
  if (rcap <= c->rcap && pcap <= c->pcap) return GLIA_HMT_OK;
  rcap = std::max(rcap, c->rcap);
  pcap = std::max(pcap, c->pcap);
  int rc = free_tables(c);
  if (rc) return rc;
  GLIA_HIP_TRY(hipMalloc(&c->rkeys, sizeof(uint32_t) * (size_t)rcap));
  GLIA_HIP_TRY(hipMalloc(&c->rrec, sizeof(uint32_t) * kRegionWords * (size_t)rcap));
  GLIA_HIP_TRY(hipMalloc(&c->pkeys, sizeof(unsigned long long) * (size_t)pcap));
  GLIA_HIP_TRY(hipMalloc(&c->prec, sizeof(uint32_t) * kPairWords * (size_t)pcap));
  c->rcap = rcap;
  c->pcap = pcap;
  return clear_tables(c);
}

// every block a RagArrays owns, once: the keys, channel 0's records (= d_rrec / d_prec), the further channels' records, the value runs
void glia::free_rag_arrays(RagArrays* a) {
  OwnedArrays own;
  for (void* p : {(void*)a->d_rlabel, (void*)a->d_rrec, (void*)a->d_pa, (void*)a->d_pb, (void*)a->d_prec}) own.adopt(p);
  for (int k = 1; k < a->K; ++k) { own.adopt(a->c_rrec[k]); own.adopt(a->c_prec[k]); }
  own.adopt(a->d_pv_off); own.adopt(a->d_pv);
  *a = RagArrays();
}

extern "C" {

static int rag_build_impl(glia_hmt_ctx* c, int dim, const int64_t dims[3], int64_t gz0, int64_t gnz, int64_t zb, int64_t ze,
                          const uint32_t* d_labels, const uint32_t* d_mask, int only_contour, const float* d_pb,
                          const glia_hmt_feat_config* cfg, glia_hmt_rag** out) {
  if (!c || !dims || !d_labels || !out || (dim != 2 && dim != 3)) {
    set_error("rag_build: invalid argument");
    return GLIA_HMT_ERR_ARG;
  }
  const int64_t nx = dims[0], ny = dims[1], nz = dim == 3 ? dims[2] : 1;
  if (nx <= 0 || ny <= 0 || nz <= 0 || nx >= (1ll << 31) || ny >= (1ll << 31) || nz >= (1ll << 31)) {
    set_error("rag_build: bad dimensions");
    return GLIA_HMT_ERR_ARG;
  }
  GLIA_HIP_TRY(hipSetDevice(c->device));
  // ---- channels: one accumulation pass per distinct (volume, bins, lo, hi) over the three feature lists; channel 0
  // is the boundary-probability volume (thresholded counts, pb linkages) ----
  struct Chan { const float* img; int bins; double lo, hi; };
  std::vector<Chan> chans;
  int map_region[GLIA_HMT_MAX_IMAGES] = {0}, map_rlabel[GLIA_HMT_MAX_IMAGES] = {0}, map_boundary[GLIA_HMT_MAX_IMAGES] = {0};
  int nthr = 0;
  double thr[GLIA_HMT_MAX_THRESH] = {0, 0, 0, 0};
  if (cfg) {
    if (cfg->n_region < 0 || cfg->n_rlabel < 0 || cfg->n_boundary < 0 || cfg->n_region > kMaxListed ||
        cfg->n_rlabel > kMaxListed || cfg->n_boundary > kMaxListed ||
        cfg->n_thresholds < 0 || cfg->n_thresholds > GLIA_HMT_MAX_THRESH) {
      set_error("rag_build: feature configuration out of range (at most " + std::to_string(kMaxListed) + " images per list, " + std::to_string(GLIA_HMT_MAX_THRESH) + " thresholds)");
      return GLIA_HMT_ERR_ARG;
    }
    const float* pbv = cfg->d_pb ? cfg->d_pb : d_pb;
    auto same = [](const Chan& c, const glia_hmt_image& g) { return c.img == g.d_image && c.bins == g.bins && c.lo == g.lo && c.hi == g.hi; };
    // channel 0: the first listed image that IS the pb volume (its histogram spec comes along), else pb with 8 bins on [0,1]
    const glia_hmt_image* lists[3] = {cfg->region, cfg->rlabel, cfg->boundary};
    const int counts[3] = {cfg->n_region, cfg->n_rlabel, cfg->n_boundary};
    for (int l = 0; l < 3 && chans.empty(); ++l)
      for (int i = 0; i < counts[l] && chans.empty(); ++i)
        if (pbv && lists[l][i].d_image == pbv) chans.push_back(Chan{pbv, lists[l][i].bins, lists[l][i].lo, lists[l][i].hi});
    if (chans.empty()) {
      if (pbv) chans.push_back(Chan{pbv, 8, 0.0, 1.0});
      else if (counts[0] + counts[1] + counts[2] > 0) {      // no pb at all: thresholds count on the first image
        const glia_hmt_image& g = counts[0] ? cfg->region[0] : (counts[1] ? cfg->rlabel[0] : cfg->boundary[0]);
        chans.push_back(Chan{g.d_image, g.bins, g.lo, g.hi});
      }
    }
    int* maps[3] = {map_region, map_rlabel, map_boundary};
    for (int l = 0; l < 3; ++l)
      for (int i = 0; i < counts[l]; ++i) {
        const glia_hmt_image& g = lists[l][i];
        if (!g.d_image) { set_error("rag_build: null image in a feature list"); return GLIA_HMT_ERR_ARG; }
        int k = -1;
        for (size_t q = 0; q < chans.size(); ++q) if (same(chans[q], g)) { k = (int)q; break; }
        if (k < 0) {
          if ((int)chans.size() >= kMaxChannels) { set_error("rag_build: more than 4 distinct (image volume, histogram) channels"); return GLIA_HMT_ERR_UNSUPPORTED; }
          chans.push_back(Chan{g.d_image, g.bins, g.lo, g.hi});
          k = (int)chans.size() - 1;
        }
        maps[l][i] = k;
      }
    nthr = cfg->n_thresholds;
    for (int i = 0; i < nthr; ++i) thr[i] = cfg->thresholds[i];
  } else if (d_pb) chans.push_back(Chan{d_pb, 8, 0.0, 1.0});
  if (chans.empty()) { set_error("rag_build: no image volume given"); return GLIA_HMT_ERR_ARG; }
  for (const Chan& ch : chans)
    if (ch.bins < 1 || ch.bins > GLIA_HMT_MAX_BINS || !(ch.hi > ch.lo)) {
      set_error("rag_build: histogram bins must be 1..16 and hi > lo");
      return GLIA_HMT_ERR_ARG;
    }
  const float* img = chans[0].img;
  const int bins = chans[0].bins;

  const int64_t N = nx * ny * nz;
  uint32_t rcap = c->hint_rcap ? c->hint_rcap : next_pow2(std::max<int64_t>(1 << 12, N / 128));
  uint32_t pcap = c->hint_pcap ? c->hint_pcap : next_pow2(std::max<int64_t>(1 << 14, N / 32));

  glia_hmt_rag* rag = new glia_hmt_rag;
  rag->ctx = c; rag->dim = dim; rag->dims[0] = nx; rag->dims[1] = ny; rag->dims[2] = gnz;
  rag->only_contour = only_contour != 0;
  rag->bins = bins; rag->nthr = nthr;
  if (cfg) { rag->cfg = *cfg; rag->has_cfg = true; }
  const uint32_t* lab_nb = d_labels;
  const uint32_t* lab_c = d_labels;
  if (d_mask) {
    if (hipError_t e = hipMalloc(&rag->d_folded, sizeof(uint32_t) * (size_t)N)) { glia_hmt_rag_free(rag); set_error(std::string("rag_build: ") + hipGetErrorString(e)); return GLIA_HMT_ERR_HIP; }
    int rcm = launch_mask_fold(d_labels, d_mask, rag->d_folded, N, c->stream);
    if (rcm) { glia_hmt_rag_free(rag); return rcm; }
    lab_nb = rag->d_folded;
    lab_c = only_contour ? d_labels : rag->d_folded;      // util/struct.hxx:133-143 has no mask test on the centre voxel
  }
  if (zb == 0 && ze == nz && gz0 == 0 && gnz == nz) {
    rag->vol.lab = lab_c; rag->vol.lab_nb = lab_nb; rag->vol.pb = d_pb ? d_pb : img; rag->vol.dim = dim;
    rag->vol.nx = nx; rag->vol.ny = ny; rag->vol.nz = nz;
  }
  if (!d_mask && dim == 3) {
    // a slab: the planes handed in, of which [zb, ze) are owned -- what collect_pair_values walks for the median linkage of the
    // slab route (the caller keeps the planes alive until glia_hmt_rag_build_distributed returns)
    rag->slab.lab = lab_c; rag->slab.lab_nb = lab_nb; rag->slab.pb = d_pb ? d_pb : img; rag->slab.dim = 3;
    rag->slab.nx = nx; rag->slab.ny = ny; rag->slab.nz = nz; rag->slab.zb = zb; rag->slab.ze = ze;
  }

  memcpy(rag->map_region, map_region, sizeof(map_region)); memcpy(rag->map_rlabel, map_rlabel, sizeof(map_rlabel));
  memcpy(rag->map_boundary, map_boundary, sizeof(map_boundary));
  double pass_ms_total = 0.0;
  for (size_t ci = 0; ci < chans.size(); ++ci) {
  RagArrays pass_arr;
  for (int attempt = 0;; ++attempt) {
    int rc = ensure_tables(c, rcap, pcap);
    if (rc) { glia_hmt_rag_free(rag); return rc; }
    AccParams p;
    p.lab = lab_nb; p.lab_c = lab_c; p.masked = d_mask ? 1 : 0; p.img = chans[ci].img;
    p.nx = nx; p.ny = ny; p.nz = nz; p.dim = dim;
    p.gz0 = gz0; p.gnz = gnz; p.zb = zb; p.ze = ze;
    p.nbx = (int)((nx + kTileX - 1) / kTileX);
    p.nby = (int)((ny + kTileY - 1) / kTileY);
    p.tz = c->tz;
    p.nbz = (int)((ze - zb + p.tz - 1) / p.tz);
    p.hist = make_hist_spec(chans[ci].bins, chans[ci].lo, chans[ci].hi);
    p.nthr = nthr;
    for (int i = 0; i < GLIA_HMT_MAX_THRESH; ++i) p.thr_f[i] = i < nthr ? ceil_f32(thr[i]) : std::numeric_limits<float>::infinity();
    p.rkeys = c->rkeys; p.rrec = c->rrec; p.rmask = c->rcap - 1;
    p.pkeys = c->pkeys; p.prec = c->prec; p.pmask = c->pcap - 1;
    p.flags = c->flags;
    { std::string dbg; p.debug = option("GLIA_HMT_DEBUG", &dbg) ? (uint32_t)strtoul(dbg.c_str(), nullptr, 0) : 0u; }
    if ((int64_t)p.nbx * p.nby * p.nbz >= (1ll << 31)) { glia_hmt_rag_free(rag); set_error("rag_build: volume too large"); return GLIA_HMT_ERR_ARG; }
    // the pass addresses a column's rows with 32-bit byte offsets from a base that moves every four planes (rag_accumulate.hip)
    if (nx * ny * 4 * 11 >= (1ll << 32)) { glia_hmt_rag_free(rag); set_error("rag_build: planes of more than 97 M voxels are not supported"); return GLIA_HMT_ERR_ARG; }
    hipError_t e = hipEventRecord(c->ev0, c->stream);
    if (e == hipSuccess) { rc = launch_accumulate(p, c->stream); e = hipEventRecord(c->ev1, c->stream); }
    if (e != hipSuccess) { glia_hmt_rag_free(rag); set_error(hipGetErrorString(e)); return GLIA_HMT_ERR_HIP; }
    if (rc) { glia_hmt_rag_free(rag); return rc; }
    uint32_t flags[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    e = hipMemcpyAsync(flags, c->flags, sizeof(flags), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { glia_hmt_rag_free(rag); set_error(std::string("rag_build: ") + hipGetErrorString(e)); return GLIA_HMT_ERR_HIP; }
    float ms = 0;
    (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
    pass_ms_total += ms;
    rag->pass_ms = pass_ms_total;
    if (p.debug & 32) {
      unsigned long long pc[12];
      (void)hipMemcpy(pc, c->flags + 16, sizeof(pc), hipMemcpyDeviceToHost);
      fprintf(stderr, "[glia_hmt debug] marching waves: %llu waits for room in a ring, %llu cycles waiting of %llu cycles marching\n", pc[9], pc[8], pc[10]);
      fprintf(stderr, "[glia_hmt debug] drainers: region batches %llu entries %llu cycles %llu | pair batches %llu entries %llu cycles %llu | idle polls %llu, drainer cycles %llu\n",
              pc[0], pc[1], pc[2], pc[3], pc[4], pc[5], pc[6], pc[7]);
      (void)hipMemsetAsync(c->flags, 0, 256, c->stream);
    }
    rag->alg_bytes = (double)(nx * ny * (ze - zb)) * 8.0 * (double)chans.size();
    // runs that found the tile's LDS tables full went to the global tables one by one (exact, slow): with more than one
    // such run per 256 voxels the supervoxels are too small for this tile depth -- use shallower tiles from now on
    if (c->tz > 4 && (double)flags[7] * 256.0 > (double)(nx * ny * (ze - zb))) c->tz /= 2;
    if (flags[7]) (void)hipMemsetAsync(c->flags + 7, 0, sizeof(uint32_t), c->stream);
    if (flags[0] || flags[1]) {
      // a table filled up: drop the partial result, grow and redo the pass
      if (attempt >= 6) { glia_hmt_rag_free(rag); set_error("rag_build: hash tables keep overflowing"); return GLIA_HMT_ERR_HIP; }
      (void)hipMemsetAsync(c->flags, 0, 64, c->stream);
      rc = clear_tables(c);
      if (rc) { glia_hmt_rag_free(rag); return rc; }
      if (flags[0]) rcap = c->rcap * 4;
      if (flags[1]) pcap = c->pcap * 4;
      continue;
    }
    rc = compact_tables(p, c->rcap, c->pcap, &pass_arr, c->stream);
    if (rc) { glia_hmt_rag_free(rag); return rc; }
    break;
  }
  if (ci == 0) rag->arr = pass_arr;
  else {
    // the keys depend on the labels only: every pass yields the same sorted key arrays, and only its records are kept
    const bool same = pass_arr.R == rag->arr.R && pass_arr.P == rag->arr.P;
    if (same) { rag->arr.c_rrec[ci] = pass_arr.d_rrec; rag->arr.c_prec[ci] = pass_arr.d_prec; pass_arr.d_rrec = pass_arr.d_prec = nullptr; }
    free_rag_arrays(&pass_arr);
    if (!same) { glia_hmt_rag_free(rag); set_error("rag_build: channel passes disagree on the region set"); return GLIA_HMT_ERR_HIP; }
  }
  rag->arr.c_bins[ci] = chans[ci].bins;
  rag->arr.K = (int)ci + 1;
  }
  *out = rag;
  return GLIA_HMT_OK;
}

int glia_hmt_rag_build(glia_hmt_ctx* c, int dim, const int64_t dims[3], const uint32_t* d_labels,
                       const uint32_t* d_mask, int only_contour, const float* d_pb,
                       const glia_hmt_feat_config* cfg, glia_hmt_rag** out) {
  if (!dims) { set_error("rag_build: invalid argument"); return GLIA_HMT_ERR_ARG; }
  const int64_t nz = dim == 3 ? dims[2] : 1;
  return rag_build_impl(c, dim, dims, 0, nz, 0, nz, d_labels, d_mask, only_contour, d_pb, cfg, out);
}

int glia_hmt_rag_build_slab(glia_hmt_ctx* c, const int64_t dims_local[3], int64_t z_global_of_plane0, int64_t nz_global,
                            int64_t z_begin, int64_t z_end, const uint32_t* d_labels, int only_contour, const float* d_pb,
                            const glia_hmt_feat_config* cfg, glia_hmt_rag** out) {
  if (!dims_local || z_begin < 0 || z_end > dims_local[2] || z_begin >= z_end || z_global_of_plane0 < 0 ||
      z_global_of_plane0 + dims_local[2] > nz_global ||
      (z_begin > 0 ? false : z_global_of_plane0 != 0) || (z_end < dims_local[2] ? false : z_global_of_plane0 + z_end != nz_global)) {
    // the plane below z_begin / above z_end-1 must be present unless the slab touches the volume face
    set_error("rag_build_slab: slab range or halo planes inconsistent");
    return GLIA_HMT_ERR_ARG;
  }
  return rag_build_impl(c, 3, dims_local, z_global_of_plane0, nz_global, z_begin, z_end, d_labels, nullptr, only_contour, d_pb,
                        cfg, out);
}

int glia_hmt_rag_merge(glia_hmt_ctx* c, glia_hmt_rag* const* parts, int n_parts, glia_hmt_rag** out) {
  if (!c || !parts || n_parts < 1 || n_parts > 255 || !out) { set_error("rag_merge: invalid argument"); return GLIA_HMT_ERR_ARG; }
  GLIA_HIP_TRY(hipSetDevice(c->device));
  std::vector<RagArrays> arrs;
  for (int i = 0; i < n_parts; ++i) {
    if (!parts[i] || parts[i]->ctx != c || parts[i]->bins != parts[0]->bins || parts[i]->nthr != parts[0]->nthr || parts[i]->arr.K != parts[0]->arr.K ||
        parts[i]->dims[0] != parts[0]->dims[0] || parts[i]->dims[1] != parts[0]->dims[1] || parts[i]->dims[2] != parts[0]->dims[2]) {
      set_error("rag_merge: parts do not belong together");
      return GLIA_HMT_ERR_ARG;
    }
    arrs.push_back(parts[i]->arr);
  }
  glia_hmt_rag* rag = rag_like(parts[0]);
  rag->pass_ms = 0; rag->alg_bytes = 0;
  for (int i = 0; i < n_parts; ++i) { rag->pass_ms += parts[i]->pass_ms; rag->alg_bytes += parts[i]->alg_bytes; }
  int rc = merge_rag_arrays(arrs.data(), n_parts, &rag->arr, c->stream);
  if (rc) { glia_hmt_rag_free(rag); return rc; }
  *out = rag;
  return GLIA_HMT_OK;
}

int glia_hmt_rag_num_channels(const glia_hmt_rag* r) { return r ? r->arr.K : -1; }

int glia_hmt_rag_copy_channel(const glia_hmt_rag* r, int channel, uint32_t* d_region_rec, uint32_t* d_pair_rec) {
  if (!r || channel < 0 || channel >= r->arr.K || !d_region_rec || !d_pair_rec) { set_error("rag_copy_channel: invalid argument"); return GLIA_HMT_ERR_ARG; }
  GLIA_HIP_TRY(hipSetDevice(r->ctx->device));
  hipStream_t s = r->ctx->stream;
  if (r->arr.R) GLIA_HIP_TRY(hipMemcpyAsync(d_region_rec, r->arr.c_rrec[channel], sizeof(uint32_t) * (size_t)r->arr.R * kRegionWords, hipMemcpyDeviceToDevice, s));
  if (r->arr.P) GLIA_HIP_TRY(hipMemcpyAsync(d_pair_rec, r->arr.c_prec[channel], sizeof(uint32_t) * (size_t)r->arr.P * kPairWords, hipMemcpyDeviceToDevice, s));
  GLIA_HIP_TRY(hipStreamSynchronize(s));
  return GLIA_HMT_OK;
}

int glia_hmt_rag_add_channel(glia_hmt_ctx* c, glia_hmt_rag* r, const uint32_t* d_region_rec, const uint32_t* d_pair_rec) {
  if (!c || !r || r->ctx != c || !d_region_rec || !d_pair_rec || r->arr.K < 1 || r->arr.K >= kMaxChannels) { set_error("rag_add_channel: invalid argument"); return GLIA_HMT_ERR_ARG; }
  GLIA_HIP_TRY(hipSetDevice(c->device));
  const int k = r->arr.K;
  OwnedArrays own;
  uint32_t *rr, *pr;
  if (int rc = own.alloc(&rr, kRegionWords * (size_t)(r->arr.R ? r->arr.R : 1))) return rc;
  if (int rc = own.alloc(&pr, kPairWords * (size_t)(r->arr.P ? r->arr.P : 1))) return rc;
  if (r->arr.R) GLIA_HIP_TRY(hipMemcpyAsync(rr, d_region_rec, sizeof(uint32_t) * (size_t)r->arr.R * kRegionWords, hipMemcpyDeviceToDevice, c->stream));
  if (r->arr.P) GLIA_HIP_TRY(hipMemcpyAsync(pr, d_pair_rec, sizeof(uint32_t) * (size_t)r->arr.P * kPairWords, hipMemcpyDeviceToDevice, c->stream));
  GLIA_HIP_TRY(hipStreamSynchronize(c->stream));
  own.keep();
  r->arr.c_rrec[k] = rr; r->arr.c_prec[k] = pr; r->arr.K = k + 1;
  return GLIA_HMT_OK;
}

int glia_hmt_rag_cut_flags(glia_hmt_ctx* c, const glia_hmt_rag* rag, const int64_t dims_local[3], int64_t z_begin, int64_t z_end,
                           const uint32_t* d_labels, uint8_t* d_region_cut, uint8_t* d_pair_cut) {
  if (!c || !rag || !dims_local || !d_labels || !d_region_cut || !d_pair_cut || rag->ctx != c || z_begin < 0 || z_end > dims_local[2] || z_begin >= z_end) {
    set_error("rag_cut_flags: invalid argument");
    return GLIA_HMT_ERR_ARG;
  }
  GLIA_HIP_TRY(hipSetDevice(c->device));
  return rag_cut_flags(rag->arr, d_labels, dims_local[0], dims_local[1], dims_local[2], z_begin, z_end, d_region_cut, d_pair_cut, c->stream);
}

int glia_hmt_rag_device_arrays(const glia_hmt_rag* r, const uint32_t** d_region_label, const uint32_t** d_region_rec,
                               const uint32_t** d_pair_a, const uint32_t** d_pair_b, const uint32_t** d_pair_rec,
                               int* region_words, int* pair_words) {
  if (!r) return GLIA_HMT_ERR_ARG;
  if (d_region_label) *d_region_label = r->arr.d_rlabel;
  if (d_region_rec) *d_region_rec = r->arr.d_rrec;
  if (d_pair_a) *d_pair_a = r->arr.d_pa;
  if (d_pair_b) *d_pair_b = r->arr.d_pb;
  if (d_pair_rec) *d_pair_rec = r->arr.d_prec;
  if (region_words) *region_words = kRegionWords;
  if (pair_words) *pair_words = kPairWords;
  return GLIA_HMT_OK;
}

int glia_hmt_rag_copy_arrays(const glia_hmt_rag* r, uint32_t* d_region_label, uint32_t* d_region_rec, uint32_t* d_pair_a,
                             uint32_t* d_pair_b, uint32_t* d_pair_rec) {
  if (!r) return GLIA_HMT_ERR_ARG;
  GLIA_HIP_TRY(hipSetDevice(r->ctx->device));
  hipStream_t st = r->ctx->stream;
  const size_t R = (size_t)r->arr.R, P = (size_t)r->arr.P;
  if (d_region_label && R) GLIA_HIP_TRY(hipMemcpyAsync(d_region_label, r->arr.d_rlabel, 4 * R, hipMemcpyDeviceToDevice, st));
  if (d_region_rec && R) GLIA_HIP_TRY(hipMemcpyAsync(d_region_rec, r->arr.d_rrec, 4 * R * kRegionWords, hipMemcpyDeviceToDevice, st));
  if (d_pair_a && P) GLIA_HIP_TRY(hipMemcpyAsync(d_pair_a, r->arr.d_pa, 4 * P, hipMemcpyDeviceToDevice, st));
  if (d_pair_b && P) GLIA_HIP_TRY(hipMemcpyAsync(d_pair_b, r->arr.d_pb, 4 * P, hipMemcpyDeviceToDevice, st));
  if (d_pair_rec && P) GLIA_HIP_TRY(hipMemcpyAsync(d_pair_rec, r->arr.d_prec, 4 * P * kPairWords, hipMemcpyDeviceToDevice, st));
  GLIA_HIP_TRY(hipStreamSynchronize(st));
  return GLIA_HMT_OK;
}

int glia_hmt_rag_from_arrays(glia_hmt_ctx* c, const glia_hmt_rag* like, int64_t n_regions, const uint32_t* d_region_label,
                             const uint32_t* d_region_rec, int64_t n_pairs, const uint32_t* d_pair_a, const uint32_t* d_pair_b,
                             const uint32_t* d_pair_rec, glia_hmt_rag** out) {
  if (!c || !like || !out || n_regions < 0 || n_pairs < 0) { set_error("rag_from_arrays: invalid argument"); return GLIA_HMT_ERR_ARG; }
  GLIA_HIP_TRY(hipSetDevice(c->device));
  glia_hmt_rag* rag = rag_like(like);
  rag->ctx = c;
  rag->arr.R = n_regions; rag->arr.P = n_pairs;
  // (the handle owns each array as soon as it is allocated: glia_hmt_rag_free releases what exists)
  auto dup = [&](uint32_t** dst, const uint32_t* src, size_t n) -> int {
    GLIA_HIP_TRY(hipMalloc(dst, sizeof(uint32_t) * (n ? n : 1)));
    if (n) GLIA_HIP_TRY(hipMemcpyAsync(*dst, src, sizeof(uint32_t) * n, hipMemcpyDeviceToDevice, c->stream));
    return GLIA_HMT_OK;
  };
  int rc;
  if ((rc = dup(&rag->arr.d_rlabel, d_region_label, (size_t)n_regions)) || (rc = dup(&rag->arr.d_rrec, d_region_rec, (size_t)n_regions * kRegionWords)) ||
      (rc = dup(&rag->arr.d_pa, d_pair_a, (size_t)n_pairs)) || (rc = dup(&rag->arr.d_pb, d_pair_b, (size_t)n_pairs)) ||
      (rc = dup(&rag->arr.d_prec, d_pair_rec, (size_t)n_pairs * kPairWords))) { glia_hmt_rag_free(rag); return rc; }
  rag->arr.K = 1; rag->arr.c_rrec[0] = rag->arr.d_rrec; rag->arr.c_prec[0] = rag->arr.d_prec;
  for (int k = 0; k < kMaxChannels; ++k) rag->arr.c_bins[k] = like->arr.c_bins[k];      // (further channels: glia_hmt_rag_add_channel)
  rag->arr.c_bins[0] = rag->bins;
  if (hipError_t e = hipStreamSynchronize(c->stream)) { glia_hmt_rag_free(rag); set_error(std::string("rag_from_arrays: ") + hipGetErrorString(e)); return GLIA_HMT_ERR_HIP; }
  *out = rag;
  return GLIA_HMT_OK;
}

void glia_hmt_rag_free(glia_hmt_rag* r) {
  if (!r) return;
  (void)hipSetDevice(r->ctx->device);
  free_rag_arrays(&r->arr);
  OwnedArrays rest;                      // what the handle owns besides its arrays
  rest.adopt(r->d_folded);
  delete r;
}

int64_t glia_hmt_rag_num_regions(const glia_hmt_rag* r) { return r ? r->arr.R : -1; }
int64_t glia_hmt_rag_num_pairs(const glia_hmt_rag* r) { return r ? r->arr.P : -1; }

int glia_hmt_rag_last_pass(const glia_hmt_rag* r, double* ms, double* bytes) {
  if (!r) return GLIA_HMT_ERR_ARG;
  if (ms) *ms = r->pass_ms;
  if (bytes) *bytes = r->alg_bytes;
  return GLIA_HMT_OK;
}

static double dword(const uint32_t* w) { double d; std::memcpy(&d, w, 8); return d; }

int glia_hmt_rag_export_regions(const glia_hmt_rag* r, uint32_t* h_label, int64_t* h_count, int64_t* h_border,
                                int64_t* h_lo, int64_t* h_hi, double* h_sum, double* h_sumsq, double* h_min,
                                double* h_max, int64_t* h_hist, int64_t* h_first) {
  if (!r) return GLIA_HMT_ERR_ARG;
  GLIA_HIP_TRY(hipSetDevice(r->ctx->device));
  const int64_t R = r->arr.R;
  std::vector<uint32_t> lab(R), rec((size_t)R * kRegionWords);
  if (R) {
    GLIA_HIP_TRY(hipMemcpy(lab.data(), r->arr.d_rlabel, sizeof(uint32_t) * R, hipMemcpyDeviceToHost));
    GLIA_HIP_TRY(hipMemcpy(rec.data(), r->arr.d_rrec, sizeof(uint32_t) * kRegionWords * R, hipMemcpyDeviceToHost));
  }
  for (int64_t i = 0; i < R; ++i) {
    const uint32_t* w = &rec[(size_t)i * kRegionWords];
    if (h_label) h_label[i] = lab[i];
    if (h_count) h_count[i] = w[R_CNT];
    if (h_border) h_border[i] = w[R_BORDER];
    for (int d = 0; d < 3; ++d) {
      if (h_lo) h_lo[3 * i + d] = (int64_t)(0x7fffffffu - w[R_LO + d]);
      if (h_hi) h_hi[3 * i + d] = (int64_t)w[R_HI + d] - 1;
    }
    if (h_sum) h_sum[i] = dword(&w[R_SUM]);
    if (h_sumsq) h_sumsq[i] = dword(&w[R_SQ]);
    if (h_min) h_min[i] = (double)ord_float(~w[R_MIN]);
    if (h_max) h_max[i] = (double)ord_float(w[R_MAX]);
    if (h_hist) for (int b = 0; b < r->bins; ++b) h_hist[i * r->bins + b] = w[R_HIST + b];
    if (h_first) { unsigned long long f; std::memcpy(&f, &w[R_FIRST], 8); h_first[i] = (int64_t)~f; }
  }
  return GLIA_HMT_OK;
}

int glia_hmt_rag_export_pairs(const glia_hmt_rag* r, uint32_t* h_a, uint32_t* h_b, int64_t* h_count, double* h_sum,
                              double* h_sumsq, double* h_min, double* h_max, int64_t* h_hist, int64_t* h_thr) {
  if (!r) return GLIA_HMT_ERR_ARG;
  GLIA_HIP_TRY(hipSetDevice(r->ctx->device));
  const int64_t P = r->arr.P;
  std::vector<uint32_t> a(P), b(P), rec((size_t)P * kPairWords);
  if (P) {
    GLIA_HIP_TRY(hipMemcpy(a.data(), r->arr.d_pa, sizeof(uint32_t) * P, hipMemcpyDeviceToHost));
    GLIA_HIP_TRY(hipMemcpy(b.data(), r->arr.d_pb, sizeof(uint32_t) * P, hipMemcpyDeviceToHost));
    GLIA_HIP_TRY(hipMemcpy(rec.data(), r->arr.d_prec, sizeof(uint32_t) * kPairWords * P, hipMemcpyDeviceToHost));
  }
  for (int64_t i = 0; i < P; ++i) {
    const uint32_t* w = &rec[(size_t)i * kPairWords];
    if (h_a) h_a[i] = a[i];
    if (h_b) h_b[i] = b[i];
    if (h_count) h_count[i] = w[P_CNT];
    if (h_sum) h_sum[i] = dword(&w[P_SUM]);
    if (h_sumsq) h_sumsq[i] = dword(&w[P_SQ]);
    if (h_min) h_min[i] = (double)ord_float(~w[P_MIN]);
    if (h_max) h_max[i] = (double)ord_float(w[P_MAX]);
    if (h_hist) for (int k = 0; k < r->bins; ++k) h_hist[i * r->bins + k] = w[P_HIST + k];
    if (h_thr) for (int k = 0; k < r->nthr; ++k) h_thr[i * r->nthr + k] = w[P_THR + k];
  }
  return GLIA_HMT_OK;
}

}  // extern "C"
