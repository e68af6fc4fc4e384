// glia_amd/csrc/truth_overlap.hip -- the leaf x truth contingency table of bc_label.
//
// Reference: hmt/main_bc_label_ri.cxx / main_bc_label_vi.cxx walk the voxels of r0, r1 and r2 of every merge again
// (stats::pairStats / stats::vi, util/image_stats.hxx:69-110,173-192).  Every quantity they compare is integer algebra over
// the counts c(leaf, t) of a leaf's voxels with truth label t (t = 0 included: it makes the region's size, VI's nPoint), so one
// streaming pass over the label and truth volumes produces all the voxel work of a merge order.
//
// One workgroup reads contiguous tiles of 4096 voxels; a thread takes 16 consecutive voxels (4 x 16-byte loads of each volume),
// folds equal (label, truth) runs, maps the label to its dense leaf with find_label (a one-entry cache per thread: neighbouring
// voxels rarely change region) and adds the run to a 2048-slot hash table in LDS.  A supervoxel meets few truth labels, so the
// LDS table absorbs almost every add; it is flushed into the global open-addressing table when more than half full and at the
// end.  Traffic: 8 B per voxel (labels + truth; with a mask the labels are the folded copy, so still 8 B).  Global keys are
// (leaf << 32 | truth); a table that gets more than 3/4 full stops inserting and reports it, and the host repeats the pass
// with twice the slots (the counts of an incomplete pass are discarded, never used).
#include <algorithm>

#include "greedy_common.hpp"

namespace glia {

namespace {

constexpr int kTOThreads = 256;
constexpr int kTOPerThread = 16;
constexpr int kTOTile = kTOThreads * kTOPerThread;
constexpr int kLdsSlots = 2048;
constexpr int kLdsProbe = 32;
constexpr unsigned long long kEmptyKey = ~0ull;

__device__ __forceinline__ uint32_t to_hash(unsigned long long k) {
  k ^= k >> 29; k *= 0xBF58476D1CE4E5B9ull; k ^= k >> 32;
  return (uint32_t)k;
}

__device__ void global_add(unsigned long long* keys, unsigned long long* cnt, uint32_t mask, uint32_t* st, unsigned long long key,
                           unsigned long long c) {
  uint32_t h = to_hash(key) & mask;
  for (uint32_t probe = 0; probe <= mask; ++probe, h = (h + 1) & mask) {
    unsigned long long k = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == kEmptyKey) {
      if (atomicAdd(&st[0], 0u) > (mask + 1) / 4 * 3) { atomicOr(&st[1], 1u); return; }   // too full: the host repeats the pass
      k = atomicCAS(&keys[h], kEmptyKey, key);
      if (k == kEmptyKey) { atomicAdd(&st[0], 1u); k = key; }
    }
    if (k == key) { atomicAdd(&cnt[h], c); return; }
  }
  atomicOr(&st[1], 1u);
}

template <bool kVec>
__global__ __launch_bounds__(kTOThreads) void to_count(const uint32_t* __restrict__ lab, const uint32_t* __restrict__ truth, long long N,
                                                       const uint32_t* __restrict__ rlabel, uint32_t R, long long tiles_per_block,
                                                       unsigned long long* keys, unsigned long long* cnt, uint32_t mask, uint32_t* st) {
  __shared__ unsigned long long s_key[kLdsSlots];
  __shared__ uint32_t s_cnt[kLdsSlots];
  __shared__ uint32_t s_used;
  for (int i = threadIdx.x; i < kLdsSlots; i += kTOThreads) { s_key[i] = kEmptyKey; s_cnt[i] = 0; }
  if (threadIdx.x == 0) s_used = 0;
  __syncthreads();
  uint32_t last_lab = kMaskedLabel, last_leaf = R;
  auto add = [&](uint32_t l, uint32_t t, uint32_t c) {
    if (l == kMaskedLabel) return;                         // masked-out voxel: in no region (util/struct.hxx:86-91)
    if (l != last_lab) {
      last_lab = l;
      last_leaf = find_label(rlabel, R, l);
      if (last_leaf < R && rlabel[last_leaf] != l) last_leaf = R;
    }
    if (last_leaf >= R) return;
    const unsigned long long key = ((unsigned long long)last_leaf << 32) | t;
    uint32_t h = to_hash(key) & (kLdsSlots - 1);
    for (int probe = 0; probe < kLdsProbe; ++probe, h = (h + 1) & (kLdsSlots - 1)) {
      unsigned long long k = s_key[h];
      if (k == kEmptyKey) {
        k = atomicCAS(&s_key[h], kEmptyKey, key);
        if (k == kEmptyKey) { atomicAdd(&s_used, 1u); k = key; }
      }
      if (k == key) { atomicAdd(&s_cnt[h], c); return; }
    }
    global_add(keys, cnt, mask, st, key, c);               // a crowded LDS neighbourhood: straight to the global table
  };
  auto flush = [&]() {
    for (int i = threadIdx.x; i < kLdsSlots; i += kTOThreads) {
      if (s_key[i] != kEmptyKey) global_add(keys, cnt, mask, st, s_key[i], s_cnt[i]);
      s_key[i] = kEmptyKey; s_cnt[i] = 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) s_used = 0;
    __syncthreads();
  };
  const long long t0 = (long long)blockIdx.x * tiles_per_block;
  for (long long tile = t0; tile < t0 + tiles_per_block; ++tile) {
    const long long base = tile * kTOTile + (long long)threadIdx.x * kTOPerThread;
    if (tile * kTOTile >= N) break;
    uint32_t L[kTOPerThread], T[kTOPerThread];
    int nv = 0;
    if (base < N) {
      if (kVec && base + kTOPerThread <= N) {
        const uint4* l4 = reinterpret_cast<const uint4*>(lab + base);
        const uint4* t4 = reinterpret_cast<const uint4*>(truth + base);
#pragma unroll
        for (int q = 0; q < kTOPerThread / 4; ++q) {
          const uint4 a = l4[q], b = t4[q];
          L[4 * q] = a.x; L[4 * q + 1] = a.y; L[4 * q + 2] = a.z; L[4 * q + 3] = a.w;
          T[4 * q] = b.x; T[4 * q + 1] = b.y; T[4 * q + 2] = b.z; T[4 * q + 3] = b.w;
        }
        nv = kTOPerThread;
      } else {
        nv = (int)std::min<long long>(kTOPerThread, N - base);
        for (int q = 0; q < nv; ++q) { L[q] = lab[base + q]; T[q] = truth[base + q]; }
      }
    }
    if (nv > 0) {
      uint32_t rl = L[0], rt = T[0], rc = 1;
      for (int q = 1; q < nv; ++q) {
        if (L[q] == rl && T[q] == rt) { ++rc; continue; }
        add(rl, rt, rc);
        rl = L[q]; rt = T[q]; rc = 1;
      }
      add(rl, rt, rc);
    }
    __syncthreads();
    if (s_used > kLdsSlots / 2) flush();
  }
  flush();
}

__global__ void to_compact(const unsigned long long* keys, const unsigned long long* cnt, uint32_t cap, uint32_t* n_out,
                           unsigned long long* out_key, unsigned long long* out_cnt) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cap || keys[i] == kEmptyKey) return;
  const uint32_t j = atomicAdd(n_out, 1u);
  out_key[j] = keys[i];
  out_cnt[j] = cnt[i];
}

}  // namespace

int truth_overlap(const VolumeRef& vol, const uint32_t* d_rlabel, uint32_t R, const uint32_t* d_truth, hipStream_t stream,
                  std::vector<TruthCount>* out, float* ms) {
  const long long N = vol.nx * vol.ny * vol.nz;
  out->clear();
  if (ms) *ms = 0;
  if (N == 0 || R == 0) return GLIA_HMT_OK;
  DeviceBuffers buf;
  CallEvents<2> ev;
  int rc;
  if ((rc = ev.create())) return rc;
  uint32_t* st;                                            // [0] keys in the table, [1] incomplete pass, [2] compacted
  if ((rc = buf.get(&st, 4, false, stream))) return rc;
  const bool vec = ((uintptr_t)vol.lab % 16 == 0) && ((uintptr_t)d_truth % 16 == 0);
  const long long tiles = (N + kTOTile - 1) / kTOTile;
  const long long blocks = std::min<long long>(tiles, 256 * 16);
  const long long per_block = (tiles + blocks - 1) / blocks;
  // slots: twice the expected keys (a leaf meets about two truth labels), a power of two; doubled while a pass overflows
  unsigned long long cap = 1ull << 16;
  while (cap < 8ull * R && cap < (1ull << 31)) cap <<= 1;
  if (option("GLIA_HMT_MINCAP")) cap = 1ull << 10;
  for (;;) {
    unsigned long long *keys, *cnt;
    if ((rc = buf.get(&keys, cap, false, stream)) || (rc = buf.get(&cnt, cap, true, stream))) return rc;
    GLIA_HIP_TRY(hipMemsetAsync(keys, 0xFF, 8 * cap, stream));
    GLIA_HIP_TRY(hipMemsetAsync(st, 0, 16, stream));
    GLIA_HIP_TRY(hipEventRecord(ev.ev[0], stream));
    if (vec)
      hipLaunchKernelGGL(to_count<true>, dim3((unsigned)blocks), dim3(kTOThreads), 0, stream, vol.lab, d_truth, N, d_rlabel, R, per_block, keys, cnt,
                         (uint32_t)(cap - 1), st);
    else
      hipLaunchKernelGGL(to_count<false>, dim3((unsigned)blocks), dim3(kTOThreads), 0, stream, vol.lab, d_truth, N, d_rlabel, R, per_block, keys, cnt,
                         (uint32_t)(cap - 1), st);
    GLIA_HIP_TRY(hipGetLastError());
    GLIA_HIP_TRY(hipEventRecord(ev.ev[1], stream));
    uint32_t h_st[2];
    GLIA_HIP_TRY(hipMemcpyAsync(h_st, st, 8, hipMemcpyDeviceToHost, stream));
    GLIA_HIP_TRY(hipStreamSynchronize(stream));
    if (ms) *ms = ev.ms(0, 1);
    if (h_st[1]) {
      if (cap >= (1ull << 31)) { set_error("bc_label: contingency table beyond 2^31 slots"); return GLIA_HMT_ERR_CAPACITY; }
      cap <<= 1;
      continue;
    }
    const uint32_t n = h_st[0];
    unsigned long long *ok, *oc;
    if ((rc = buf.get(&ok, n, false, stream)) || (rc = buf.get(&oc, n, false, stream))) return rc;
    GLIA_HIP_TRY(hipMemsetAsync(st + 2, 0, 4, stream));
    hipLaunchKernelGGL(to_compact, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, stream, keys, cnt, (uint32_t)cap, st + 2, ok, oc);
    GLIA_HIP_TRY(hipGetLastError());
    std::vector<unsigned long long> hk(n), hc(n);
    if (n) {
      GLIA_HIP_TRY(hipMemcpyAsync(hk.data(), ok, 8 * (size_t)n, hipMemcpyDeviceToHost, stream));
      GLIA_HIP_TRY(hipMemcpyAsync(hc.data(), oc, 8 * (size_t)n, hipMemcpyDeviceToHost, stream));
    }
    GLIA_HIP_TRY(hipStreamSynchronize(stream));
    out->resize(n);
    for (uint32_t i = 0; i < n; ++i) (*out)[i] = TruthCount{(uint32_t)(hk[i] >> 32), (uint32_t)hk[i], hc[i]};
    std::sort(out->begin(), out->end(), [](const TruthCount& a, const TruthCount& b) { return a.leaf != b.leaf ? a.leaf < b.leaf : a.truth < b.truth; });
    return GLIA_HMT_OK;
  }
}

}  // namespace glia
