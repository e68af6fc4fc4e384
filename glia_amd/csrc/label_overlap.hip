// glia_amd/csrc/label_overlap.hip -- the contingency table of two label volumes under a mask.
//
// Reference: stats::pairStats and stats::centropy on images (util/image_stats.hxx:122-158,248-273), stats::getOverlap (:308-335)
// and the tools built on them (gadget/main_eval_ri.cxx, main_eval_vi.cxx) walk two label images and a mask once and count the
// voxels of every label pair in an unordered_map.  Every score they print is algebra over those counts c(a, b), so one streaming
// pass produces all their voxel work.  Dimensionality plays no part: the volumes are flat streams.
//
// A voxel takes part if its mask value is not MASK_OUT_VAL = 0 (no mask: every voxel) and it is not dropped by "a == 0" / "b == 0".
//
// Loads: a lane reads one 16-byte word (4 consecutive voxels) of each volume per step, so a wave covers 1 KiB of contiguous
// addresses and a 256-thread workgroup 4 KiB per volume per step; a workgroup owns one contiguous range of the stream.  The loads
// of kLOAhead steps are issued before the first is consumed.  Traffic: 8 B per voxel, 12 B with a mask.  The vector path needs every
// pointer 16-byte aligned; otherwise, and in the last word of the stream (n_voxels % 4), the same lanes read their voxels one by one.
//
// Counting: a lane folds the equal pairs it meets in a group of steps into one add to a 2048-slot open-addressing table in LDS
// (64-bit keys a << 32 | b, u32 counts: a workgroup sees fewer than 2^32 voxels).  The table is flushed into the global
// open-addressing table (u64 keys and counts, 64-bit atomics) when more than half full and once at the end; an add that finds its
// LDS neighbourhood crowded goes straight to the global table.  A global table more than 3/4 full (the workgroups report their
// new keys once per flush), or one in which a probe walks 4096 slots without an end, marks the pass incomplete; the host discards
// that pass and repeats it with twice the slots.
//
// Labels are arbitrary 32-bit values on both sides, so the pair (0xFFFFFFFF, 0xFFFFFFFF) has the key that marks an empty slot:
// it never enters a table, lanes count it in a register and add it to one counter of its own at the end.
//
// Barriers: every thread of a workgroup reaches every __syncthreads().  The step loop's bounds depend on blockIdx only, the flush
// decision is a value every thread reads between two barriers (nobody writes it there), and every probing loop is bounded.
#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>

#include "greedy_common.hpp"

namespace glia {

namespace {

constexpr int kLOThreads = 256;
constexpr int kLOStep = kLOThreads * 4;      // voxels of a workgroup's step: 4 KiB per volume
constexpr int kLOAhead = 2;                  // steps whose loads are in flight together
// Steps of one workgroup (a multiple of kLOAhead): 16 Ki voxels.  Measured: 16 - 32 steps are the fastest at 512^3 and
// at 1024^3; a grid capped at 2048 - 4096 workgroups, i.e. hundreds of steps each at 1024^3, took up to 1.5 times as long.
constexpr int kLOStepsPerBlock = 16;
constexpr int kLdsSlots = 2048;
constexpr int kLdsProbe = 32;
constexpr uint32_t kGlobalProbe = 4096;
constexpr unsigned long long kEmptyKey = ~0ull;

__device__ __forceinline__ uint32_t lo_hash(unsigned long long k) {
  k ^= k >> 29; k *= 0xBF58476D1CE4E5B9ull; k ^= k >> 32;
  return (uint32_t)k;
}

// Adds c to the slot of `key`; true when this call put the key into the table.  Probing is bounded: a walk of kGlobalProbe slots
// without an end means a table far fuller than the 3/4 the workgroups allow one another, and marks the pass incomplete (st[1]).
__device__ bool lo_global_add(unsigned long long* keys, unsigned long long* cnt, uint32_t mask, uint32_t* st, unsigned long long key,
                              unsigned long long c) {
  uint32_t h = lo_hash(key) & mask;
  const uint32_t most = mask < kGlobalProbe ? mask + 1 : kGlobalProbe;
  for (uint32_t probe = 0; probe < most; ++probe, h = (h + 1) & mask) {
    unsigned long long k = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bool fresh = false;
    if (k == kEmptyKey) {
      k = atomicCAS(&keys[h], kEmptyKey, key);
      if (k == kEmptyKey) { fresh = true; k = key; }
    }
    if (k == key) { atomicAdd(&cnt[h], c); return fresh; }
  }
  atomicOr(&st[1], 1u);
  return false;
}

// s_ctr: [0] slots of the LDS table in use, [1] keys this workgroup has put into the global table since it last reported them.
// One call site per run a lane may end (9 in a group of steps): a function of its own keeps the probing loops out of the unrolled
// step code.
__device__ __noinline__ void lo_lds_add(unsigned long long* s_key, uint32_t* s_cnt, uint32_t* s_ctr, unsigned long long* keys,
                                        unsigned long long* cnt, uint32_t mask, uint32_t* st, unsigned long long key, uint32_t c) {
  uint32_t h = lo_hash(key) & (kLdsSlots - 1);
  for (int probe = 0; probe < kLdsProbe; ++probe, h = (h + 1) & (kLdsSlots - 1)) {
    unsigned long long k = s_key[h];
    if (k == kEmptyKey) {
      k = atomicCAS(&s_key[h], kEmptyKey, key);
      if (k == kEmptyKey) { atomicAdd(&s_ctr[0], 1u); k = key; }
    }
    if (k == key) { atomicAdd(&s_cnt[h], c); return; }
  }
  if (lo_global_add(keys, cnt, mask, st, key, c)) atomicAdd(&s_ctr[1], 1u);   // a crowded LDS neighbourhood: straight to the global table
}

template <bool kVec, bool kMask>
__global__ __launch_bounds__(kLOThreads) void lo_count(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, const uint32_t* __restrict__ m,
                                                       unsigned long long N, uint32_t drop_a, uint32_t drop_b, unsigned long long steps_per_block,
                                                       unsigned long long* keys, unsigned long long* cnt, uint32_t mask, uint32_t* st,
                                                       unsigned long long* reserved) {
  __shared__ unsigned long long s_key[kLdsSlots];
  __shared__ uint32_t s_cnt[kLdsSlots];
  __shared__ uint32_t s_ctr[2];
  for (int i = threadIdx.x; i < kLdsSlots; i += kLOThreads) { s_key[i] = kEmptyKey; s_cnt[i] = 0; }
  if (threadIdx.x < 2) s_ctr[threadIdx.x] = 0;
  __syncthreads();
  uint32_t own_reserved = 0;                                 // voxels of the pair whose key is kEmptyKey
  auto add = [&](uint32_t va, uint32_t vb, uint32_t c) {
    const unsigned long long key = ((unsigned long long)va << 32) | vb;
    if (key == kEmptyKey) own_reserved += c;
    else lo_lds_add(s_key, s_cnt, s_ctr, keys, cnt, mask, st, key, c);
  };
  // The LDS table into the global one.  The keys in the global table are counted per workgroup and reported with ONE atomic per
  // flush (st[0]; a counter every insertion touched would be one hot word for the whole device); the workgroup whose report takes
  // the count past 3/4 of the slots marks the pass incomplete.
  auto flush = [&]() {
    uint32_t fresh = 0;
    for (int i = threadIdx.x; i < kLdsSlots; i += kLOThreads) {
      if (s_key[i] != kEmptyKey && lo_global_add(keys, cnt, mask, st, s_key[i], s_cnt[i])) ++fresh;
      s_key[i] = kEmptyKey; s_cnt[i] = 0;
    }
    if (fresh) atomicAdd(&s_ctr[1], fresh);
    __syncthreads();
    if (threadIdx.x == 0) {
      if (s_ctr[1] && atomicAdd(&st[0], s_ctr[1]) + s_ctr[1] > (mask + 1) / 4 * 3) atomicOr(&st[1], 1u);
      s_ctr[0] = 0; s_ctr[1] = 0;
    }
    __syncthreads();
  };
  const unsigned long long total = (N + kLOStep - 1) / kLOStep;
  const unsigned long long s0 = (unsigned long long)blockIdx.x * steps_per_block;
  const unsigned long long s1 = s0 + steps_per_block < total ? s0 + steps_per_block : total;
  for (unsigned long long s = s0; s < s1; s += kLOAhead) {
    uint32_t A[kLOAhead][4], B[kLOAhead][4], M[kLOAhead][4];
    int nv[kLOAhead];
#pragma unroll
    for (int k = 0; k < kLOAhead; ++k) {
      const unsigned long long i = (s + k) * kLOStep + (unsigned long long)threadIdx.x * 4;
      nv[k] = (s + k < s1 && i < N) ? (N - i < 4 ? (int)(N - i) : 4) : 0;
      if (kVec && nv[k] == 4) {
        const uint4 va = *reinterpret_cast<const uint4*>(a + i), vb = *reinterpret_cast<const uint4*>(b + i);
        A[k][0] = va.x; A[k][1] = va.y; A[k][2] = va.z; A[k][3] = va.w;
        B[k][0] = vb.x; B[k][1] = vb.y; B[k][2] = vb.z; B[k][3] = vb.w;
        if (kMask) { const uint4 vm = *reinterpret_cast<const uint4*>(m + i); M[k][0] = vm.x; M[k][1] = vm.y; M[k][2] = vm.z; M[k][3] = vm.w; }
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const bool in = q < nv[k];
          A[k][q] = in ? a[i + q] : 0u;
          B[k][q] = in ? b[i + q] : 0u;
          if (kMask) M[k][q] = in ? m[i + q] : 0u;
        }
      }
    }
    uint32_t ra = 0, rb = 0, rc = 0;                         // the run of equal pairs this lane is in (rc = 0: none)
#pragma unroll
    for (int k = 0; k < kLOAhead; ++k) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (q >= nv[k]) continue;
        const uint32_t va = A[k][q], vb = B[k][q];
        if ((kMask && M[k][q] == 0u) || (drop_a && va == 0u) || (drop_b && vb == 0u)) continue;
        if (rc && va == ra && vb == rb) { ++rc; continue; }
        if (rc) add(ra, rb, rc);
        ra = va; rb = vb; rc = 1;
      }
    }
    if (rc) add(ra, rb, rc);
    __syncthreads();
    const uint32_t used = s_ctr[0];                          // written by no thread between these two barriers
    __syncthreads();
    if (used > kLdsSlots / 2) flush();
  }
  flush();
  if (own_reserved) atomicAdd(reserved, (unsigned long long)own_reserved);
}

__global__ void lo_compact(const unsigned long long* keys, const unsigned long long* cnt, uint32_t cap, uint32_t* n_out,
                           unsigned long long* out_key, unsigned long long* out_cnt) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cap || keys[i] == kEmptyKey) return;
  const uint32_t j = atomicAdd(n_out, 1u);
  out_key[j] = keys[i];
  out_cnt[j] = cnt[i];
}

}  // namespace

int label_overlap(const uint32_t* d_a, const uint32_t* d_b, const uint32_t* d_mask, unsigned long long N, int flags, hipStream_t stream,
                  std::vector<glia_hmt_overlap_entry>* out, OverlapPass* info) {
  out->clear();
  *info = OverlapPass();
  DeviceBuffers buf;
  CallEvents<2> ev;
  int rc;
  if ((rc = ev.create())) return rc;
  unsigned long long* st64;                                  // [0] voxels of the reserved pair; then, as u32: keys in the table, incomplete pass, compacted
  if ((rc = buf.get(&st64, 4, false, stream))) return rc;
  uint32_t* st = reinterpret_cast<uint32_t*>(st64 + 1);
  const bool vec = ((uintptr_t)d_a % 16 == 0) && ((uintptr_t)d_b % 16 == 0) && ((uintptr_t)d_mask % 16 == 0);
  const unsigned long long steps = (N + kLOStep - 1) / kLOStep;
  const unsigned long long per_block = kLOStepsPerBlock;
  const unsigned long long blocks = (steps + per_block - 1) / per_block;      // <= 2^32 / 16 Ki = 262 144 workgroups
  // slots: the number of pairs is not known before the pass; one slot per 64 voxels to start with (a power of two between 2^16
  // and 2^26), doubled while a pass overflows
  unsigned long long cap = 1ull << 16;
  while (cap < N / 64 && cap < (1ull << 26)) cap <<= 1;
  if (option("GLIA_HMT_MINCAP")) cap = 1ull << 10;
  const uint32_t drop_a = (flags & GLIA_HMT_OVERLAP_DROP_ZERO_A) ? 1u : 0u, drop_b = (flags & GLIA_HMT_OVERLAP_DROP_ZERO_B) ? 1u : 0u;
  for (;;) {
    unsigned long long *keys, *cnt;
    if ((rc = buf.get(&keys, cap, false, stream)) || (rc = buf.get(&cnt, cap, true, stream))) return rc;
    GLIA_HIP_TRY(hipMemsetAsync(keys, 0xFF, 8 * cap, stream));
    GLIA_HIP_TRY(hipMemsetAsync(st64, 0, 32, stream));
    GLIA_HIP_TRY(hipEventRecord(ev.ev[0], stream));
#define GLIA_LO_LAUNCH(V, M)                                                                                                          \
  hipLaunchKernelGGL((lo_count<V, M>), dim3((unsigned)blocks), dim3(kLOThreads), 0, stream, d_a, d_b, d_mask, N, drop_a, drop_b, per_block, \
                     keys, cnt, (uint32_t)(cap - 1), st, st64)
    if (vec) { if (d_mask) GLIA_LO_LAUNCH(true, true); else GLIA_LO_LAUNCH(true, false); }
    else { if (d_mask) GLIA_LO_LAUNCH(false, true); else GLIA_LO_LAUNCH(false, false); }
#undef GLIA_LO_LAUNCH
    GLIA_HIP_TRY(hipGetLastError());
    GLIA_HIP_TRY(hipEventRecord(ev.ev[1], stream));
    unsigned long long h_st[2];                              // reserved pair | keys, incomplete
    GLIA_HIP_TRY(hipMemcpyAsync(h_st, st64, 16, hipMemcpyDeviceToHost, stream));
    GLIA_HIP_TRY(hipStreamSynchronize(stream));
    info->ms += ev.ms(0, 1);
    const uint32_t n = (uint32_t)h_st[1], incomplete = (uint32_t)(h_st[1] >> 32);
    if (incomplete) {
      if (cap >= (1ull << 31)) { set_error("label_overlap: contingency table beyond 2^31 slots"); return GLIA_HMT_ERR_CAPACITY; }
      cap <<= 1;
      ++info->repeats;
      continue;
    }
    std::vector<unsigned long long> hk(n), hc(n);
    if (n) {
      unsigned long long *ok, *oc, *sk, *sc;
      if ((rc = buf.get(&ok, n, false, stream)) || (rc = buf.get(&oc, n, false, stream)) || (rc = buf.get(&sk, n, false, stream)) ||
          (rc = buf.get(&sc, n, false, stream))) return rc;
      hipLaunchKernelGGL(lo_compact, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, stream, keys, cnt, (uint32_t)cap, st + 2, ok, oc);
      GLIA_HIP_TRY(hipGetLastError());
      // the keys are distinct, so the sorted order -- ascending (a, b) -- does not depend on the order the compaction left
      if ((rc = rocprim_run(buf, stream, [&](void* t, size_t& bytes) { return rocprim::radix_sort_pairs(t, bytes, ok, sk, oc, sc, (size_t)n, 0, 64, stream); })))
        return rc;
      GLIA_HIP_TRY(hipMemcpyAsync(hk.data(), sk, 8 * (size_t)n, hipMemcpyDeviceToHost, stream));
      GLIA_HIP_TRY(hipMemcpyAsync(hc.data(), sc, 8 * (size_t)n, hipMemcpyDeviceToHost, stream));
      GLIA_HIP_TRY(hipStreamSynchronize(stream));
    }
    out->resize((size_t)n + (h_st[0] ? 1 : 0));
    for (uint32_t i = 0; i < n; ++i) (*out)[i] = glia_hmt_overlap_entry{(uint32_t)(hk[i] >> 32), (uint32_t)hk[i], hc[i]};
    if (h_st[0]) out->back() = glia_hmt_overlap_entry{0xFFFFFFFFu, 0xFFFFFFFFu, h_st[0]};      // the largest key: it sorts last
    return GLIA_HMT_OK;
  }
}

}  // namespace glia
