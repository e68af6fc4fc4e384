// glia_amd/csrc/components.hip -- face-connected component labelling of a label volume (labelcc_image, labelicc_image).
//
// Reference:
//   labelIdentityConnectedComponents (util/image.hxx:331-373, gadget/main_labelicc_image.cxx): "Used to relabel 3D label sub-volume
//     cut from bigger volume" -- one breadth-first flood per component over equal labels, started in raster order;
//   labelConnectedComponents (util/image.hxx:302-313, gadget/main_labelcc_image.cxx) = itk::ConnectedComponentImageFilter with
//     SetFullyConnected(false) over the non-zero voxels; with --invert over the zero voxels (main_labelcc_image.cxx:10-18).
//
// Semantics (all three modes):
//   * a component is a maximal face-connected set of voxels that take part: 4 neighbours in 2D, 6 in 3D, in the reference order
//     -x, +x, -y, +y, -z, +z (type/neighbor.hxx:72-89; the order does not influence the result);
//   * components are numbered 1..n in raster order of their first voxel (x fastest); every other voxel gets 0 (BG_VAL);
//   * GLIA_HMT_CC_IDENTITY        a voxel takes part if label != 0 and not masked out; neighbours join if both take part and their
//                                 labels are equal;
//     GLIA_HMT_CC_BINARY          takes part if label != 0 and not masked out; neighbours join if both take part;
//     GLIA_HMT_CC_BINARY_INVERTED takes part if label == 0 and not masked out; neighbours join if both take part;
//   * mask: MASK_OUT_VAL = 0 masks a voxel out; it is then never a start and never a neighbour (image.hxx:349,
//     neighbor.hxx:80-86) and its output is 0.  The reference gives only the identity mode a mask: a mask in the binary modes is
//     an extension.
// The identity mode is plain C++ in the reference and pinned exactly.  The binary modes are an ITK filter: the partition is not in
// doubt, ITK's label order is unpinned (ITK is absent).
//
// Both modes are one rule on a KEY per voxel (0 = takes no part; identity: the label; binary: 1): neighbours join when their keys are
// equal and not 0.  Components are the sets of a union-find forest over voxel indices (union_find.hpp), built by one of two routes
// that give the same bytes (GLIA_HMT_CC = tiled | global):
//   global  the watershed's plateau step restated: every voxel is its own root, one pass unites the +x / +y / +z pairs with atomic
//           minimum links in global memory, one pass flattens.  The cross-check.
//   tiled   1. a workgroup loads a 16^3 (2D: 64^2) tile of keys into LDS, unites the pairs INSIDE the tile on LDS words (runs along
//              x by a wave ballot, the first y and z pair of each run with LDS atomics), and writes per voxel the global index of
//              its tile-local root (inside a box tile the local raster order and the global one agree, so the smallest local
//              index is the smallest global one);
//           2. a second launch visits only the voxel pairs that straddle a tile face and unites their roots in global memory --
//              of a run of equal pairs along a face only the first: step 1 joined the rest to it on either side;
//           3. a third launch flattens.
// Numbering, both routes: "p is a root" scanned exclusively over the volume (rocprim) gives rank[p] = roots before p, and
// out[p] = rank[root(p)] + 1.
//
// Invariants:
//   * a parent index is never larger than its child's (links are atomic minima from a root to a smaller root).  Every root walk
//     therefore ends in any interleaving, the root of a finished component is its smallest linear index, and the scan numbers
//     components in raster order without a sort;
//   * no kernel waits for another workgroup and nothing spins on a flag: the steps are separate launches and the launch boundary is
//     the only hand-over between workgroups.  Inside the tile kernel the hand-overs between waves go through __syncthreads();
//   * voxels that take no part hold kCcNone and are never walked: a walk starts at a voxel that takes part and follows links that
//     only unions of such voxels made;
//   * the input is read by every step up to the flatten (the face pass reads keys while other workgroups write parents), so the
//     volume is never labelled in place.
// Voxel indices are 32-bit (at most 2^32 - 2 voxels: kCcNone stays free); every arithmetic step on an index is 64-bit.
// Scratch: the output volume is the parent array; the ranks are 4 bytes per voxel from the block cache, plus rocprim's scan storage.
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "greedy_common.hpp"
#include "hmt_internal.hpp"
#include "union_find.hpp"

namespace glia {
namespace {

constexpr uint32_t kCcNone = 0xFFFFFFFFu;
struct CcGrid { long long nx, ny, nz, n; int dim, mode; };

__device__ __forceinline__ uint32_t cc_key(const CcGrid& G, const uint32_t* lab, const uint32_t* mask, long long p) {
  if (mask && mask[p] == 0u) return 0u;
  const uint32_t l = lab[p];
  if (G.mode == GLIA_HMT_CC_IDENTITY) return l;
  return ((l != 0u) == (G.mode == GLIA_HMT_CC_BINARY)) ? 1u : 0u;
}

// ---- global route -----------------------------------------------------------------------------------------------------------
__global__ void cc_init(CcGrid G, const uint32_t* lab, const uint32_t* mask, uint32_t* parent) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p < G.n) parent[p] = cc_key(G, lab, mask, p) ? (uint32_t)p : kCcNone;
}
__global__ void cc_unite_all(CcGrid G, const uint32_t* lab, const uint32_t* mask, uint32_t* parent) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= G.n) return;
  const uint32_t k = cc_key(G, lab, mask, p);
  if (!k) return;
  const long long x = p % G.nx, y = (p / G.nx) % G.ny, z = p / (G.nx * G.ny);
  constexpr int S = __HIP_MEMORY_SCOPE_AGENT;
  if (x + 1 < G.nx && cc_key(G, lab, mask, p + 1) == k) uf_unite<S>(parent, (uint32_t)p, (uint32_t)(p + 1));
  if (y + 1 < G.ny && cc_key(G, lab, mask, p + G.nx) == k) uf_unite<S>(parent, (uint32_t)p, (uint32_t)(p + G.nx));
  if (G.dim == 3 && z + 1 < G.nz && cc_key(G, lab, mask, p + G.nx * G.ny) == k) uf_unite<S>(parent, (uint32_t)p, (uint32_t)(p + G.nx * G.ny));
}

// ---- tiled route ------------------------------------------------------------------------------------------------------------
constexpr int kCcThreads = 512;
constexpr int kCcCells = 4096;                // 16^3 = 64^2
template <bool D3> struct CcTile {
  static constexpr int tx = D3 ? 16 : 64, ty = D3 ? 16 : 64, tz = D3 ? 16 : 1;
};
static_assert(CcTile<true>::tx * CcTile<true>::ty * CcTile<true>::tz == kCcCells && CcTile<false>::tx * CcTile<false>::ty == kCcCells, "tile = kCcCells");
static_assert(64 % CcTile<true>::tx == 0 && 64 % CcTile<false>::tx == 0 && kCcThreads % 64 == 0 && kCcCells % kCcThreads == 0, "a wave holds whole rows");

template <bool D3>
__global__ __launch_bounds__(kCcThreads) void cc_tile_local(CcGrid G, const uint32_t* lab, const uint32_t* mask, uint32_t* parent) {
  using T = CcTile<D3>;
  __shared__ uint32_t skey[kCcCells];
  __shared__ uint32_t spar[kCcCells];
  constexpr int S = __HIP_MEMORY_SCOPE_WORKGROUP;
  const long long nbx = (G.nx + T::tx - 1) / T::tx, nby = (G.ny + T::ty - 1) / T::ty;
  const long long b = blockIdx.x;
  const long long x0 = (b % nbx) * T::tx, y0 = ((b / nbx) % nby) * T::ty, z0 = (b / (nbx * nby)) * T::tz;
  for (int c = threadIdx.x; c < kCcCells; c += kCcThreads) {
    const long long x = x0 + c % T::tx, y = y0 + (c / T::tx) % T::ty, z = z0 + c / (T::tx * T::ty);
    const uint32_t k = (x < G.nx && y < G.ny && z < G.nz) ? cc_key(G, lab, mask, (z * G.ny + y) * G.nx + x) : 0u;   // outside the volume: no part
    skey[c] = k;
    // x pairs without an atomic: a wave holds whole rows (64 consecutive cells, tx divides 64), so every voxel starts under the
    // first voxel of its run of equal keys along x -- a root, and not larger than the voxel
    const uint32_t left = __shfl_up(k, 1);           // by every lane, before any condition: an inactive lane would give nothing
    const bool first = c % T::tx == 0 || left != k;
    const int lane = threadIdx.x & 63;
    const unsigned long long firsts = __ballot(first) & (~0ull >> (63 - lane));      // lanes 0..lane: never empty, a row starts there
    spar[c] = k ? (uint32_t)(c - (lane - (63 - __clzll((long long)firsts)))) : kCcNone;
  }
  __syncthreads();
  // y and z pairs: of a run of equal pairs along x only the first is united -- the runs above joined the rest to it on either side
  for (int c = threadIdx.x; c < kCcCells; c += kCcThreads) {
    const uint32_t k = skey[c];
    if (!k) continue;
    const int cx = c % T::tx, cy = (c / T::tx) % T::ty, cz = c / (T::tx * T::ty);
    const bool run = cx > 0 && skey[c - 1] == k;
    if (cy + 1 < T::ty && skey[c + T::tx] == k && !(run && skey[c + T::tx - 1] == k)) uf_unite<S>(spar, (uint32_t)c, (uint32_t)(c + T::tx));
    if (D3 && cz + 1 < T::tz && skey[c + T::tx * T::ty] == k && !(run && skey[c + T::tx * T::ty - 1] == k))
      uf_unite<S>(spar, (uint32_t)c, (uint32_t)(c + T::tx * T::ty));
  }
  __syncthreads();
  // the forest is final: walks only read it.  Each voxel writes the GLOBAL index of its tile-local root.
  for (int c = threadIdx.x; c < kCcCells; c += kCcThreads) {
    const long long x = x0 + c % T::tx, y = y0 + (c / T::tx) % T::ty, z = z0 + c / (T::tx * T::ty);
    if (x >= G.nx || y >= G.ny || z >= G.nz) continue;
    uint32_t g = kCcNone;
    if (skey[c]) {
      const int r = (int)uf_root<S>(spar, (uint32_t)c);
      g = (uint32_t)(((z0 + r / (T::tx * T::ty)) * G.ny + (y0 + (r / T::tx) % T::ty)) * G.nx + (x0 + r % T::tx));
    }
    parent[(z * G.ny + y) * G.nx + x] = g;
  }
}

// one thread per voxel pair that straddles a tile face: fx pairs across x faces, then fy across y faces, then fz across z faces
template <bool D3>
__global__ void cc_tile_faces(CcGrid G, const uint32_t* lab, const uint32_t* mask, uint32_t* parent, long long fx, long long fy, long long fz) {
  using T = CcTile<D3>;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long x, y, z, stride;
  // back1 / back2: the step to the pair before this one along each of the face's two axes, 0 where that pair lies in other tiles
  long long back1, back2;
  const long long sy = G.nx, sz = G.nx * G.ny;
  if (i < fx) {
    const long long faces = (G.nx + T::tx - 1) / T::tx - 1;
    x = (i % faces + 1) * T::tx - 1; i /= faces; y = i % G.ny; z = i / G.ny; stride = 1;
    back1 = y % T::ty ? sy : 0; back2 = z % T::tz ? sz : 0;
  } else if (i - fx < fy) {
    i -= fx;
    const long long faces = (G.ny + T::ty - 1) / T::ty - 1;
    x = i % G.nx; i /= G.nx; y = (i % faces + 1) * T::ty - 1; z = i / faces; stride = sy;
    back1 = x % T::tx ? 1 : 0; back2 = z % T::tz ? sz : 0;
  } else if (i - fx - fy < fz) {
    i -= fx + fy;
    x = i % G.nx; i /= G.nx; y = i % G.ny; z = (i / G.ny + 1) * T::tz - 1; stride = sz;
    back1 = x % T::tx ? 1 : 0; back2 = y % T::ty ? sy : 0;
  } else return;
  const long long p = (z * G.ny + y) * G.nx + x, q = p + stride;
  const uint32_t k = cc_key(G, lab, mask, p);
  if (!k || cc_key(G, lab, mask, q) != k) return;
  // Only the first pair of a run is united.  If the pair before this one (same two tiles) has the same key on both sides, step 1
  // joined p to that pair's voxel on this side and q to the one on the other side, and that pair is united -- by its own thread or,
  // by this rule again, through a pair before it (the pairs of a face are ordered, so the chain ends at a pair that is united).
  if (back1 && cc_key(G, lab, mask, p - back1) == k && cc_key(G, lab, mask, q - back1) == k) return;
  if (back2 && cc_key(G, lab, mask, p - back2) == k && cc_key(G, lab, mask, q - back2) == k) return;
  uf_unite<__HIP_MEMORY_SCOPE_AGENT>(parent, (uint32_t)p, (uint32_t)q);
}

// ---- both routes ------------------------------------------------------------------------------------------------------------
__global__ void cc_flatten(CcGrid G, uint32_t* parent) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= G.n) return;
  const uint32_t v = parent[p];                       // only this thread writes parent[p]
  if (v == kCcNone) return;
  const uint32_t r = uf_root<__HIP_MEMORY_SCOPE_AGENT>(parent, v);
  if (r != v) parent[p] = r;
}
struct CcIsRoot {
  const uint32_t* parent;
  __host__ __device__ uint32_t operator()(size_t p) const { return parent[p] == (uint32_t)p ? 1u : 0u; }
};
// in place over the flattened parents: a thread reads only its own parent word before it overwrites it
__global__ void cc_number(CcGrid G, const uint32_t* rank, uint32_t* out) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= G.n) return;
  const uint32_t r = out[p];
  out[p] = r == kCcNone ? 0u : rank[r] + 1u;
}

}  // namespace

int label_components(int dim, const int64_t dims[3], const uint32_t* d_in, const uint32_t* d_mask, int mode, int route, uint32_t* d_out,
                     uint32_t* n_components, hipStream_t stream) {
  CcGrid G;
  G.dim = dim; G.mode = mode; G.nx = dims[0]; G.ny = dims[1]; G.nz = dim == 3 ? dims[2] : 1; G.n = G.nx * G.ny * G.nz;
  const long long n = G.n;
  const unsigned blocks = (unsigned)((n + 255) / 256);
  uint32_t* const parent = d_out;
  DeviceBuffers buf;
  uint32_t* rank = nullptr;
  if (int rc = buf.get(&rank, (size_t)n, false, stream)) return rc;
  if (route == GLIA_HMT_CC_ROUTE_GLOBAL) {
    hipLaunchKernelGGL(cc_init, dim3(blocks), dim3(256), 0, stream, G, d_in, d_mask, parent);
    hipLaunchKernelGGL(cc_unite_all, dim3(blocks), dim3(256), 0, stream, G, d_in, d_mask, parent);
  } else {
    const long long tx = dim == 3 ? CcTile<true>::tx : CcTile<false>::tx, tz = dim == 3 ? CcTile<true>::tz : 1;
    const long long nbx = (G.nx + tx - 1) / tx, nby = (G.ny + tx - 1) / tx, nbz = (G.nz + tz - 1) / tz;
    const long long fx = (nbx - 1) * G.ny * G.nz, fy = (nby - 1) * G.nx * G.nz, fz = (nbz - 1) * G.nx * G.ny;
    const unsigned tiles = (unsigned)(nbx * nby * nbz), fblocks = (unsigned)((fx + fy + fz + 255) / 256);
    if (dim == 3) {
      hipLaunchKernelGGL(cc_tile_local<true>, dim3(tiles), dim3(kCcThreads), 0, stream, G, d_in, d_mask, parent);
      if (fblocks) hipLaunchKernelGGL(cc_tile_faces<true>, dim3(fblocks), dim3(256), 0, stream, G, d_in, d_mask, parent, fx, fy, fz);
    } else {
      hipLaunchKernelGGL(cc_tile_local<false>, dim3(tiles), dim3(kCcThreads), 0, stream, G, d_in, d_mask, parent);
      if (fblocks) hipLaunchKernelGGL(cc_tile_faces<false>, dim3(fblocks), dim3(256), 0, stream, G, d_in, d_mask, parent, fx, fy, fz);
    }
  }
  hipLaunchKernelGGL(cc_flatten, dim3(blocks), dim3(256), 0, stream, G, parent);
  GLIA_HIP_TRY(hipGetLastError());
  const auto flags = rocprim::make_transform_iterator(rocprim::counting_iterator<size_t>(0), CcIsRoot{parent});
  if (int rc = rocprim_run(buf, stream, [&](void* t, size_t& b) {
        return rocprim::exclusive_scan(t, b, flags, rank, 0u, (size_t)n, rocprim::plus<uint32_t>(), stream); })) return rc;
  uint32_t last[2] = {0, 0};                          // components = rank[n-1] + (voxel n-1 is a root)
  GLIA_HIP_TRY(hipMemcpyAsync(&last[0], rank + (n - 1), 4, hipMemcpyDeviceToHost, stream));
  GLIA_HIP_TRY(hipMemcpyAsync(&last[1], parent + (n - 1), 4, hipMemcpyDeviceToHost, stream));
  hipLaunchKernelGGL(cc_number, dim3(blocks), dim3(256), 0, stream, G, rank, d_out);
  GLIA_HIP_TRY(hipGetLastError());
  GLIA_HIP_TRY(hipStreamSynchronize(stream));         // the blocks go back to the cache when buf dies: nothing may still use them
  *n_components = last[0] + (last[1] == (uint32_t)(n - 1) ? 1u : 0u);
  return GLIA_HMT_OK;
}

}  // namespace glia
