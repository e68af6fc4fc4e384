// glia_amd/csrc/blur.hip -- blur_image on the device: separable discrete Gaussian smoothing of a volume.
//
// Reference: blurImage (util/image.hxx:376-407, gadget/main_blur_image.cxx) = itk::DiscreteGaussianImageFilter; the definition that
// is reproduced bit for bit is this project's own (include/glia_hmt.h, gaussian_kernel.hpp: the host function every route must equal).
//
// One axis pass:  out[p] = f32( sum_{o = -r..+r} c[|o|] * (double) in[clamp(p + o e_axis)] ), o ascending from an accumulator of
// +0.0, product and sum rounded apart (the library is built with -ffp-contract=off), x then y then z.  An axis that is left alone
// is a copy of the bits (radius -1 below), never a pass with the kernel {1}: that would turn -0.0 into +0.0 and quiet a NaN.
//
// Two routes to the same bytes (GLIA_HMT_BLUR = passes | march):
//   passes  one launch per blurred axis; a thread walks 8 rows at its x and reads 2 r + 1 clamped taps per voxel from global memory
//           (the neighbours of a wave's 64 voxels along y and z are again 64 consecutive voxels: every tap is a coalesced read,
//           re-reads are served by the caches).  Intermediate volumes are float32 scratch.  Any radius.
//   march   a workgroup of 256 threads owns a tile of kBlurTileX x kBlurTileY voxels and a run of kBlurChunkZ planes.  Per input plane:
//             1. tile + halo (clamped coordinates) -> LDS as float32;
//             2. x pass over the tile's rows and its y-halo rows -> LDS, rounded to float32;
//             3. y pass -> the next slot of a ring of 2 rz + 1 of x-y blurred planes in LDS -- or straight to global memory when z is
//                left alone (2D, skip_axis = 2): then there is no ring;
//             4. the z pass of plane z - rz over the ring -> global memory.
//           The z pass reads the x-y blurred volume at clamped z, so the ring needs no special first or last plane: plane
//           clamp(z + o) is in the ring because the walk starts at max(0, z0 - rz) and simply stops computing planes past nz - 1.
//           A run of planes re-computes rz planes on either side (2 rz / kBlurChunkZ more reads), which buys workgroups for every CU.
//           LDS: all three arrays are indexed by consecutive lanes with stride 1 (a wave is one row of 64 voxels), so every access
//           is conflict-free; static, 59,408 B of the 64 KiB a kernel may declare statically (two workgroups per CU) -- that is what
//           limits kBlurMarchRadius to 5.  Barriers: after 1, after 2, and after 3 when there is a ring; step 4 and the next plane's
//           step 1 touch different arrays and need none.
// Voxel indices are 64-bit throughout.  No kernel writes outside [0, n): every store is guarded by x < nx, y < ny, z < z1 <= nz.
#include "gaussian_kernel.hpp"
#include "greedy_common.hpp"
#include "hmt_internal.hpp"

namespace glia {
namespace {

struct BlurGrid { long long nx, ny, nz; };

__device__ __forceinline__ float blur_load(const void* p, int type, long long i) {
  if (type == GLIA_HMT_PIXEL_UINT8) return (float)((const uint8_t*)p)[i];
  if (type == GLIA_HMT_PIXEL_UINT16) return (float)((const uint16_t*)p)[i];
  return ((const float*)p)[i];
}
__device__ __forceinline__ void blur_store(void* p, int type, long long i, float v) {
  if (type == GLIA_HMT_PIXEL_UINT8) ((uint8_t*)p)[i] = blur_to_integer<uint8_t>(v);
  else if (type == GLIA_HMT_PIXEL_UINT16) ((uint16_t*)p)[i] = blur_to_integer<uint16_t>(v);
  else ((float*)p)[i] = v;
}
__device__ __forceinline__ long long blur_clamp(long long v, long long hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// ---- passes route -----------------------------------------------------------------------------------------------------------
struct PassTaps { int radius; double c[kBlurMaxRadius + 1]; };

// a workgroup owns 256 consecutive x of kBlurPassRows consecutive rows of the planes z, z + gz, ... (gz planes are in the grid: all of
// them unless the grid would pass 2^31 - 1 workgroups): the three divisions that locate it are 32-bit and paid once per thread, not
// per voxel
constexpr int kBlurPassRows = 8;
__global__ __launch_bounds__(256) void blur_pass(BlurGrid G, uint32_t gz, int axis, PassTaps k, int in_type, int out_type, const void* in, void* out) {
  const uint32_t nbx = (uint32_t)((G.nx + 255) / 256), nby = (uint32_t)((G.ny + kBlurPassRows - 1) / kBlurPassRows);
  const uint32_t b = blockIdx.x, bx = b % nbx, by = (b / nbx) % nby;
  const long long x = (long long)bx * 256 + threadIdx.x, y0 = (long long)by * kBlurPassRows;
  if (x >= G.nx) return;
  const long long extent = axis == 0 ? G.nx : axis == 1 ? G.ny : G.nz, stride = axis == 0 ? 1 : axis == 1 ? G.nx : G.nx * G.ny;
  for (long long z = b / (nbx * nby); z < G.nz; z += gz)
  for (long long y = y0; y < y0 + kBlurPassRows && y < G.ny; ++y) {
    const long long p = (z * G.ny + y) * G.nx + x, at = axis == 0 ? x : axis == 1 ? y : z;
    double acc = 0.0;
    for (int o = -k.radius; o <= k.radius; ++o) {
      const long long q = blur_clamp(at + o, extent - 1);
      acc = acc + k.c[o < 0 ? -o : o] * (double)blur_load(in, in_type, p + (q - at) * stride);
    }
    blur_store(out, out_type, p, (float)acc);
  }
}

// ---- march route ------------------------------------------------------------------------------------------------------------
constexpr int kBlurThreads = 256;
constexpr int kBlurChunkZ = 64;                                     // planes a workgroup writes
constexpr int kBlurTile = kBlurTileX * kBlurTileY;
constexpr int kBlurHaloX = kBlurTileX + 2 * kBlurMarchRadius, kBlurHaloY = kBlurTileY + 2 * kBlurMarchRadius;
static_assert(4 * (kBlurHaloX * kBlurHaloY + kBlurTileX * kBlurHaloY + (2 * kBlurMarchRadius + 1) * kBlurTile) <= 65536, "static LDS: 64 KiB");
static_assert(kBlurTileX == 64, "a wave is one row of the tile");

struct MarchTaps { int r[3]; double c[3][kBlurMarchRadius + 1]; };   // r[a] = -1: axis a is left alone

template <bool RING>
__global__ __launch_bounds__(kBlurThreads) void blur_march(BlurGrid G, MarchTaps k, int in_type, int out_type, const void* in, void* out) {
  __shared__ float s_in[kBlurHaloX * kBlurHaloY];                   // tile + halo of the input plane
  __shared__ float s_x[kBlurTileX * kBlurHaloY];                    // its x pass: the tile's columns, rows with the y halo
  __shared__ float s_ring[RING ? (2 * kBlurMarchRadius + 1) * kBlurTile : 1];   // x-y blurred planes, slot = (z - first plane of the walk) mod (2 rz + 1)
  const int rx = k.r[0] < 0 ? 0 : k.r[0], ry = k.r[1] < 0 ? 0 : k.r[1], rz = RING ? k.r[2] : 0;
  const int w_in = kBlurTileX + 2 * rx, rows = kBlurTileY + 2 * ry, slots = 2 * rz + 1;
  const long long nbx = (G.nx + kBlurTileX - 1) / kBlurTileX, nby = (G.ny + kBlurTileY - 1) / kBlurTileY;
  const long long b = blockIdx.x;
  const long long x0 = (b % nbx) * kBlurTileX, y0 = ((b / nbx) % nby) * kBlurTileY, z0 = (b / (nbx * nby)) * kBlurChunkZ;
  const long long z1 = z0 + kBlurChunkZ < G.nz ? z0 + kBlurChunkZ : G.nz;
  const int tid = threadIdx.x;
  const long long first = RING ? (z0 - rz > 0 ? z0 - rz : 0) : z0, last = z1 - 1 + rz;
  int slot_in = 0;                                                  // slot of plane zi = (zi - first) mod slots, counted, not divided
  for (long long zi = first; zi <= last; ++zi) {
    if (zi < G.nz) {                                                // (uniform over the workgroup: the barriers below are reached by all)
      for (int yy = tid / 64; yy < rows; yy += kBlurThreads / 64) {            // a wave loads a row: no division by the row length
        const long long row = (zi * G.ny + blur_clamp(y0 - ry + yy, G.ny - 1)) * G.nx;
        for (int xx = tid % 64; xx < w_in; xx += 64) s_in[yy * w_in + xx] = blur_load(in, in_type, row + blur_clamp(x0 - rx + xx, G.nx - 1));
      }
      __syncthreads();
      for (int i = tid; i < rows * kBlurTileX; i += kBlurThreads) {
        const float* row = s_in + (i / kBlurTileX) * w_in + i % kBlurTileX + rx;
        float v = row[0];
        if (k.r[0] >= 0) {
          double acc = 0.0;
          for (int o = -rx; o <= rx; ++o) acc = acc + k.c[0][o < 0 ? -o : o] * (double)row[o];
          v = (float)acc;
        }
        s_x[i] = v;
      }
      __syncthreads();
      for (int i = tid; i < kBlurTile; i += kBlurThreads) {
        const float* col = s_x + i + ry * kBlurTileX;
        float v = col[0];
        if (k.r[1] >= 0) {
          double acc = 0.0;
          for (int o = -ry; o <= ry; ++o) acc = acc + k.c[1][o < 0 ? -o : o] * (double)col[o * kBlurTileX];
          v = (float)acc;
        }
        if (RING) s_ring[slot_in * kBlurTile + i] = v;
        else {
          const long long x = x0 + i % kBlurTileX, y = y0 + i / kBlurTileX;
          if (x < G.nx && y < G.ny) blur_store(out, out_type, (zi * G.ny + y) * G.nx + x, v);
        }
      }
      if (RING) { __syncthreads(); slot_in = slot_in + 1 == slots ? 0 : slot_in + 1; }
    }
    if (!RING) continue;
    const long long zo = zi - rz;                                   // its planes clamp(zo - rz .. zo + rz) are all in the ring now
    if (zo < z0) continue;
    const long long q_lo = blur_clamp(zo - rz, G.nz - 1);
    const int slot_lo = (int)((uint32_t)(q_lo - first) % (uint32_t)slots);   // once per plane; the taps step from it
    for (int i = tid; i < kBlurTile; i += kBlurThreads) {
      const long long x = x0 + i % kBlurTileX, y = y0 + i / kBlurTileX;
      if (x >= G.nx || y >= G.ny) continue;
      double acc = 0.0;
      long long q_was = q_lo;
      int slot = slot_lo;
      for (int o = -rz; o <= rz; ++o) {
        const long long q = blur_clamp(zo + o, G.nz - 1);
        if (q != q_was) { slot = slot + 1 == slots ? 0 : slot + 1; q_was = q; }   // clamped taps repeat a plane, the others step by one
        acc = acc + k.c[2][o < 0 ? -o : o] * (double)s_ring[slot * kBlurTile + i];
      }
      blur_store(out, out_type, (zo * G.ny + y) * G.nx + x, (float)acc);
    }
  }
}

}  // namespace

int blur_image_device(int dim, const int64_t dims[3], int pixel_type, const void* d_in, const GaussianKernel* const taps[3], int route, void* d_out,
                      hipStream_t stream, double* ms, int* route_used) {
  BlurGrid G;
  G.nx = dims[0]; G.ny = dims[1]; G.nz = dim == 3 ? dims[2] : 1;
  const long long n = G.nx * G.ny * G.nz;
  const size_t px = pixel_type == GLIA_HMT_PIXEL_UINT8 ? 1 : pixel_type == GLIA_HMT_PIXEL_UINT16 ? 2 : 4;
  int blurred = 0, widest = 0;
  for (int a = 0; a < 3; ++a) if (taps[a]) { ++blurred; widest = std::max(widest, taps[a]->radius); }
  if (route == GLIA_HMT_BLUR_ROUTE_MARCH && widest > kBlurMarchRadius) route = GLIA_HMT_BLUR_ROUTE_PASSES;
  CallEvents<2> ev;
  if (int rc = ev.create()) return rc;
  DeviceBuffers buf;
  GLIA_HIP_TRY(hipEventRecord(ev.ev[0], stream));
  if (!blurred) GLIA_HIP_TRY(hipMemcpyAsync(d_out, d_in, (size_t)n * px, hipMemcpyDeviceToDevice, stream));
  else if (route == GLIA_HMT_BLUR_ROUTE_MARCH) {
    MarchTaps k;
    for (int a = 0; a < 3; ++a) {
      k.r[a] = taps[a] ? taps[a]->radius : -1;
      for (int i = 0; i <= kBlurMarchRadius; ++i) k.c[a][i] = taps[a] && i <= taps[a]->radius ? taps[a]->c[(size_t)i] : 0.0;
    }
    const long long nbx = (G.nx + kBlurTileX - 1) / kBlurTileX, nby = (G.ny + kBlurTileY - 1) / kBlurTileY, nbz = (G.nz + kBlurChunkZ - 1) / kBlurChunkZ;
    const dim3 grid((unsigned)(nbx * nby * nbz)), block(kBlurThreads);
    if (taps[2]) hipLaunchKernelGGL(blur_march<true>, grid, block, 0, stream, G, k, pixel_type, pixel_type, d_in, d_out);
    else hipLaunchKernelGGL(blur_march<false>, grid, block, 0, stream, G, k, pixel_type, pixel_type, d_in, d_out);
    GLIA_HIP_TRY(hipGetLastError());
  } else {
    // in -> scratch -> scratch -> out: one float32 volume per pass but the last
    const void* src = d_in;
    int src_type = pixel_type, done = 0;
    for (int a = 0; a < 3; ++a) {
      if (!taps[a]) continue;
      const bool is_last = ++done == blurred;
      void* dst = d_out;
      if (!is_last) { float* s = nullptr; if (int rc = buf.get(&s, (size_t)n, false, stream)) return rc; dst = s; }
      PassTaps k;
      k.radius = taps[a]->radius;
      for (int i = 0; i <= kBlurMaxRadius; ++i) k.c[i] = i <= k.radius ? taps[a]->c[(size_t)i] : 0.0;
      const int dst_type = is_last ? pixel_type : GLIA_HMT_PIXEL_FLOAT32;
      const long long per_plane = ((G.nx + 255) / 256) * ((G.ny + kBlurPassRows - 1) / kBlurPassRows);
      const long long gz = std::min<long long>(G.nz, std::max<long long>(1, 0x7FFFFFFFll / per_plane));
      hipLaunchKernelGGL(blur_pass, dim3((unsigned)(per_plane * gz)), dim3(256), 0, stream, G, (uint32_t)gz, a, k, src_type, dst_type, src, dst);
      GLIA_HIP_TRY(hipGetLastError());
      src = dst; src_type = GLIA_HMT_PIXEL_FLOAT32;
    }
  }
  GLIA_HIP_TRY(hipEventRecord(ev.ev[1], stream));
  GLIA_HIP_TRY(hipStreamSynchronize(stream));         // the scratch goes back to the cache when buf dies: nothing may still use it
  *ms = ev.ms(0, 1);
  *route_used = route;
  return GLIA_HMT_OK;
}

}  // namespace glia
