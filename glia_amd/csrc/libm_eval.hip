// glia_amd/csrc/libm_eval.hip -- evaluates the device restatements of the host libm's logarithms, pow, exp and the sigmoid
// built on exp over an array (glia_hmt_libm_eval: parity tests compare the bits with the host's std:: functions; see glibc_math.hpp).
#include "bc_features.hpp"

namespace glia {

__global__ void libm_eval_kernel(int function, int variant, const double* __restrict__ in, double* __restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double x = in[i];
  // 3 = exp, 4 = the sigmoid of the classifier loop's MLP; variant 0: the device's own exp
  if (function == 3) out[i] = variant == kLibmFma ? glibc::exp_fma(x) : variant == kLibmSse2 ? glibc::exp_sse2(x) : exp(x);
  else if (function == 4) out[i] = glibc::sigmoid(x, variant);
  else out[i] = function == 0 ? feat::host_log2(x, variant) : function == 1 ? feat::host_log(x, variant) : feat::pow_perim(x, 3, variant);
}

int launch_libm_eval(int function, int variant, const double* d_in, double* d_out, int64_t n, hipStream_t stream) {
  if (n == 0) return GLIA_HMT_OK;
  libm_eval_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(function, variant, d_in, d_out, (long long)n);
  GLIA_HIP_TRY(hipGetLastError());
  return GLIA_HMT_OK;
}

}  // namespace glia
