// Self-test of the field and scalar primitives (one of the translation units, see launch.h; the CROSS-CHECK build only).
//   k_fe_selftest   one item per lane, one op per launch: selftest_ops.h fe_selftest_item on caller-supplied raw limbs
//                   (tests/test_gpu_field_bounds.py: limb for limb against the host twin, values against Python integers)
#include <hip/hip_runtime.h>
#include "launch.h"
#include "selftest_ops.h"
using namespace kyb;

#ifdef KYB_CROSSCHECK
// a, b, c, out: 16 words per item; param: one word per item
__global__ void __launch_bounds__(64)
k_fe_selftest(uint32_t op, size_t n, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, const uint32_t* __restrict__ c,
              const uint32_t* __restrict__ param, uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t A[16], B[16], C[16], O[16];
  KYB_UNROLL for (int j = 0; j < 16; ++j) { A[j] = a[16 * i + j]; B[j] = b[16 * i + j]; C[j] = c[16 * i + j]; }
  fe_selftest_item(op, A, B, C, param[i], O);
  KYB_UNROLL for (int j = 0; j < 16; ++j) out[16 * i + j] = O[j];
}

namespace kyb { namespace launch {
hipError_t fe_selftest(hipStream_t st, uint32_t op, size_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* param, uint32_t* out) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_fe_selftest, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, op, n, a, b, c, param, out);
  return hipGetLastError();
}
}}  // namespace kyb::launch
#endif
