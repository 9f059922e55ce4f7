// lzm_search_sampled_mlp.hip — the one-launch Sampled EfficientZero search's kernels (lzm_search_sampled_mlp.h) and
// their launcher. The plan, the schedule, the argument checks and the error text live with the C entry points in
// lzm_kernels.hip.
#include <hip/hip_runtime.h>

#define LZM_DEVICE_HELPERS_ONLY  // the shared headers' device helpers without their kernels (lzm_kernels.hip's)
#include "lzm_search_sampled_mlp.h"

namespace lzm {

hipError_t sampled_mlp_launch(const SampledSearchArgs &p, int R, bool tree_in_lds, size_t lds, hipStream_t stream) {
  typedef void (*Kernel)(SampledSearchArgs);
  static const Kernel kernels[3][2] = {  // [R = 1, 2, 4][tree in LDS, tree in HBM]
      {search_sampled_mlp_kernel<1, true>, search_sampled_mlp_kernel<1, false>},
      {search_sampled_mlp_kernel<2, true>, search_sampled_mlp_kernel<2, false>},
      {search_sampled_mlp_kernel<4, true>, search_sampled_mlp_kernel<4, false>}};
  if (R != 1 && R != 2 && R != 4) return hipErrorInvalidValue;
  const Kernel fn = kernels[R == 1 ? 0 : R == 2 ? 1 : 2][tree_in_lds ? 0 : 1];
  const hipError_t e = hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fn, dim3((p.B + R - 1) / R), dim3(kThreads), lds, stream, p);
  return hipGetLastError();
}

}  // namespace lzm
