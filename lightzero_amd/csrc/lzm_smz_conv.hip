// lzm_smz_conv.hip — the Stochastic MuZero conv step kernel (lzm_smz_conv.h) and its launcher. Argument checks, the
// weight packing and the error text live with the C entry points in lzm_kernels.hip.
#include <hip/hip_runtime.h>

#include "lzm_smz_conv.h"

namespace lzm {

template <int NRES, int P>
static hipError_t smz_conv_launch(const SmzConvArgs &a, hipStream_t s) {
  hipLaunchKernelGGL((smz_conv_step_kernel<NRES, P>), dim3((a.B + P - 1) / P), dim3(kSmzThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t smz_conv_launch_step(int nres, int positions, const SmzConvArgs &a, hipStream_t s) {
  if (positions == 0) positions = kSmzBoards;
  if (positions == 2) return nres == 1 ? smz_conv_launch<1, 2>(a, s) : smz_conv_launch<2, 2>(a, s);
  return nres == 1 ? smz_conv_launch<1, 1>(a, s) : smz_conv_launch<2, 1>(a, s);
}

}  // namespace lzm
