// lzm_az_gomoku_n_split.hip — the split-fp16 Gomoku 9 x 9 / 15 x 15 network kernel (lzm_az_gomoku_n_net_split.h) and
// its launcher; a unit of its own so that lzm_az_gomoku_n.hip, the exact-f32 kernels' unit, compiles as before.
// Argument checks and the error text live with the C entry points in lzm_kernels.hip.
#include <hip/hip_runtime.h>

#include <atomic>

#define LZM_DEVICE_HELPERS_ONLY  // lzm_conv.h's split-scheme helpers without its kernels (lzm_kernels.hip's)
#include "lzm_az_gomoku_n_net_split.h"

namespace lzm {

template <int NRES, int N>
static hipError_t gmkn_net_split_launch(const float *w, const float *state, int n, float *probs, float *value,
                                        int32_t *err, hipStream_t s) {
  constexpr size_t lds = (size_t)Gns<N>::lds_bytes;
  static std::atomic<bool> attr[64];  // per device ordinal, as gmkn_net_launch
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= 64 || !attr[dev].load(std::memory_order_acquire)) {
    e = hipFuncSetAttribute((const void *)gomoku_n_net_eval_split_kernel<NRES, N>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 64) attr[dev].store(true, std::memory_order_release);
  }
  hipLaunchKernelGGL((gomoku_n_net_eval_split_kernel<NRES, N>), dim3(n), dim3(kGnsThreads), lds, s, w, state, n, probs,
                     value, err);
  return hipGetLastError();
}

template <int N>
static hipError_t gmkn_net_split_launch_n(int nres, const float *w, const float *state, int n, float *probs,
                                          float *value, int32_t *err, hipStream_t s) {
  return nres == 1 ? gmkn_net_split_launch<1, N>(w, state, n, probs, value, err, s)
                   : gmkn_net_split_launch<2, N>(w, state, n, probs, value, err, s);
}

hipError_t gmkn_launch_net_split_eval(int n_board, int nres, const float *w, const float *state, int n, float *probs,
                                      float *value, int32_t *err, hipStream_t s) {
  return n_board == 9 ? gmkn_net_split_launch_n<9>(nres, w, state, n, probs, value, err, s)
                      : gmkn_net_split_launch_n<15>(nres, w, state, n, probs, value, err, s);
}

}  // namespace lzm
