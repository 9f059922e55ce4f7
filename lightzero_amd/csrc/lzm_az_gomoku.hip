// lzm_az_gomoku.hip — the Gomoku AlphaZero kernels (lzm_az_gomoku.h, lzm_az_gomoku_net.h) and their launchers.
// Argument checks, the workspace carve and the error text live with the C entry points in lzm_kernels.hip.
#include <hip/hip_runtime.h>

#include <atomic>

#include "lzm_az_gomoku.h"
#include "lzm_az_gomoku_net.h"

namespace lzm {

hipError_t gmk_launch_begin(const GmkTree &t, const int32_t *boards, const int32_t *start_index, float *state,
                            hipStream_t s) {
  hipLaunchKernelGGL(gmk_begin_kernel, dim3(t.B), dim3(kGmkThreads), 0, s, t, boards, start_index, state);
  return hipGetLastError();
}

hipError_t gmk_launch_step(const GmkTree &t, const GmkStepArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(gmk_step_kernel, dim3(t.B), dim3(kGmkThreads), 0, s, t, a);
  return hipGetLastError();
}

hipError_t gmk_launch_finish(const GmkTree &t, double temperature, int sample, uint32_t seed, const int64_t *counter,
                             int32_t *visits, double *probs, int32_t *action, hipStream_t s) {
  hipLaunchKernelGGL(gmk_finish_kernel, dim3(t.B), dim3(kGmkThreads), 0, s, t, temperature, sample, seed, counter,
                     visits, probs, action);
  return hipGetLastError();
}

hipError_t gmk_launch_export(const GmkTree &t, int32_t *visit, float *vsum, int32_t *first, float *prior,
                             int32_t *nnodes, hipStream_t s) {
  const size_t nodes = (size_t)t.B * t.cap;
  hipLaunchKernelGGL(gmk_export_kernel, dim3((unsigned)((nodes + 255) / 256)), dim3(256), 0, s, t, visit, vsum, first,
                     prior, nnodes);
  return hipGetLastError();
}

hipError_t gmk_launch_done_winner(const int32_t *boards, int n, int32_t *out, hipStream_t s) {
  hipLaunchKernelGGL(gmk_done_winner_kernel, dim3(n), dim3(kGmkThreads), 0, s, boards, n, out);
  return hipGetLastError();
}

template <int NRES, int P>
static hipError_t gmk_net_launch(const float *w, const float *state, int n, float *probs, float *value, hipStream_t s) {
  constexpr size_t lds = (size_t)GmkNet<P>::lds_bytes;
  // the attribute belongs to the (kernel, device) pair: set once per device ordinal (setting it twice is harmless)
  static std::atomic<bool> attr[64];
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= 64 || !attr[dev].load(std::memory_order_acquire)) {
    e = hipFuncSetAttribute((const void *)gomoku_net_eval_kernel<NRES, P>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 64) attr[dev].store(true, std::memory_order_release);
  }
  hipLaunchKernelGGL((gomoku_net_eval_kernel<NRES, P>), dim3((n + P - 1) / P), dim3(kGmkNetThreads), lds, s, w, state, n,
                     probs, value);
  return hipGetLastError();
}

template <int P>
static hipError_t gmk_net_launch_p(int nres, const float *w, const float *state, int n, float *probs, float *value,
                                   hipStream_t s) {
  return nres == 1 ? gmk_net_launch<1, P>(w, state, n, probs, value, s)
                   : gmk_net_launch<2, P>(w, state, n, probs, value, s);
}

hipError_t gmk_launch_net_eval(int nres, int positions, const float *w, const float *state, int n, float *probs,
                               float *value, hipStream_t s) {
  // measured: one position per workgroup up to 512 positions, two beyond
  if (positions == 0) positions = n < kGmkNetP2From ? 1 : 2;
  if (positions == 1) return gmk_net_launch_p<1>(nres, w, state, n, probs, value, s);
  return gmk_net_launch_p<2>(nres, w, state, n, probs, value, s);
}

}  // namespace lzm
