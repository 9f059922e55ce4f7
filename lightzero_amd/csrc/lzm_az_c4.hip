// lzm_az_c4.hip — the Connect4 AlphaZero kernels (lzm_az_c4.h, lzm_az_c4_net.h, lzm_az_c4_net_split.h) and their launchers. Argument
// checks, the workspace carve and the error text live with the C entry points in lzm_kernels.hip.
#include <hip/hip_runtime.h>

#include <atomic>

#include "lzm_az_c4.h"
#include "lzm_az_c4_net.h"
#define LZM_DEVICE_HELPERS_ONLY  // lzm_conv.h's split-scheme helpers without its kernels (lzm_kernels.hip's)
#include "lzm_az_c4_net_split.h"

namespace lzm {

static dim3 c4_groups(int n) {
  const int per = kC4Threads / kC4Group;
  return dim3((n + per - 1) / per);
}

hipError_t c4_launch_begin(const C4Tree &t, const int32_t *boards, const int32_t *start_index, float *state,
                           hipStream_t s) {
  hipLaunchKernelGGL(c4_begin_kernel, c4_groups(t.B), dim3(kC4Threads), 0, s, t, boards, start_index, state);
  return hipGetLastError();
}

hipError_t c4_launch_step(const C4Tree &t, const C4StepArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(c4_step_kernel, c4_groups(t.B), dim3(kC4Threads), 0, s, t, a);
  return hipGetLastError();
}

hipError_t c4_launch_finish(const C4Tree &t, double temperature, int sample, uint32_t seed, const int64_t *counter,
                            int32_t *visits, double *probs, int32_t *action, hipStream_t s) {
  hipLaunchKernelGGL(c4_finish_kernel, dim3((t.B + 127) / 128), dim3(128), 0, s, t, temperature, sample, seed,
                     counter, visits, probs, action);
  return hipGetLastError();
}

hipError_t c4_launch_export(const C4Tree &t, int32_t *visit, float *vsum, int32_t *first, float *prior,
                            int32_t *nnodes, hipStream_t s) {
  const size_t nodes = (size_t)t.B * t.cap;
  hipLaunchKernelGGL(c4_export_kernel, dim3((unsigned)((nodes + 255) / 256)), dim3(256), 0, s, t, visit, vsum, first,
                     prior, nnodes);
  return hipGetLastError();
}

hipError_t c4_launch_done_winner(const int32_t *boards, int n, int32_t *out, hipStream_t s) {
  hipLaunchKernelGGL(c4_done_winner_kernel, c4_groups(n), dim3(kC4Threads), 0, s, boards, n, out);
  return hipGetLastError();
}

template <int NRES>
static hipError_t c4_net_launch(const float *w, const float *state, int n, float *probs, float *value, hipStream_t s) {
  constexpr size_t lds = (size_t)kC4nLdsFloats * 4;
  // the attribute belongs to the (kernel, device) pair: set once per device ordinal (setting it twice is harmless)
  static std::atomic<bool> attr[64];
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= 64 || !attr[dev].load(std::memory_order_acquire)) {
    e = hipFuncSetAttribute((const void *)c4_net_eval_kernel<NRES>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 64) attr[dev].store(true, std::memory_order_release);
  }
  hipLaunchKernelGGL((c4_net_eval_kernel<NRES>), dim3((n + kC4nBoards - 1) / kC4nBoards), dim3(kC4nThreads), lds, s, w,
                     state, n, probs, value);
  return hipGetLastError();
}

hipError_t c4_launch_net_eval(int nres, const float *w, const float *state, int n, float *probs, float *value,
                              hipStream_t s) {
  return nres == 1 ? c4_net_launch<1>(w, state, n, probs, value, s) : c4_net_launch<2>(w, state, n, probs, value, s);
}

template <int NRES, int P>
static hipError_t c4_net_split_launch(const float *w, const float *state, int n, float *probs, float *value,
                                      int32_t *err, hipStream_t s) {
  constexpr size_t lds = (size_t)C4s<P>::lds_bytes;
  static std::atomic<bool> attr[64];  // per device ordinal, as c4_net_launch
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= 64 || !attr[dev].load(std::memory_order_acquire)) {
    e = hipFuncSetAttribute((const void *)c4_net_eval_split_kernel<NRES, P>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 64) attr[dev].store(true, std::memory_order_release);
  }
  hipLaunchKernelGGL((c4_net_eval_split_kernel<NRES, P>), dim3((n + P - 1) / P), dim3(kC4nThreads), lds, s, w, state, n,
                     probs, value, err);
  return hipGetLastError();
}

hipError_t c4_launch_net_split_eval(int nres, int boards, const float *w, const float *state, int n, float *probs,
                                    float *value, int32_t *err, hipStream_t s) {
  if (boards == 0) boards = kC4sBoards;
  if (boards == 2)
    return nres == 1 ? c4_net_split_launch<1, 2>(w, state, n, probs, value, err, s)
                     : c4_net_split_launch<2, 2>(w, state, n, probs, value, err, s);
  return nres == 1 ? c4_net_split_launch<1, 4>(w, state, n, probs, value, err, s)
                   : c4_net_split_launch<2, 4>(w, state, n, probs, value, err, s);
}

}  // namespace lzm
