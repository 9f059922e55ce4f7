// lzm_az_gomoku_n.hip — the Gomoku 9 x 9 / 15 x 15 AlphaZero kernels (lzm_az_gomoku_n.h, lzm_az_gomoku_n_net.h)
// and their launchers. Argument checks, the workspace carve and the error text live with the C entry points in
// lzm_kernels.hip.
#include <hip/hip_runtime.h>

#include <atomic>

#include "lzm_az_gomoku_n.h"
#include "lzm_az_gomoku_n_net.h"

namespace lzm {

hipError_t gmkn_launch_begin(int n_board, const GmkNTree &t, const int32_t *boards, const int32_t *start_index,
                             float *state, hipStream_t s) {
  if (n_board == 9)
    hipLaunchKernelGGL(gmkn_begin_kernel<9>, dim3(t.B), dim3(kGmkNThreads), 0, s, t, boards, start_index, state);
  else
    hipLaunchKernelGGL(gmkn_begin_kernel<15>, dim3(t.B), dim3(kGmkNThreads), 0, s, t, boards, start_index, state);
  return hipGetLastError();
}

hipError_t gmkn_launch_step(int n_board, const GmkNTree &t, const GmkNStepArgs &a, hipStream_t s) {
  if (n_board == 9)
    hipLaunchKernelGGL(gmkn_step_kernel<9>, dim3(t.B), dim3(kGmkNThreads), 0, s, t, a);
  else
    hipLaunchKernelGGL(gmkn_step_kernel<15>, dim3(t.B), dim3(kGmkNThreads), 0, s, t, a);
  return hipGetLastError();
}

hipError_t gmkn_launch_finish(int n_board, const GmkNTree &t, double temperature, int sample, uint32_t seed,
                              const int64_t *counter, int32_t *visits, double *probs, int32_t *action, hipStream_t s) {
  if (n_board == 9)
    hipLaunchKernelGGL(gmkn_finish_kernel<9>, dim3(t.B), dim3(kGmkNThreads), 0, s, t, temperature, sample, seed,
                       counter, visits, probs, action);
  else
    hipLaunchKernelGGL(gmkn_finish_kernel<15>, dim3(t.B), dim3(kGmkNThreads), 0, s, t, temperature, sample, seed,
                       counter, visits, probs, action);
  return hipGetLastError();
}

hipError_t gmkn_launch_export(const GmkNTree &t, int32_t *visit, float *vsum, int32_t *first, float *prior,
                              int32_t *nnodes, hipStream_t s) {
  const size_t nodes = (size_t)t.B * t.cap;
  hipLaunchKernelGGL(gmkn_export_kernel, dim3((unsigned)((nodes + 255) / 256)), dim3(256), 0, s, t, visit, vsum, first,
                     prior, nnodes);
  return hipGetLastError();
}

hipError_t gmkn_launch_done_winner(int n_board, const int32_t *boards, int n, int32_t *out, hipStream_t s) {
  if (n_board == 9)
    hipLaunchKernelGGL(gmkn_done_winner_kernel<9>, dim3(n), dim3(kGmkNThreads), 0, s, boards, n, out);
  else
    hipLaunchKernelGGL(gmkn_done_winner_kernel<15>, dim3(n), dim3(kGmkNThreads), 0, s, boards, n, out);
  return hipGetLastError();
}

template <int NRES, int N, int P>
static hipError_t gmkn_net_launch(const float *w, const float *state, int n, float *probs, float *value,
                                  hipStream_t s) {
  constexpr size_t lds = (size_t)GmkNNet<N, P>::lds_bytes;
  // the attribute belongs to the (kernel, device) pair: set once per device ordinal (setting it twice is harmless)
  static std::atomic<bool> attr[64];
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= 64 || !attr[dev].load(std::memory_order_acquire)) {
    e = hipFuncSetAttribute((const void *)gomoku_n_net_eval_kernel<NRES, N, P>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 64) attr[dev].store(true, std::memory_order_release);
  }
  hipLaunchKernelGGL((gomoku_n_net_eval_kernel<NRES, N, P>), dim3((n + P - 1) / P), dim3(kGmkNNetThreads), lds, s, w,
                     state, n, probs, value);
  return hipGetLastError();
}

template <int N, int P>
static hipError_t gmkn_net_launch_p(int nres, const float *w, const float *state, int n, float *probs, float *value,
                                    hipStream_t s) {
  return nres == 1 ? gmkn_net_launch<1, N, P>(w, state, n, probs, value, s)
                   : gmkn_net_launch<2, N, P>(w, state, n, probs, value, s);
}

hipError_t gmkn_launch_net_eval(int n_board, int nres, const float *w, const float *state, int n, float *probs,
                                float *value, hipStream_t s) {
  return n_board == 9 ? gmkn_net_launch_p<9, 1>(nres, w, state, n, probs, value, s)
                      : gmkn_net_launch_p<15, 1>(nres, w, state, n, probs, value, s);
}

}  // namespace lzm
