// The CIFAR ResNet "plan A" shortcut (tf_cnn_benchmarks ResnetCifar10Model: apool(1, 1, s, s) 'VALID'
// then tf.pad on the channel axis): a spatial subsample plus a centred zero pad of the channels,
//   y[n, p, q, k] = x[n, p*s, q*s, k - pad]   for pad <= k < pad + C, else 0      (pad = (K - C) / 2)
// and its gradient
//   dx[n, h, w, c] = g[n, h/s, w/s, pad + c]  where h % s == 0 and w % s == 0, else 0.
// Both are pure copies in units of 16 bytes (C and pad are multiples of 8 elements), so one pair of
// kernels serves every activation format: 16-bit, fp32, and the fp32 path's bf16 planes -- subsampling
// and zero padding commute with the hi / mid / lo split, the three planes are 3N images of one launch.
// One thread per OUTPUT vector: every element of y / dx is written by the kernel itself (no memset
// node in the captured step, no reliance on zeroed memory), each by exactly one thread.
#include "common.h"
#include "kernels.h"

namespace hcb {

__global__ __launch_bounds__(256) void shortcut_pad_fwd_kernel(const u32x4* __restrict__ x, u32x4* __restrict__ y,
                                                               int64_t total, int H, int W, int P, int Q, int s,
                                                               int Cv, int Kv, int padv) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int kv = (int)(i % Kv);
  int64_t t = i / Kv;
  const int q = (int)(t % Q);
  t /= Q;
  const int p = (int)(t % P);
  const int64_t n = t / P;
  const int c = kv - padv;
  u32x4 v = u32x4{0u, 0u, 0u, 0u};
  if ((unsigned)c < (unsigned)Cv) v = x[((n * H + (int64_t)p * s) * W + (int64_t)q * s) * Cv + c];
  y[i] = v;
}

__global__ __launch_bounds__(256) void shortcut_pad_bwd_kernel(const u32x4* __restrict__ g, u32x4* __restrict__ dx,
                                                               int64_t total, int H, int W, int P, int Q, int s,
                                                               int Cv, int Kv, int padv) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int cv = (int)(i % Cv);
  int64_t t = i / Cv;
  const int w = (int)(t % W);
  t /= W;
  const int h = (int)(t % H);
  const int64_t n = t / H;
  u32x4 v = u32x4{0u, 0u, 0u, 0u};
  if (h % s == 0 && w % s == 0) v = g[((n * P + h / s) * Q + w / s) * Kv + padv + cv];
  dx[i] = v;
}

// x [NI][H][W][Cv] -> y [NI][P][Q][Kv] in 16-byte vectors (NI = images, x 3 for planes); the caller
// checked P == ceil(H / s), Q == ceil(W / s), Kv == Cv + 2 * padv
void launch_shortcut_pad_fwd(const void* x, void* y, int64_t NI, int H, int W, int P, int Q, int s, int Cv, int Kv,
                             int padv, hipStream_t st) {
  const int64_t total = NI * P * Q * Kv;
  if (total == 0) return;
  hipLaunchKernelGGL(shortcut_pad_fwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                     reinterpret_cast<const u32x4*>(x), reinterpret_cast<u32x4*>(y), total, H, W, P, Q, s, Cv, Kv, padv);
}

void launch_shortcut_pad_bwd(const void* g, void* dx, int64_t NI, int H, int W, int P, int Q, int s, int Cv, int Kv,
                             int padv, hipStream_t st) {
  const int64_t total = NI * H * W * Cv;
  if (total == 0) return;
  hipLaunchKernelGGL(shortcut_pad_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                     reinterpret_cast<const u32x4*>(g), reinterpret_cast<u32x4*>(dx), total, H, W, P, Q, s, Cv, Kv, padv);
}

}  // namespace hcb
