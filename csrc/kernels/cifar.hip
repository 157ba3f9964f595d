// CIFAR-10 batch assembly on the GPU: the whole split lives in device memory as the python
// pickles store it (uint8 [N][3][32][32], planar: 1,024 R, 1,024 G, 1,024 B bytes per image), and one
// launch per batch gathers, pads, crops, flips and normalises B images and gathers their labels.
// The host sends only desc [B][4] int32 = (index, oy, ox, flip) per image:
//   x' = flip ? 31 - x : x,  r = y + oy - 4,  c = x' + ox - 4
//   out[b, y, x, ch] = (0 <= r, c < 32 ? data[index, ch, r, c] : 0) * (1 / 127.5) - 1   for ch < 3
// -- tf_cnn_benchmarks' zero pad to 40 x 40, random 32 x 32 crop (offsets 0..8), random flip, then
// this engine's x / 127.5 - 1 (a padded pixel is -1.0); oy = ox = 4, flip = 0 is the evaluation
// preprocessing. Channels 3..Cpad-1 are zero. index == -1 is a padding row of a short last batch: an
// all-zero image with label -1 (eval_metrics skips it).
//
// One thread per output pixel, one 16-byte store per 8 channels (16-bit) / per 4 (fp32). A wave's 64
// lanes read two 32-byte row segments of each byte plane (reversed under a flip): coalesced byte
// loads. ~0.4 MB moved per 128-image batch: the launch, not the kernel, is the cost.
#include "common.h"
#include "kernels.h"

namespace hcb {

template <bool F32>
__global__ __launch_bounds__(256) void cifar_batch_kernel(const uint8_t* __restrict__ data,
                                                          const int64_t* __restrict__ labels_all,
                                                          const int* __restrict__ desc, void* __restrict__ out,
                                                          int64_t* __restrict__ labels_out, int Cpad) {
  const int img = blockIdx.y;
  const int pix = blockIdx.x * 256 + threadIdx.x;  // grid.x * 256 == 1024: every thread owns a pixel
  const int idx = desc[img * 4 + 0];
  const int oy = desc[img * 4 + 1], ox = desc[img * 4 + 2], flip = desc[img * 4 + 3];
  if (pix == 0) labels_out[img] = idx < 0 ? (int64_t)-1 : labels_all[idx];
  float v[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) v[c] = 0.f;
  if (idx >= 0) {
    const int y = pix >> 5, x = pix & 31;
    const int r = y + oy - 4, c = (flip ? 31 - x : x) + ox - 4;
    const bool in = (unsigned)r < 32u && (unsigned)c < 32u;
    const uint8_t* p = data + (size_t)idx * 3072 + (in ? r * 32 + c : 0);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float raw = in ? (float)p[ch * 1024] : 0.f;
      v[ch] = raw * (1.0f / 127.5f) - 1.0f;
    }
  }
  const size_t base = ((size_t)img * 1024 + pix) * Cpad;
  if constexpr (F32) {
    float* o = reinterpret_cast<float*>(out) + base;
    *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], 0.f);
    for (int c = 4; c < Cpad; c += 4) *reinterpret_cast<float4*>(o + c) = make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    uint16_t* o = reinterpret_cast<uint16_t*>(out) + base;
    *reinterpret_cast<u32x4*>(o) = pack8(v);
    for (int c = 8; c < Cpad; c += 8) *reinterpret_cast<u32x4*>(o + c) = u32x4{0u, 0u, 0u, 0u};
  }
}

void launch_cifar_batch(const uint8_t* data, const int64_t* labels_all, const int* desc, int B, void* out,
                        int64_t* labels_out, int Cpad, bool f32, hipStream_t st) {
  dim3 grid(4, B);
  if (f32)
    hipLaunchKernelGGL(cifar_batch_kernel<true>, grid, dim3(256), 0, st, data, labels_all, desc, out, labels_out, Cpad);
  else
    hipLaunchKernelGGL(cifar_batch_kernel<false>, grid, dim3(256), 0, st, data, labels_all, desc, out, labels_out,
                       Cpad);
}

}  // namespace hcb
