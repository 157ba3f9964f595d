// Local response normalisation over the channel axis of NHWC activations on gfx950 (tf.nn.lrn, the
// `cnn.lrn` of tf_cnn_benchmarks' CIFAR-10 AlexNet), forward and backward:
//   s[m, d]  = bias + alpha * sum_{j = max(0, d-r) .. min(C-1, d+r)} x[m, j]^2     (alpha is NOT divided by
//   y        = x * s^(-beta)                                                        the window size)
//   dx[m, j] = dy[j] * s[j]^(-beta) - 2 alpha beta x[j] * sum_{d in window(j)} dy[d] x[d] s[d]^(-beta-1)
// The backward recomputes s from x: no scale tensor is saved.
//
// There is no reduction a matrix core could take: every byte moves once and each element costs 2r+1
// adds and one power. A thread owns 8 consecutive channels of one pixel (one 16-byte access of 16-bit
// data, two of fp32, three of bf16 planes). With r <= 4 every tap outside a thread's own 8 channels
// lives in the lane to its left or right, so the halo is a cross-lane exchange, never a second load:
// the forward exchanges the squares (8 shuffles), the backward the squares and then
// t = dy * x * s^(-beta-1) (s at +-4 needs x at +-8, still one lane each side).
//
// Lane map: the C/8 lanes of a pixel are consecutive lanes of ONE wave; a wave holds floor(64 / (C/8))
// whole pixels and its remaining lanes idle (C = 72: 7 pixels of 9 lanes, one idle lane), so a pixel
// never straddles a wave and C <= 512. A lane at a pixel's edge (and every idle lane) SELECTS zeros
// instead of what the shuffle returned, so nothing crosses from a neighbouring pixel -- not even a NaN.
// All 64 lanes execute the shuffles; idle lanes neither load nor store.
//
// Formats (F): 0 = the build's 16-bit type, 1 = plain fp32, 2 = bf16 hi / mid / lo planes (x = hi + mid
// + lo summed in fp32, exact; written with the split of the BN apply kernels). Arithmetic is fp32.
// One launch each, no atomics, no zeroed memory: every output element is written by exactly one thread.
#include "common.h"
#include "kernels.h"

namespace hcb {

namespace {

template <int F>
__device__ __forceinline__ void lrn_load8(const void* base, int64_t plane, size_t off, float* f) {
  if constexpr (F == 0) {
    Act8<uint16_t> v;
    v.load(reinterpret_cast<const uint16_t*>(base) + off);
    v.to_f(f);
  } else if constexpr (F == 1) {
    Act8<float> v;
    v.load(reinterpret_cast<const float*>(base) + off);
    v.to_f(f);
  } else {
    const uint16_t* p = reinterpret_cast<const uint16_t*>(base) + off;
    const u32x4 h = *reinterpret_cast<const u32x4*>(p);
    const u32x4 m = *reinterpret_cast<const u32x4*>(p + plane);
    const u32x4 l = *reinterpret_cast<const u32x4*>(p + 2 * plane);
    merge_p3(h, m, l, f);
  }
}

template <int F>
__device__ __forceinline__ void lrn_store8(void* base, int64_t plane, size_t off, const float* f) {
  if constexpr (F == 0)
    Act8<uint16_t>::store(reinterpret_cast<uint16_t*>(base) + off, f);
  else if constexpr (F == 1)
    Act8<float>::store(reinterpret_cast<float*>(base) + off, f);
  else
    store_p3(reinterpret_cast<uint16_t*>(base) + off, plane, f);
}

// where this thread works: pixel `pix`, channel vector `cv` of CV; all 64 lanes of a wave get a map
struct LrnMap {
  size_t off;  // element offset of the thread's 8 channels
  bool active, first, last;
};
__device__ __forceinline__ LrnMap lrn_map(const LrnParams& p) {
  const int CV = p.C >> 3;
  const int ppw = 64 / CV;  // whole pixels per wave
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int pl = lane / CV, cv = lane - pl * CV;
  const int64_t pix = wave * ppw + pl;
  LrnMap m;
  m.active = pl < ppw && pix < p.M;
  m.first = cv == 0;
  m.last = cv == CV - 1;
  m.off = m.active ? (size_t)pix * (size_t)p.C + (size_t)cv * 8 : 0;
  return m;
}

// a[0..3] = channels -4..-1 (the left lane's last four), a[4..11] = v, a[12..15] = channels 8..11 (the
// right lane's first four); zeros past the pixel's edges. Every lane of the wave must call this.
__device__ __forceinline__ void lrn_halo(const float* v, const LrnMap& m, float* a) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float l = __shfl_up(v[4 + i], 1, 64);
    const float r = __shfl_down(v[i], 1, 64);
    a[i] = m.first ? 0.f : l;
    a[12 + i] = m.last ? 0.f : r;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) a[4 + e] = v[e];
}

template <int R>
__device__ __forceinline__ void lrn_window_r(const float* a, float* w) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float acc = a[e + 4 - R];
#pragma unroll
    for (int j = -R + 1; j <= R; ++j) acc += a[e + 4 + j];
    w[e] = acc;
  }
}
// w[e] = sum_{|j| <= r} a[e + 4 + j], left to right (r is uniform: one branch per wave)
__device__ __forceinline__ void lrn_window(const float* a, int r, float* w) {
  switch (r) {
    case 1: lrn_window_r<1>(a, w); break;
    case 2: lrn_window_r<2>(a, w); break;
    case 3: lrn_window_r<3>(a, w); break;
    default: lrn_window_r<4>(a, w); break;
  }
}

// s^(-beta) and s^(-beta-1) for s >= bias > 0. pmode 1: beta == 0.75, 2: beta == 0.5 (rsqrt / sqrt
// forms, ~1 ulp per step); 0: exp2(-beta * log2 s) on the hardware transcendentals
__device__ __forceinline__ void lrn_pow(float s, float beta, int pmode, float& pb, float& pb1) {
  if (pmode == 1) {
    const float q = __builtin_amdgcn_rsqf(s);  // s^-0.5
    pb = q * __builtin_amdgcn_sqrtf(q);
    pb1 = pb * (q * q);
  } else if (pmode == 2) {
    const float q = __builtin_amdgcn_rsqf(s);
    pb = q;
    pb1 = q * (q * q);
  } else {
    const float l = __builtin_amdgcn_logf(s);
    pb = __builtin_amdgcn_exp2f(-beta * l);
    pb1 = __builtin_amdgcn_exp2f(-(beta + 1.f) * l);
  }
}

template <int XF, int YF>
__global__ __launch_bounds__(256) void lrn_fwd_kernel(LrnParams p) {
  const LrnMap m = lrn_map(p);
  float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (m.active) lrn_load8<XF>(p.x, p.x_plane, m.off, x);
  float sq[8], a[16], w[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) sq[e] = x[e] * x[e];
  lrn_halo(sq, m, a);
  if (!m.active) return;
  lrn_window(a, p.r, w);
  float y[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float pb, pb1;
    lrn_pow(fmaf(p.alpha, w[e], p.bias), p.beta, p.pmode, pb, pb1);
    y[e] = x[e] * pb;
  }
  lrn_store8<YF>(p.out, p.out_plane, m.off, y);
}

template <int XF, int GF>
__global__ __launch_bounds__(256) void lrn_bwd_kernel(LrnParams p) {
  const LrnMap m = lrn_map(p);
  float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (m.active) {
    lrn_load8<XF>(p.x, p.x_plane, m.off, x);
    lrn_load8<GF>(p.dy, 0, m.off, g);
  }
  float sq[8], a[16], w[8], pb[8], t[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) sq[e] = x[e] * x[e];
  lrn_halo(sq, m, a);
  lrn_window(a, p.r, w);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float pb1;
    lrn_pow(fmaf(p.alpha, w[e], p.bias), p.beta, p.pmode, pb[e], pb1);
    t[e] = g[e] * x[e] * pb1;  // (an idle lane: s = bias, t = 0)
  }
  lrn_halo(t, m, a);
  if (!m.active) return;
  lrn_window(a, p.r, w);
  const float k = -2.f * p.alpha * p.beta;
  float dx[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) dx[e] = fmaf(k * x[e], w[e], g[e] * pb[e]);
  lrn_store8<GF>(p.out, 0, m.off, dx);
}

// blocks of 4 waves, floor(64 / (C/8)) pixels per wave; the host checked the count fits a grid
dim3 lrn_grid(const LrnParams& p) {
  const int ppw = 64 / (p.C / 8);
  const int64_t waves = (p.M + ppw - 1) / ppw;
  return dim3((unsigned)((waves + 3) / 4));
}

}  // namespace

int64_t lrn_blocks(int64_t M, int C) {
  const int ppw = 64 / (C / 8);
  return ((M + ppw - 1) / ppw + 3) / 4;
}

void launch_lrn_fwd(const LrnParams& p, int xf, int yf, hipStream_t st) {
  const dim3 grid = lrn_grid(p);
#define HCB_LRN_FWD(XF, YF) hipLaunchKernelGGL((lrn_fwd_kernel<XF, YF>), grid, dim3(256), 0, st, p)
  if (xf == 0)
    HCB_LRN_FWD(0, 0);
  else if (xf == 1 && yf == 1)
    HCB_LRN_FWD(1, 1);
  else if (xf == 1)
    HCB_LRN_FWD(1, 2);
  else if (yf == 1)
    HCB_LRN_FWD(2, 1);
  else
    HCB_LRN_FWD(2, 2);
#undef HCB_LRN_FWD
}

void launch_lrn_bwd(const LrnParams& p, int xf, hipStream_t st) {
  const dim3 grid = lrn_grid(p);
  if (xf == 0)
    hipLaunchKernelGGL((lrn_bwd_kernel<0, 0>), grid, dim3(256), 0, st, p);
  else if (xf == 1)
    hipLaunchKernelGGL((lrn_bwd_kernel<1, 1>), grid, dim3(256), 0, st, p);
  else
    hipLaunchKernelGGL((lrn_bwd_kernel<2, 1>), grid, dim3(256), 0, st, p);
}

}  // namespace hcb
