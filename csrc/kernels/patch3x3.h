// The shared pieces of the patch-resident BN-ReLU 3x3 kernels (dense3x3*.hip, preact3x3*.hip, preact_block.hip).
//
// The family's layout, stated once. Every kernel is a 3x3 convolution (or its gradient) over a raw NHWC map whose
// BatchNorm + ReLU is applied in fp32 registers on the way into an LDS patch; the nine taps read that resident patch,
// so an input element crosses global -> LDS once.
//   LDS unit      the VPP 16-byte columns (8 channels each) of one pixel or weight row: 64 bytes = one 32-channel MFMA
//                 K chunk (32 bytes where only a 16-channel half exists). The columns are XOR-swizzled with bits 2..
//                 of the unit index (patch_off), so the 16 lanes of a fragment read -- 16 consecutive units, one
//                 column -- hit 16 distinct 16-byte bank groups.
//   patch store   bnrelu_store: fmaxf(x * sc + sh, 0.f) per element, halo pixels and channels past C SELECTED to zero
//                 (the conv pads the normalised map), then the MFMA operand: 16-bit, or on the fp32 path the bf16
//                 hi / mid / lo split into three planes patch_b bytes apart.
//   MFMA          v_mfma_f32_16x16x32 (bf16, or f16 in the HCB_F16 build); fp32: six bf16 products per fragment pair,
//                 small terms first, as conv_p3 orders them (mfma_acc). The order is numerically significant.
//   statistics    input: mean / invstd finalised in the kernel from the R replicas of the accumulator
//                 (bn_coef_from_acc, bn_apply_acc's arithmetic). Output: shifted sums of the fp32 accumulators, across
//                 lanes by shuffles, across waves through LDS in wave order, one atomic per channel and workgroup into
//                 replica blockIdx.x % R (stats_reduce).
//   weight grads  per (chunk, slab) partials in a caller-owned workspace, summed by wgrad_fold_kernel in a fixed order.
// Only helpers live here; the plans (strip rows, slabs, LDS budgets) are each kernel's measured policy and stay with it.
#pragma once
#include <cstdio>
#include <cstdlib>

#include "common.h"

namespace hcb {

// the LDS of a gfx950 workgroup: what launch_big_lds raises a kernel's dynamic limit to
constexpr size_t PATCH_LDS_LIMIT = 160 * 1024;

// byte offset of 16-byte column v of patch unit `unit` (VPP columns of 16 bytes)
template <int VPP = 4>
__device__ __forceinline__ uint32_t patch_off(int unit, int v) {
  return (uint32_t)unit * (16u * VPP) + (uint32_t)((v ^ ((unit >> 2) & (VPP - 1))) << 4);
}

// 8 K values of one fragment column: two transposed reads (ds_read_b64_tr_b16) of 4 pixels each
__device__ __forceinline__ u32x4 frag_tr16(const char* r0, const char* r1) {
  const short4v a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((short4v HCB_LDS*)r0);
  const short4v b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((short4v HCB_LDS*)r1);
  const short8 t = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  return __builtin_bit_cast(u32x4, t);
}

// BN coefficients of the p.C input channels from the replica sums (bn_coef_fwd's arithmetic) into coef = [2][Cr]
// scale, shift (zeros past C); M = pixels of the batch. Where `pub`, the block also publishes the saved moments and
// updates the moving statistics. The caller's barrier follows.
template <typename P>
__device__ __forceinline__ void bn_coef_from_acc(const P& p, float* coef, int Cr, int M, bool pub) {
  const float inv_n = 1.f / (float)M;
  for (int c = threadIdx.x; c < Cr; c += 256) {
    float sc = 0.f, sh = 0.f;
    if (c < p.C) {
      float su = 0.f, q = 0.f;
      for (int r = 0; r < p.R; ++r) {
        su += p.acc[(size_t)r * 2 * p.acc_C + c];
        q += p.acc[(size_t)r * 2 * p.acc_C + p.acc_C + c];
      }
      const float k = p.shift != nullptr ? p.shift[c] : 0.f;
      const float d = su * inv_n;
      const float mu = d + k;
      const float var = fmaxf(q * inv_n - d * d, 0.f);
      const float is = rsqrtf(var + p.eps);
      sc = p.gamma[c] * is;
      sh = p.beta[c] - mu * sc;
      if (pub) {
        if (p.saved_mean != nullptr) p.saved_mean[c] = mu;
        if (p.saved_invstd != nullptr) p.saved_invstd[c] = is;
        if (p.run_mean != nullptr) {
          const float unb = M > 1 ? var * (float)M / (float)(M - 1) : var;
          p.run_mean[c] = p.momentum * p.run_mean[c] + (1.f - p.momentum) * mu;
          p.run_var[c] = p.momentum * p.run_var[c] + (1.f - p.momentum) * unb;
        }
      }
    }
    coef[c] = sc;
    coef[Cr + c] = sh;
  }
}

// scale / shift of the 8 channels c .. c + 7 (c % 8 == 0) from the [2][Cr] table in LDS
__device__ __forceinline__ void bn_coef_load8(const float* coef, int Cr, int c, float* sc, float* sh) {
  const f32x4* cs = reinterpret_cast<const f32x4*>(coef + c);
  const f32x4* ch = reinterpret_cast<const f32x4*>(coef + Cr + c);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    sc[e] = cs[0][e];
    sc[4 + e] = cs[1][e];
    sh[e] = ch[0][e];
    sh[4 + e] = ch[1][e];
  }
}

// one prefetched vector -> the stored MFMA operand at pb + lds_off: BN + ReLU, !ok (halo, channel past C) selected
// to zero, then 16-bit, or (fp32) the hi / mid / lo planes at + 0, + patch_b, + 2 patch_b
template <typename T>
__device__ __forceinline__ void bnrelu_store(char* pb, uint32_t patch_b, uint32_t lds_off, const Act8<T>& xv, bool ok,
                                             const float* sc, const float* sh) {
  float f[8];
  xv.to_f(f);
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = ok ? fmaxf(f[e] * sc[e] + sh[e], 0.f) : 0.f;
  if constexpr (sizeof(T) == 4) {
    u32x4 a, bq, hi, mid, lo;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      a[e] = __float_as_uint(f[e]);
      bq[e] = __float_as_uint(f[4 + e]);
    }
    split3_8(a, bq, hi, mid, lo);
    *reinterpret_cast<u32x4*>(pb + lds_off) = hi;
    *reinterpret_cast<u32x4*>(pb + patch_b + lds_off) = mid;
    *reinterpret_cast<u32x4*>(pb + 2 * patch_b + lds_off) = lo;
  } else {
    *reinterpret_cast<u32x4*>(pb + lds_off) = pack8(f);
  }
}

// acc += a x bb: one 16-bit MFMA, or (F32: a, bb = hi / mid / lo planes) the six bf16 products, small terms first
template <bool F32>
__device__ __forceinline__ void mfma_acc(const u32x4* a, const u32x4* bb, f32x4& acc) {
  if constexpr (F32) {
    acc = mfma_bf16(a[2], bb[0], acc);
    acc = mfma_bf16(a[0], bb[2], acc);
    acc = mfma_bf16(a[1], bb[1], acc);
    acc = mfma_bf16(a[1], bb[0], acc);
    acc = mfma_bf16(a[0], bb[1], acc);
    acc = mfma_bf16(a[0], bb[0], acc);
  } else {
    acc = mfma16(__builtin_bit_cast(act16x8, a[0]), __builtin_bit_cast(act16x8, bb[0]), acc);
  }
}

// The output-statistics tail of a forward kernel whose 4 waves hold NCT column tiles (wave w: tile w % NCT). s1 / s2:
// the lane's sums of (y - K), (y - K)^2 of its 4 channels; lanes of one fq = lane >> 4 hold the same channels. Sums
// the 16 pixels by shuffles, then the waves of a column tile through red = [4 waves][2][16] in wave order, then ONE
// atomic add per channel into replica blockIdx.x % stats_R of stats = [R][2][stats_C], columns n0 .. n0 + 16 NCT
template <int NCT>
__device__ __forceinline__ void stats_reduce(float* s1, float* s2, float* red, float* stats, int stats_R, int stats_C,
                                             int n0, int wave, int frow, int fq) {
  constexpr int NPW = 4 / NCT;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      s1[e] += __shfl_xor(s1[e], o, 64);
      s2[e] += __shfl_xor(s2[e], o, 64);
    }
    if (frow == 0) {
      red[wave * 32 + fq * 4 + e] = s1[e];
      red[wave * 32 + 16 + fq * 4 + e] = s2[e];
    }
  }
  __syncthreads();
  const int tid = threadIdx.x;
  if (tid < 32 * NCT) {
    const int t = tid >> 5, j = tid & 31;  // column tile t (waves t, t + NCT, ...), sum j < 16, square sum j >= 16
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < NPW; ++k) a += red[(k * NCT + t) * 32 + j];
    float* dst = stats + (size_t)(blockIdx.x % stats_R) * 2 * stats_C + n0 + t * 16;
    atomicAdd(dst + (j < 16 ? j : stats_C + j - 16), a);
  }
}

#ifdef PATCH3X3_WGRAD_FOLD  // defined by the two weight-gradient files: a kernel in a header is emitted wherever it is seen
namespace {

// dw[n][tap * C + c] += sum over the slabs of ws[slab][n][tap][c], ws = [nslabs][ws_rows][9][C rounded up to 32]; rows
// n < live_rows only. A block folds 16 consecutive elements: thread (sl, el) sums slabs sl, sl + 16, ... of element el
// in slab order, then the 16 partial sums meet in LDS and are added in sl order -- a fixed order, whatever the
// device. (File-local, as every kernel of this library: one copy per weight-gradient file.)
__global__ __launch_bounds__(256) void wgrad_fold_kernel(const float* ws, float* dw, int C, int ldw, int nslabs,
                                                         int ws_rows, int live_rows) {
  __shared__ float part[16][17];
  const int el = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int idx = blockIdx.x * 16 + el;
  const int K = 9 * C;
  const bool ok = idx < live_rows * K;
  const int n = ok ? idx / K : 0, k = ok ? idx - n * K : 0;
  float s = 0.f;
  if (ok) {
    const int tap = k / C, c = k - tap * C;
    const int C32 = (C + 31) & ~31;
    const size_t stride = (size_t)ws_rows * 9 * C32;
    const float* src = ws + ((size_t)n * 9 + tap) * C32 + c;
    for (int b = sl; b < nslabs; b += 16) s += src[b * stride];
  }
  part[sl][el] = s;
  __syncthreads();
  if (sl != 0 || !ok) return;
  float t = part[0][el];
#pragma unroll
  for (int j = 1; j < 16; ++j) t += part[j][el];
  dw[(size_t)n * ldw + k] += t;
}

}  // namespace
#endif

// TF 'SAME' for a 3-wide window: output size and the leading pad
inline void same3(int size, int s, int* out, int* lead) {
  *out = (size + s - 1) / s;
  const int total = (*out - 1) * s + 3 - size;
  *lead = (total > 0 ? total : 0) / 2;
}

// Launch a 256-thread kernel with `lds` bytes of dynamic LDS. More than the default 64 KiB is raised on every launch
// (a host-side attribute of the current device's function, no stream work), so every device gets it and a failure
// is seen here
template <typename P>
inline void launch_big_lds(void (*kernel)(P), dim3 grid, size_t lds, hipStream_t st, const P& params, const char* name) {
  if (lds > 64 * 1024) {
    const hipError_t e =
        hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PATCH_LDS_LIMIT);
    if (e != hipSuccess) {
      fprintf(stderr, "hcb %s: cannot raise the dynamic LDS limit: %s\n", name, hipGetErrorString(e));
      abort();
    }
  }
  hipLaunchKernelGGL(kernel, grid, dim3(256), lds, st, params);
}

}  // namespace hcb
