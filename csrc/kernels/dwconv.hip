// Depthwise 3x3 convolution for NHWC activations on gfx950 (MobileNet-v2's 17 depthwise layers):
// forward, data gradient and weight gradient. T = the build's 16-bit type (bf16 / fp16) or fp32; the
// fp32 path works on plain fp32 tensors (no MFMA operand is involved, so no planes). Arithmetic is
// fp32 FMA throughout.
//
// A depthwise conv has no reduction over channels, hence no GEMM and nothing for the matrix cores:
// it is a stencil that moves every byte once and does 9 FMAs per output element. The kernels are
// laid out like the BN passes (bn.hip): a thread owns one vector of 8 channels (16-byte accesses of
// 16-bit data, two for fp32), keeps the 72 fp32 weights of its channels in registers, and walks its
// share of the pixels; blocks tile (pixel split) x (channel group), so consecutive lanes read
// consecutive channel vectors of one pixel. Every load is a raw buffer load: a tap outside the image
// gets the out-of-range offset and reads zero, which is the padding halo (top / left pads are
// explicit, bottom / right come from the range check).
//
//   dwconv_strip_kernel   z[n,p,q,c] = sum_{r,s} x[n, p*S-pt+r, q*S-pl+s, c] * w[c,r,s]: each thread
//                         computes a strip of adjacent outputs (4; 2 on fp32) of one row, reusing the input
//                         columns the strip's windows share in registers (rows are re-read through
//                         L1 by the same thread's next strip row). Optionally the BN statistics
//                         sum(z - shift), sum((z - shift)^2) go into the R replicas by row block,
//                         as the conv GEMM epilogues leave them. With FLIP it is the stride-1 data
//                         gradient: the same stencil over dz with the kernel rotated by 180 degrees.
//   dwconv_dgrad_gather_kernel  the strided data gradient, gather form: a thread per dx pixel and
//                         channel vector, the taps whose source index is not a multiple of the
//                         stride are skipped (their loads are forced out of range). No atomics.
//   dwconv_wgrad_kernel   stage one of dw[c,r,s] = sum_{n,p,q} dz * x: every workgroup reduces its
//                         slab of pixels into 9 sums per channel (registers, then LDS across the
//                         threads of a channel vector, fixed order) and STORES them to the caller's
//                         workspace [blocks][9][C]; dwconv_wgrad_fold_kernel sums the partials in
//                         block order and stores dw. No atomics, no zeroed memory: bitwise
//                         reproducible in every mode.
#include "common.h"
#include "kernels.h"

namespace hcb {

namespace {

// outputs per strip: 4 on 16-bit data, 2 on fp32 (whose column vectors take twice the registers:
// 4-wide fp32 strips need all 256 VGPRs and leave one wave per SIMD)
template <typename T>
constexpr int dw_tq() {
  return sizeof(T) == 4 ? 2 : 4;
}

// channel vectors (of 8) per block: 8 when possible, else the whole (small) C, else the largest
// divisor <= 32 (the grouping of the BN kernels)
int dw_group_vecs(int CV) {
  if (CV % 8 == 0) return 8;
  if (CV <= 32) return CV;
  for (int d = 32; d > 1; --d)
    if (CV % d == 0) return d;
  return 1;
}

// (item splits) x (channel groups): ~2048 blocks in total, every thread at least one item
dim3 dw_grid(int64_t items, int C, int* cvb_out, int cap = 2048) {
  const int CV = C / 8;
  const int cvb = dw_group_vecs(CV);
  const int groups = CV / cvb;
  const int rows = 256 / cvb;
  int64_t need = (items + rows - 1) / rows;
  int64_t target = cap / groups;
  if (target < 1) target = 1;
  int64_t s = need < target ? need : target;
  if (s < 1) s = 1;
  *cvb_out = cvb;
  return dim3((unsigned)s, (unsigned)groups);
}

struct DwMap {
  int cv, r0, rows, c0, CB, cl;
  bool active;
};
__device__ __forceinline__ DwMap dwmap(int CVB) {
  DwMap g;
  g.CB = CVB * 8;
  g.c0 = blockIdx.y * g.CB;
  g.rows = 256 / CVB;
  g.r0 = threadIdx.x / CVB;
  g.cl = (threadIdx.x % CVB) * 8;
  g.cv = blockIdx.y * CVB + (threadIdx.x % CVB);
  g.active = g.r0 < g.rows;
  return g;
}

// the 72 weights of channel vector cv: w[c][3][3] fp32, 288 contiguous bytes per vector
__device__ __forceinline__ void load_weights(const float* __restrict__ w, int cv, float* wr) {
  const f32x4* p = reinterpret_cast<const f32x4*>(w + (size_t)cv * 72);
#pragma unroll
  for (int i = 0; i < 18; ++i) {
    const f32x4 v = p[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) wr[i * 4 + e] = v[e];
  }
}

__device__ __forceinline__ uint32_t dw_bytes(int64_t rows, int ld, int C, uint32_t esz) {
  return (uint32_t)((((size_t)rows - 1) * (size_t)ld + (size_t)C) * esz);  // < 2 GiB: checked on the host
}

template <typename T, int S, bool FLIP>
__global__ __launch_bounds__(256) void dwconv_strip_kernel(DwParams p) {
  constexpr uint32_t E = Act8<T>::ESZ;
  constexpr int DW_TQ = dw_tq<T>();
  constexpr int NC = (DW_TQ - 1) * S + 3;  // input columns under a strip
  extern __shared__ __attribute__((aligned(16))) float lds_f[];  // statistics: [2][rows][CB]
  const DwMap gm = dwmap(p.CVB);
  // FLIP (data gradient): the input is dz [N,P,Q], the output dx [N,H,W]
  const int IH = FLIP ? p.P : p.H, IW = FLIP ? p.Q : p.W, OH = FLIP ? p.H : p.P, OW = FLIP ? p.W : p.Q;
  const int ldi = FLIP ? p.ldz : p.ldx, ldo = FLIP ? p.ldx : p.ldz;
  const int pt = FLIP ? 2 - p.pt : p.pt, pl = FLIP ? 2 - p.pl : p.pl;
  const T* __restrict__ in = reinterpret_cast<const T*>(FLIP ? p.z : p.x);
  T* __restrict__ out = reinterpret_cast<T*>(const_cast<void*>(FLIP ? p.x : p.z));
  float s1[8] = {0}, s2[8] = {0};
  if (gm.active) {
    float wr[72], kshift[8];
    load_weights(p.w, gm.cv, wr);
#pragma unroll
    for (int e = 0; e < 8; ++e) kshift[e] = (p.stats != nullptr && p.shift != nullptr) ? p.shift[gm.cv * 8 + e] : 0.f;
    const __amdgpu_buffer_rsrc_t ir = make_rsrc(in, dw_bytes((int64_t)p.N * IH * IW, ldi, p.C, E));
    const int QS = (OW + DW_TQ - 1) / DW_TQ;
    const int nstrips = p.N * OH * QS;
    for (int st = blockIdx.x * gm.rows + gm.r0; st < nstrips; st += gridDim.x * gm.rows) {
      const int qs = st % QS, t = st / QS;
      const int pp = t % OH, n = t / OH;
      const int q0 = qs * DW_TQ;
      const int h0 = pp * S - pt, w0 = q0 * S - pl;
      float acc[DW_TQ][8];
#pragma unroll
      for (int j = 0; j < DW_TQ; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[j][e] = 0.f;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const int h = h0 + r;
        const bool hok = (unsigned)h < (unsigned)IH;
        Act8<T> col[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) {
          const int wc = w0 + j;
          const bool ok = hok && (unsigned)wc < (unsigned)IW;
          col[j].load(ir, ok ? (uint32_t)(((size_t)(n * IH + h) * IW + wc) * ldi + gm.cv * 8) * E : HCB_OOB);
        }
#pragma unroll
        for (int j = 0; j < NC; ++j) {
          float f[8];
          col[j].to_f(f);
#pragma unroll
          for (int tq = 0; tq < DW_TQ; ++tq) {
            const int s = j - tq * S;  // the tap of output tq that reads column j (compile time)
            if (s < 0 || s > 2) continue;
            const int k = FLIP ? (2 - r) * 3 + (2 - s) : r * 3 + s;
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[tq][e] = fmaf(f[e], wr[e * 9 + k], acc[tq][e]);
          }
        }
      }
#pragma unroll
      for (int tq = 0; tq < DW_TQ; ++tq) {
        const int q = q0 + tq;
        if (q >= OW) continue;
        T* dst = out + ((size_t)(n * OH + pp) * OW + q) * ldo + gm.cv * 8;
        if (p.stats != nullptr) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float d = acc[tq][e] - kshift[e];
            s1[e] += d;
            s2[e] += d * d;
          }
        }
        if (p.accumulate) {
          Act8<T> prev;
          prev.load(dst);
          float f[8];
          prev.to_f(f);
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[tq][e] += f[e];
        }
        Act8<T>::store(dst, acc[tq]);
      }
    }
  }
  if (p.stats == nullptr) return;  // (uniform)
  // block partial -> LDS rows -> column sums in row order -> one add per (replica, channel)
  if (gm.active) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      lds_f[gm.r0 * gm.CB + gm.cl + e] = s1[e];
      lds_f[gm.rows * gm.CB + gm.r0 * gm.CB + gm.cl + e] = s2[e];
    }
  }
  __syncthreads();
  float* dst = p.stats + (size_t)(blockIdx.x % p.R) * 2 * p.C;
  for (int i = threadIdx.x; i < gm.CB; i += 256) {
    float a = 0.f, b = 0.f;
    for (int r = 0; r < gm.rows; ++r) {
      a += lds_f[r * gm.CB + i];
      b += lds_f[gm.rows * gm.CB + r * gm.CB + i];
    }
    atomicAdd(dst + gm.c0 + i, a);
    atomicAdd(dst + p.C + gm.c0 + i, b);
  }
}

// strided data gradient, gather form: dx[n,h,w,c] = sum over the taps (r, s) with (h + pt - r) and
// (w + pl - s) multiples of the stride of dz[n, (h+pt-r)/S, (w+pl-s)/S, c] * w[c,r,s]
template <typename T, int S>
__global__ __launch_bounds__(256) void dwconv_dgrad_gather_kernel(DwParams p) {
  constexpr uint32_t E = Act8<T>::ESZ;
  const DwMap gm = dwmap(p.CVB);
  if (!gm.active) return;
  float wr[72];
  load_weights(p.w, gm.cv, wr);
  const T* __restrict__ dz = reinterpret_cast<const T*>(p.z);
  T* __restrict__ dx = reinterpret_cast<T*>(const_cast<void*>(p.x));
  const __amdgpu_buffer_rsrc_t zr = make_rsrc(dz, dw_bytes((int64_t)p.N * p.P * p.Q, p.ldz, p.C, E));
  const int M = p.N * p.H * p.W;
  for (int m = blockIdx.x * gm.rows + gm.r0; m < M; m += gridDim.x * gm.rows) {
    const int w = m % p.W, t = m / p.W;
    const int h = t % p.H, n = t / p.H;
    Act8<T> v[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int hs = h + p.pt - r;
      const int pp = hs / S;
      const bool hok = hs >= 0 && hs % S == 0 && pp < p.P;
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const int ws = w + p.pl - s;
        const int q = ws / S;
        const bool ok = hok && ws >= 0 && ws % S == 0 && q < p.Q;
        v[r * 3 + s].load(zr, ok ? (uint32_t)(((size_t)(n * p.P + pp) * p.Q + q) * p.ldz + gm.cv * 8) * E : HCB_OOB);
      }
    }
    float acc[8] = {0};
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      float f[8];
      v[k].to_f(f);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = fmaf(f[e], wr[e * 9 + k], acc[e]);
    }
    T* dst = dx + (size_t)m * p.ldx + gm.cv * 8;
    if (p.accumulate) {
      Act8<T> prev;
      prev.load(dst);
      float f[8];
      prev.to_f(f);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += f[e];
    }
    Act8<T>::store(dst, acc);
  }
}

// weight gradient, stage one: this workgroup's pixels -> ws[blockIdx.x][9][C]
template <typename T, int S>
__global__ __launch_bounds__(256) void dwconv_wgrad_kernel(DwParams p, float* __restrict__ ws) {
  constexpr uint32_t E = Act8<T>::ESZ;
  extern __shared__ __attribute__((aligned(16))) float lds_f[];  // [rows][CB]
  const DwMap gm = dwmap(p.CVB);
  float acc[9][8];
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[k][e] = 0.f;
  if (gm.active) {
    const T* __restrict__ x = reinterpret_cast<const T*>(p.x);
    const T* __restrict__ dz = reinterpret_cast<const T*>(p.z);
    const __amdgpu_buffer_rsrc_t xr = make_rsrc(x, dw_bytes((int64_t)p.N * p.H * p.W, p.ldx, p.C, E));
    const __amdgpu_buffer_rsrc_t zr = make_rsrc(dz, dw_bytes((int64_t)p.N * p.P * p.Q, p.ldz, p.C, E));
    const int M = p.N * p.P * p.Q;
    for (int m = blockIdx.x * gm.rows + gm.r0; m < M; m += gridDim.x * gm.rows) {
      const int q = m % p.Q, t = m / p.Q;
      const int pp = t % p.P, n = t / p.P;
      const int h0 = pp * S - p.pt, w0 = q * S - p.pl;
      Act8<T> g, v[9];
      g.load(zr, (uint32_t)((size_t)m * p.ldz + gm.cv * 8) * E);
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          const int h = h0 + r, w = w0 + s;
          const bool ok = (unsigned)h < (unsigned)p.H && (unsigned)w < (unsigned)p.W;
          v[r * 3 + s].load(xr, ok ? (uint32_t)(((size_t)(n * p.H + h) * p.W + w) * p.ldx + gm.cv * 8) * E : HCB_OOB);
        }
      float gf[8];
      g.to_f(gf);
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        float f[8];
        v[k].to_f(f);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[k][e] = fmaf(gf[e], f[e], acc[k][e]);
      }
    }
  }
  // per tap: the block's threads of one channel vector meet in LDS and are summed in row order
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    if (gm.active) {
#pragma unroll
      for (int e = 0; e < 8; ++e) lds_f[gm.r0 * gm.CB + gm.cl + e] = acc[k][e];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < gm.CB; i += 256) {
      float a = 0.f;
      for (int r = 0; r < gm.rows; ++r) a += lds_f[r * gm.CB + i];
      ws[((size_t)blockIdx.x * 9 + k) * p.C + gm.c0 + i] = a;
    }
    __syncthreads();
  }
}

// stage two: dw[c][k] = sum over blocks (in block order) of ws[b][k][c]; stores, never adds
__global__ __launch_bounds__(256) void dwconv_wgrad_fold_kernel(const float* __restrict__ ws, int nblk, int C,
                                                                float* __restrict__ dw) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 9 * C) return;
  const int k = i / C, c = i - k * C;
  float a = 0.f;
  for (int b = 0; b < nblk; ++b) a += ws[((size_t)b * 9 + k) * C + c];
  dw[c * 9 + k] = a;
}

}  // namespace

int dwconv_wgrad_blocks(int N, int P, int Q, int C) {
  int cvb;
  // one slab per ~4 pixels per thread at least, at most 512 / groups slabs: the fold reads
  // blocks * 9 * C floats, a small fraction of the activations the slabs cover
  const int64_t M = (int64_t)N * P * Q;
  return (int)dw_grid((M + 3) / 4, C, &cvb, 512).x;
}

void launch_dwconv_fwd(const DwParams& p0, hipStream_t st, bool f32) {
  DwParams p = p0;
  const int tq = f32 ? dw_tq<float>() : dw_tq<uint16_t>();
  const int QS = (p.Q + tq - 1) / tq;
  dim3 grid = dw_grid((int64_t)p.N * p.P * QS, p.C, &p.CVB);
  size_t lds = 0;
  if (p.stats != nullptr) {
    // deterministic mode: at most R row blocks, so each replica slot receives a single add
    if (deterministic() && (int)grid.x > p.R) grid.x = p.R;
    lds = (size_t)2 * (256 / p.CVB) * p.CVB * 8 * 4;
  }
  p.accumulate = 0;
  if (f32) {
    if (p.S == 1)
      hipLaunchKernelGGL((dwconv_strip_kernel<float, 1, false>), grid, dim3(256), lds, st, p);
    else
      hipLaunchKernelGGL((dwconv_strip_kernel<float, 2, false>), grid, dim3(256), lds, st, p);
  } else {
    if (p.S == 1)
      hipLaunchKernelGGL((dwconv_strip_kernel<uint16_t, 1, false>), grid, dim3(256), lds, st, p);
    else
      hipLaunchKernelGGL((dwconv_strip_kernel<uint16_t, 2, false>), grid, dim3(256), lds, st, p);
  }
}

void launch_dwconv_dgrad(const DwParams& p0, hipStream_t st, bool f32) {
  DwParams p = p0;
  p.stats = nullptr;
  p.shift = nullptr;
  if (p.S == 1) {
    const int tq = f32 ? dw_tq<float>() : dw_tq<uint16_t>();
    const int QS = (p.W + tq - 1) / tq;
    dim3 grid = dw_grid((int64_t)p.N * p.H * QS, p.C, &p.CVB);
    if (f32)
      hipLaunchKernelGGL((dwconv_strip_kernel<float, 1, true>), grid, dim3(256), 0, st, p);
    else
      hipLaunchKernelGGL((dwconv_strip_kernel<uint16_t, 1, true>), grid, dim3(256), 0, st, p);
    return;
  }
  dim3 grid = dw_grid((int64_t)p.N * p.H * p.W, p.C, &p.CVB);
  if (f32)
    hipLaunchKernelGGL((dwconv_dgrad_gather_kernel<float, 2>), grid, dim3(256), 0, st, p);
  else
    hipLaunchKernelGGL((dwconv_dgrad_gather_kernel<uint16_t, 2>), grid, dim3(256), 0, st, p);
}

void launch_dwconv_wgrad(const DwParams& p0, float* ws, int nblk, float* dw, hipStream_t st, bool f32) {
  DwParams p = p0;
  p.stats = nullptr;
  p.shift = nullptr;
  const int CV = p.C / 8;
  p.CVB = dw_group_vecs(CV);
  const dim3 grid((unsigned)nblk, (unsigned)(CV / p.CVB));
  const size_t lds = (size_t)(256 / p.CVB) * p.CVB * 8 * 4;
  if (f32) {
    if (p.S == 1)
      hipLaunchKernelGGL((dwconv_wgrad_kernel<float, 1>), grid, dim3(256), lds, st, p, ws);
    else
      hipLaunchKernelGGL((dwconv_wgrad_kernel<float, 2>), grid, dim3(256), lds, st, p, ws);
  } else {
    if (p.S == 1)
      hipLaunchKernelGGL((dwconv_wgrad_kernel<uint16_t, 1>), grid, dim3(256), lds, st, p, ws);
    else
      hipLaunchKernelGGL((dwconv_wgrad_kernel<uint16_t, 2>), grid, dim3(256), lds, st, p, ws);
  }
  hipLaunchKernelGGL(dwconv_wgrad_fold_kernel, dim3((9 * p.C + 255) / 256), dim3(256), 0, st, ws, nblk, p.C, dw);
}

}  // namespace hcb
