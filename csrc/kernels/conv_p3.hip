// fp32 convolutions on bf16 PLANES (the reference's precision, --compute_dtype fp32): every fp32
// GEMM operand is held in memory as three bf16 planes hi / mid / lo (x = hi + mid + lo exactly: 8 +
// 8 + 8 significant bits), written once by its PRODUCER (BN apply, BN backward, the plane-split
// kernel) where the split costs nothing -- those kernels are memory bound. The GEMMs then stage
// plain bf16 tiles: LDS-DMA (buffer_load ... lds) of 3 images per operand, no register staging, no
// VALU split, and six MFMA products per (A, B) fragment set (bf16x6: hi*hi + hi*mid + mid*hi +
// mid*mid + hi*lo + lo*hi, fp32 accumulation; the dropped mid*lo, lo*mid, lo*lo are ~2^-24).
//
// Roles (the reference's MKL-DNN fp32 Conv2D fwd / bwd-data / bwd-filter primitives, SURVEY.md
// §2.6, driven by /root/reference/benchmark-scripts/run-tf-sing-ucx-openmpi.sh:62-81):
//   * conv_igemm_p3_kernel  forward and data-gradient implicit GEMMs (fp32 output, fused BN
//                           statistics, beta-accumulate, split-K via splitk_gather)
//   * conv_p3_patch_kernel  the 3x3 / stride 1 forward and data gradient with the input patch
//                           resident in LDS (conv_p3_patch.h)
//   * conv_wgrad_p3_kernel  weight-gradient implicit GEMM (transposed fragment reads,
//                           ds_read_b64_tr_b16, split-K with fp32 atomics)
//
// Design for CDNA4: bf16x6 does 6 MFMAs per 3+3 fragment reads, twice the MFMA work per LDS byte
// of the bf16 GEMM, so these kernels can be MFMA bound -- the constraint is LDS CAPACITY (3 images
// per operand): a 128x64 block tile is 72 KB per k-step, so the ring is two stages (144 KB, one
// workgroup per CU). Each stage carries 6x the MFMA time of a bf16 k-step (1536 cycles per wave at
// 64x32 wave tiles), which covers the next stage's DMA latency, so double buffering is enough.
#include "conv_p3_fwd.h"
#include "conv_p3_patch.h"
#include "conv_p3_persist.h"
#include "conv_p3_wgrad.h"

namespace hcb {

// The rows of gemm_cfg.h HCB_P3_CFGS beyond the per-tile kernels: the persistent and
// weights-resident launchers return false for a problem they do not serve (an epilogue, a shape);
// the row's fallback then runs (a retired row's always), down to a per-tile cfg, which is returned.
// -1: launched.
#define HCB_CASE_TILE(...)
#define HCB_CASE_PERSIST(C, WM, WN, TM, TN, KW, NST, OCC, FB) \
  case C: return launch_p3p<WM, WN, TM, TN, KW, NST, OCC, false>(p, st) ? -1 : launch_p3_persist(p, FB, st);
#define HCB_CASE_BRES(C, WM, WN, TM, TN, KW, NST, OCC, FB) \
  case C: return launch_p3p<WM, WN, TM, TN, KW, NST, OCC, true>(p, st) ? -1 : launch_p3_persist(p, FB, st);
#define HCB_CASE_RETIRED(C, WM, WN, TM, TN, KW, NST, OCC, FB) \
  case C: return launch_p3_persist(p, FB, st);
static int launch_p3_persist(const ConvParams& p, int cfg, hipStream_t st) {
  switch (cfg) {
    HCB_P3_CFGS(HCB_CASE)
    default: return cfg;
  }
}
#undef HCB_CASE_TILE
#undef HCB_CASE_PERSIST
#undef HCB_CASE_BRES
#undef HCB_CASE_RETIRED

void launch_conv_p3(const ConvParams& p, int cfg, hipStream_t st) {
  if (p.inf) {  // the inference epilogue: per-tile kernels only (checked by the binding)
    launch_p3_cfg<false, true>(p, cfg, st);
    return;
  }
  if (p3_cfg_patch(cfg) && (cfg = launch_p3_patch_cfg(p, cfg, st)) < 0) return;
  if (cfg >= 0 && (cfg = launch_p3_persist(p, cfg, st)) < 0) return;
  if (p.bnb_acc != nullptr)
    launch_p3_cfg<true, false>(p, cfg, st);
  else
    launch_p3_cfg<false, false>(p, cfg, st);
}

// the rows of gemm_cfg.h HCB_WP3_CFGS; a cfg outside the table runs cfg 2
#define HCB_CASE_TILE(C, WM, WN, TM, TN, KW, NST, OCC) \
  case C: wlaunch_p3<WM, WN, TM, TN, NST, KW, OCC>(p, splits, st); break;
#define HCB_CASE_PERSIST(C, WM, WN, TM, TN, KW, NST, OCC) \
  case C: wlaunch_p3p<WM, WN, TM, TN, OCC>(p, splits, st); break;
void launch_wgrad_p3(const WgradParams& p, int cfg, int splits, hipStream_t st) {
  switch (cfg) {
    HCB_WP3_CFGS(HCB_CASE)
    default: launch_wgrad_p3(p, 2, splits, st); break;
  }
}
#undef HCB_CASE_TILE
#undef HCB_CASE_PERSIST

// ============================================================== plane split / merge
// x fp32 [rows][ldx] (C channels used) -> three bf16 planes [3][rows][ldo] (plane stride `plane`
// elements): hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid) (round to nearest even;
// hi + mid + lo == x for finite 2^-100 <= |x| <= 2^127 and for +0; -0 merges to +0, below
// 2^-110 the lo plane underflows bf16 (the merged value is within 2^-134), and where hi rounds to Inf the merged value is NaN:
// tests/test_loss_ref_cpu.py pins the domain)
__global__ __launch_bounds__(256) void split_planes_kernel(const float* __restrict__ x, int ldx, int C, int64_t n8,
                                                           uint16_t* __restrict__ out, int ldo, int64_t plane) {
  const int CV = C >> 3;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / CV;
    const int cv = (int)(i - row * CV);
    const u32x4* src = reinterpret_cast<const u32x4*>(x + row * ldx + cv * 8);
    u32x4 hi, mid, lo;
    split3_8(src[0], src[1], hi, mid, lo);
    uint16_t* o = out + row * ldo + cv * 8;
    *reinterpret_cast<u32x4*>(o) = hi;
    *reinterpret_cast<u32x4*>(o + plane) = mid;
    *reinterpret_cast<u32x4*>(o + 2 * plane) = lo;
  }
}

__global__ __launch_bounds__(256) void merge_planes_kernel(const uint16_t* __restrict__ in, int ldi, int64_t plane,
                                                           int C, int64_t n8, float* __restrict__ y, int ldy) {
  const int CV = C >> 3;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / CV;
    const int cv = (int)(i - row * CV);
    const uint16_t* s = in + row * ldi + cv * 8;
    float h[8], m[8], l[8];
    unpack_bf16x8(*reinterpret_cast<const u32x4*>(s), h);
    unpack_bf16x8(*reinterpret_cast<const u32x4*>(s + plane), m);
    unpack_bf16x8(*reinterpret_cast<const u32x4*>(s + 2 * plane), l);
    float* o = y + row * ldy + cv * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = h[e] + (m[e] + l[e]);
  }
}

// global average pool on planes (the ResNet head on the fp32 path): x planes [N][HW][C] -> the
// pooled features as planes [N][C] (the classifier GEMM's operand); fp32 sums of the exact values
__global__ __launch_bounds__(256) void gap_fwd_p3_kernel(const uint16_t* __restrict__ x, int64_t xps,
                                                         uint16_t* __restrict__ y, int64_t yps, int N, int HW, int C) {
  const int CV = C >> 3;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= N * CV) return;
  const int n = idx / CV, cv = idx % CV;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int i = 0; i < HW; ++i) {
    const uint16_t* s = x + ((size_t)n * HW + i) * C + cv * 8;
    float f[8];
    merge_p3(*reinterpret_cast<const u32x4*>(s), *reinterpret_cast<const u32x4*>(s + xps),
             *reinterpret_cast<const u32x4*>(s + 2 * xps), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += f[e];
  }
  const float inv = 1.f / (float)HW;
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] *= inv;
  store_p3(y + (size_t)n * C + cv * 8, yps, acc);
}

void launch_gap_fwd_p3(const uint16_t* x, int64_t xps, uint16_t* y, int64_t yps, int N, int HW, int C, hipStream_t st) {
  const int total = N * (C / 8);
  hipLaunchKernelGGL(gap_fwd_p3_kernel, dim3((total + 255) / 256), dim3(256), 0, st, x, xps, y, yps, N, HW, C);
}

static int p3_grid(int64_t n8) {
  int64_t b = (n8 + 255) / 256;
  return (int)(b < 4096 ? (b > 0 ? b : 1) : 4096);
}

void launch_split_planes(const float* x, int ldx, int64_t rows, int C, uint16_t* out, int ldo, int64_t plane,
                         hipStream_t st) {
  const int64_t n8 = rows * (C / 8);
  hipLaunchKernelGGL(split_planes_kernel, dim3(p3_grid(n8)), dim3(256), 0, st, x, ldx, C, n8, out, ldo, plane);
}

void launch_merge_planes(const uint16_t* in, int ldi, int64_t plane, int64_t rows, int C, float* y, int ldy,
                         hipStream_t st) {
  const int64_t n8 = rows * (C / 8);
  hipLaunchKernelGGL(merge_planes_kernel, dim3(p3_grid(n8)), dim3(256), 0, st, in, ldi, plane, C, n8, y, ldy);
}

}  // namespace hcb
