// DenseNet dense layer on gfx950: BatchNorm (batch statistics) -> ReLU -> conv 3x3 / stride 1 / SAME with
// at most 16 output channels, in ONE pass over the raw concat buffer:
//   y[:, slot] = conv3x3( relu( gamma * (x - mean) * invstd + beta ) ),   x = channels [0, C) of the buffer
// The normalised operand is never written to memory. A growth-rate-12 layer is a GEMM of 16 output
// columns (12 padded to 16): it is bound by reading its input, and the unfused chain (BN apply writes
// the operand, the GEMM reads it back, nine taps through L2) moves that input three times.
//
// The LDS unit and swizzle, the BN + ReLU patch store, the MFMA order, the coefficients from the replica sums
// and the output-statistics reduction are the family's: patch3x3.h states them once.
//
// Work split (not a row of gemm_cfg.h): a workgroup of 4 waves owns a strip of TR whole output rows
// of one image (TR * W <= 128 pixels = 8 MFMA tiles of 16 pixels, two per wave) and all 16 output
// channels. It walks C in chunks of 32 channels, one MFMA K:
//   global -> registers   the chunk's input patch, (TR + 2) x (W + 2) pixels x 32 channels, 16-byte raw
//                         buffer loads; pixels outside the image and channels past C get the
//                         out-of-range offset. The chunk's weights, 9 taps x 16 rows x 32 channels of
//                         the [Nout][Kpad] pack (rows past Nout out of range: zeros), come the same way.
//   registers -> LDS      bnrelu_store (halo pixels are SELECTED to zero: the conv pads the normalised map).
//   LDS -> MFMA           A = the tap's weight rows, B = 16 pixels, so a lane ends with 4 consecutive output
//                         channels of one pixel (an 8- or 16-byte store). The nine taps read the resident
//                         patch: an input element crosses global -> LDS once per layer.
// Both LDS buffers (patch + weights) are doubled: the loads of chunk c + 1 are issued before the MFMAs
// of chunk c and transformed and stored after them; one barrier per chunk. LDS-DMA is not usable here,
// the data is transformed on its way.
//
// This is preact3x3.hip's kernel at one column tile and stride 1, plus three things a slot of Nout <= 16 channels
// needs: weight rows past Nout are read out of range, output channels Nout..15 are stored as literal zeros, whatever
// the operands hold (an Inf or NaN input cannot reach them; their statistics stay zero), and stats_shift is read
// only below Nout. Running it AS that kernel (stride and patch width as run-time parameters) was measured 1.1 - 3.7 %
// slower on every layer shape (profiles/patch3x3_refactor.txt), so the two stay separate kernels over one set of
// helpers; per output pixel both sum K in the same order, and y is bitwise equal between them.
//
// Block 0 publishes mean / invstd and updates the moving statistics. Deterministic mode caps the grid at R blocks
// (the kernel strides over the strips), so every replica slot of the output statistics gets one add.
//
// Resources (hipcc -O3, gfx950; no scratch in either build or form):
//   16-bit: 159 VGPRs (bf16 and fp16 builds), dynamic LDS = 8 * C32 + 512 + 2 * (patch_pix + 144) * 64 bytes
//   fp32:   213 VGPRs, dynamic LDS = 8 * C32 + 512 + 6 * (patch_pix + 144) * 64 bytes (three tiles of each)
// with C32 = C rounded up to 32 and patch_pix = (TR + 2) * (W + 2) <= 320. TR = min(128 / W, 16, H), on maps
// of at most 256 pixels 64 / W, of at most 64 pixels H / 2 (more workgroups: measured, profiles/densenet.txt);
// the launcher lowers it until 160 KiB hold the fp32 form (32 x 32 maps, C = 208: TR = 4, 46 KiB / 133 KiB).
// The registers go to the prefetched chunk (5 patch + 3 weight vectors per thread, twice that and three
// planes of weights on fp32) and to the 27 precomputed LDS addresses.
#include <cstdio>
#include <cstdlib>

#include "common.h"
#include "kernels.h"
#include "patch3x3.h"

namespace hcb {

namespace {

constexpr int DN_MAXIT = 5;   // patch vectors (8 channels of one pixel) per thread and chunk: patch_pix * 4 <= 5 * 256
constexpr int DN_WIT = 3;     // weight vectors per thread and chunk: 9 * 16 * 4 = 576 <= 3 * 256
constexpr int DN_TILES = 2;   // 16-pixel MFMA tiles per wave
constexpr int DN_WUNITS = 9 * 16;
constexpr uint32_t DN_WBYTES = DN_WUNITS * 64u;
constexpr size_t DN_LDS_MAX = 160 * 1024;

size_t dn_lds_bytes(int C, int patch_pix, bool f32) {
  const int Cr = (C + 31) & ~31;
  return (size_t)(2 * Cr + 128) * 4 + 2 * (size_t)(f32 ? 3 : 1) * ((size_t)patch_pix * 64 + DN_WBYTES);
}

template <typename T>
__global__ __launch_bounds__(256) void dense_conv3x3_kernel(DenseParams p) {
  constexpr bool F32 = sizeof(T) == 4;
  constexpr int NPL = F32 ? 3 : 1;
  constexpr uint32_t E = Act8<T>::ESZ;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id_uniform();
  const int frow = lane & 15, fq = lane >> 4;
  const int Cr = (p.C + 31) & ~31;
  float* coef = reinterpret_cast<float*>(smem);  // [2][Cr]: scale, shift (zeros past C)
  float* red = coef + 2 * Cr;                    // [4 waves][2][16]
  char* bufs = smem + (size_t)(2 * Cr + 128) * 4;
  const uint32_t patch_b = (uint32_t)p.patch_pix * 64u;
  const uint32_t buf_b = NPL * (patch_b + DN_WBYTES);

  // ---- BN coefficients of the C input channels from the replica sums; block 0 publishes the moments
  bn_coef_from_acc(p, coef, Cr, p.N * p.H * p.W, blockIdx.x == 0);
  __syncthreads();

  const __amdgpu_buffer_rsrc_t xr = make_rsrc(p.x, p.x_bytes);
  __amdgpu_buffer_rsrc_t wr[NPL];
  wr[0] = make_rsrc(p.w, p.w_bytes);
  if constexpr (F32) {
    wr[1] = make_rsrc(p.w_mid, p.w_bytes);
    wr[2] = make_rsrc(p.w_lo, p.w_bytes);
  }
  const int v = tid & 3;  // the thread's 16-byte column of every unit it stages (256 % 4 == 0)
  const int W2 = p.W + 2;

  // the weight vectors this thread stages: unit = tap * 16 + row
  uint32_t woff[DN_WIT], wlds[DN_WIT];
#pragma unroll
  for (int it = 0; it < DN_WIT; ++it) {
    const int unit = (it * 256 + tid) >> 2;
    const int tap = unit >> 4, row = unit & 15;
    const bool ok = unit < DN_WUNITS && row < p.Nout;
    woff[it] = ok ? (uint32_t)(row * p.Kpad + tap * p.C) * 2u : HCB_OOB;
    wlds[it] = unit < DN_WUNITS ? patch_off(unit, v) : HCB_OOB;
  }
  const uint32_t a0 = patch_off(frow, fq);  // this lane's weight fragment of tap 0; tap t: + t * 1024

  float kout[4];
#pragma unroll
  for (int e = 0; e < 4; ++e)
    kout[e] = (p.stats_shift != nullptr && fq * 4 + e < p.Nout) ? p.stats_shift[fq * 4 + e] : 0.f;
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};

  const int nchunks = Cr >> 5;
  for (int strip = blockIdx.x; strip < p.nstrips; strip += gridDim.x) {
    const int n = strip / p.strips_per_img;
    const int h0 = (strip - n * p.strips_per_img) * p.TR;
    const int rows = min(p.TR, p.H - h0);
    const int npix = rows * p.W;
    const int ntiles = (npix + 15) >> 4;

    // the patch vectors this thread stages: byte offset of the pixel (or out of range) and LDS place
    uint32_t goff[DN_MAXIT], plds[DN_MAXIT];
#pragma unroll
    for (int it = 0; it < DN_MAXIT; ++it) {
      const int pp = (it * 256 + tid) >> 2;
      const int r = pp / W2, c = pp - r * W2;
      const int h = h0 - 1 + r, w = c - 1;
      const bool in = pp < p.patch_pix;
      const bool ok = in && (unsigned)h < (unsigned)p.H && (unsigned)w < (unsigned)p.W;
      goff[it] = ok ? (uint32_t)(((size_t)(n * p.H + h) * p.W + w) * p.ldx) * E : HCB_OOB;
      plds[it] = in ? patch_off(pp, v) : HCB_OOB;
    }
    // the pixel fragments this lane reads: tile = wave + 4 * ti, pixel frow of it (clamped into the strip)
    uint32_t baddr[DN_TILES][9];
#pragma unroll
    for (int ti = 0; ti < DN_TILES; ++ti) {
      const int o = min((wave + 4 * ti) * 16 + frow, npix - 1);
      const int orow = o / p.W, ocol = o - orow * p.W;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) baddr[ti][tap] = patch_off((orow + tap / 3) * W2 + ocol + tap % 3, fq);
    }

    Act8<T> xv[DN_MAXIT];
    u32x4 wv[DN_WIT][NPL];
    auto gload = [&](int c0) {
      const int cc = c0 + v * 8;
      const bool cok = cc < p.C;
#pragma unroll
      for (int it = 0; it < DN_MAXIT; ++it)
        xv[it].load(xr, (cok && goff[it] != HCB_OOB) ? goff[it] + (uint32_t)cc * E : HCB_OOB);
#pragma unroll
      for (int it = 0; it < DN_WIT; ++it)
#pragma unroll
        for (int t = 0; t < NPL; ++t)
          wv[it][t] = buf_load16(wr[t], (cok && woff[it] != HCB_OOB) ? woff[it] + (uint32_t)cc * 2u : HCB_OOB);
    };
    auto lstore = [&](int b, int c0) {
      char* pb = bufs + (size_t)b * buf_b;
      char* wb = pb + NPL * patch_b;
      float sc[8], sh[8];
      bn_coef_load8(coef, Cr, c0 + v * 8, sc, sh);
#pragma unroll
      for (int it = 0; it < DN_MAXIT; ++it)
        if (plds[it] != HCB_OOB) bnrelu_store<T>(pb, patch_b, plds[it], xv[it], goff[it] != HCB_OOB, sc, sh);
#pragma unroll
      for (int it = 0; it < DN_WIT; ++it) {
        if (wlds[it] == HCB_OOB) continue;
#pragma unroll
        for (int t = 0; t < NPL; ++t) *reinterpret_cast<u32x4*>(wb + t * DN_WBYTES + wlds[it]) = wv[it][t];
      }
    };

    f32x4 acc[DN_TILES];
#pragma unroll
    for (int ti = 0; ti < DN_TILES; ++ti) acc[ti] = f32x4{0.f, 0.f, 0.f, 0.f};

    gload(0);
    lstore(0, 0);
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
      const bool more = c + 1 < nchunks;
      if (more) gload((c + 1) * 32);
      {
        const char* pb = bufs + (size_t)(c & 1) * buf_b;
        const char* wb = pb + NPL * patch_b;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          u32x4 a[NPL];
#pragma unroll
          for (int t = 0; t < NPL; ++t) a[t] = *reinterpret_cast<const u32x4*>(wb + t * DN_WBYTES + a0 + tap * 1024);
#pragma unroll
          for (int ti = 0; ti < DN_TILES; ++ti) {
            if (wave + 4 * ti >= ntiles) continue;  // (wave-uniform)
            u32x4 bb[NPL];
#pragma unroll
            for (int t = 0; t < NPL; ++t) bb[t] = *reinterpret_cast<const u32x4*>(pb + t * patch_b + baddr[ti][tap]);
            mfma_acc<F32>(a, bb, acc[ti]);
          }
        }
      }
      if (more) lstore((c + 1) & 1, (c + 1) * 32);
      __syncthreads();
    }

    // ---- the strip's outputs: lane = pixel frow of its tiles, channels fq * 4 .. + 3
    const size_t m0 = ((size_t)n * p.H + h0) * p.W;
#pragma unroll
    for (int ti = 0; ti < DN_TILES; ++ti) {
      const int o = (wave + 4 * ti) * 16 + frow;
      if (o >= npix) continue;
      // the slot's pad channels are structural zeros: stored as literal zeros (not as 0 * operand, which
      // an Inf or NaN operand would turn into NaN), and their statistics stay zero with them
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (fq * 4 + e >= p.Nout) acc[ti][e] = 0.f;
      if (p.stats != nullptr) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = acc[ti][e] - kout[e];
          s1[e] += d;
          s2[e] += d * d;
        }
      }
      T* dst = reinterpret_cast<T*>(p.y) + (m0 + o) * p.ldy + fq * 4;
      if constexpr (F32) {
        *reinterpret_cast<f32x4*>(dst) = acc[ti];
      } else {
        u32x2 o2;
        o2[0] = pack2(acc[ti][0], acc[ti][1]);
        o2[1] = pack2(acc[ti][2], acc[ti][3]);
        *reinterpret_cast<u32x2*>(dst) = o2;
      }
    }
  }

  if (p.stats == nullptr) return;  // (uniform)
  stats_reduce<1>(s1, s2, red, p.stats, p.stats_R, p.stats_C, 0, wave, frow, fq);
}

// strip rows and patch size for this problem; false when even one-row strips do not fit
bool dn_plan(int H, int W, int C, bool f32, int* TR_out, int* pix_out, size_t* lds_out) {
  if (W > 128) return false;
  int TR = 128 / W;
  if (TR > 16) TR = 16;
  if (TR > H) TR = H;
  // small maps: shorter strips, so that a batch of 64 launches 128 - 256 workgroups instead of 64 - 128
  // (16 x 16: 4 rows, 8 x 8: 4 rows). The strip depends on the map alone: a layer runs the same code
  // path at every batch
  if (H * W <= 64 && H >= 2)
    TR = (H + 1) / 2;
  else if (H * W <= 256 && TR * W > 64)
    TR = 64 / W > 0 ? 64 / W : 1;
  for (; TR >= 1; --TR) {
    const int pix = (TR + 2) * (W + 2);
    const size_t lds = dn_lds_bytes(C, pix, f32);
    if (pix * 4 <= DN_MAXIT * 256 && lds <= DN_LDS_MAX) {
      *TR_out = TR;
      *pix_out = pix;
      *lds_out = lds;
      return true;
    }
  }
  return false;
}

}  // namespace

bool dense_conv3x3_fits(int N, int H, int W, int C, bool f32) {
  int TR, pix;
  size_t lds;
  return N >= 1 && dn_plan(H, W, C, f32, &TR, &pix, &lds);
}

void launch_dense_conv3x3(const DenseParams& p0, hipStream_t st, bool f32) {
  DenseParams p = p0;
  size_t lds;
  if (!dn_plan(p.H, p.W, p.C, f32, &p.TR, &p.patch_pix, &lds)) {  // (the binding refuses it by name first)
    fprintf(stderr, "hcb dense_conv3x3: W = %d, C = %d does not fit the LDS budget\n", p.W, p.C);
    abort();
  }
  p.strips_per_img = (p.H + p.TR - 1) / p.TR;
  p.nstrips = p.N * p.strips_per_img;
  dim3 grid((unsigned)p.nstrips);
  // deterministic mode: at most R blocks, so each replica slot receives a single add
  if (p.stats != nullptr && deterministic() && (int)grid.x > p.stats_R) grid.x = p.stats_R;
  if (f32)
    launch_big_lds(dense_conv3x3_kernel<float>, grid, lds, st, p, "dense_conv3x3");
  else
    launch_big_lds(dense_conv3x3_kernel<uint16_t>, grid, lds, st, p, "dense_conv3x3");
}

}  // namespace hcb
