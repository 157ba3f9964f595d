// The whole MobileNet-v2 inverted-residual block, 16-bit inference, in ONE launch on gfx950:
//   h1  = relu6(bn1(x @ We))               1x1 expand cin -> mid, we [mid][Kpad1]; without an expand h1 = x, mid = cin
//   h2  = relu6(bn2(dw3x3_SAME(s)(h1)))    depthwise, wd fp32 [mid][3][3], stride s in {1, 2}
//   out = bn3(h2 @ Wp) [+ res]             1x1 linear projection mid -> cout, wp [cout][Kpad2]; res added in fp32
// x [N][H][W] (row stride ldx), res / out [N][P][Q] (row strides ldr / ldo). The three BatchNorms use their moving
// statistics. The pads of the depthwise belong to the ACTIVATED h1: outside the image it is 0, not relu6(shift). The
// expanded tensors h1 and h2 -- six times the block's channels -- never leave the chip; each is rounded to 16 bits once.
//
// Work split. A workgroup of 4 waves owns a strip of TR whole output rows of one image. It stages the raw x patch --
// (TR - 1) s + 3 rows x W columns, all cin channels in 32-channel planes (K zero-padded to the MFMA's 32) -- ONCE, with
// range-checked 16-byte buffer loads, into the swizzled 64-byte units of patch3x3.h. Then it loops over chunks of
// MC = 32 expanded channels (a last partial chunk runs on zero weights and zero coefficients):
//   1 expand     patch pixels x cin -> 32 channels by v_mfma_f32_16x16x32: wave w takes pixel tiles w, w + 4, ... and
//                both 16-channel tiles, so a pixel fragment is read once for two MFMAs. BN1 + ReLU6 in fp32 on the
//                accumulators, rows outside the image selected to zero, one rounding, 8-byte stores into the h1 patch
//                ((TR - 1) s + 3 rows x (W + 2) columns of 64-byte units; columns 0 and W + 1 stay zero). Without an
//                expand the x plane of the chunk is copied there instead.
//   2 depthwise  thread (pixel, 8-channel column): nine 16-byte reads of the h1 patch (stride 2 is an address
//                pattern), the 72 fp32 weights of its channels in registers, fp32 FMAs, BN2 + ReLU6, one rounding, a
//                16-byte store into the h2 tile -- the unit layout the next MFMA reads as its pixel operand.
//   3 project    strip pixels x 32 -> cout, accumulated in fp32 registers ACROSS the chunks. The waves split the
//                16-column tiles of cout cw = 1 | 2 | 4 ways and the pixel tiles 4 / cw ways: J x I accumulator tiles per
//                wave (J column tiles whose weight fragments stay in registers over the I pixel tiles), 80 registers.
// The chunk's three weight blocks (expand [32][cin], depthwise [32][9] fp32, project [cout][32]) of chunk g + 1 are
// loaded global -> registers before the MFMAs of chunk g and stored to the other LDS buffer before the barrier that
// already publishes h2. Two barriers per chunk: h1 and h2 are single buffers (expand g + 1 may overlap project g).
// After the last chunk: BN3 on the accumulators, + res in fp32, one rounding, 8-byte stores of channels < cout only.
//
// BN scale / shift of all three layers are derived at kernel start from the live parameter vectors (inf_coeff's
// arithmetic), so a graph replay sees parameters that changed since capture. No statistics, no atomics, no memset, no
// scratch, nothing relies on zeroed memory; every output element is one thread's fixed-order sum.
//
// Strip rows (mb_plan): the tile budgets bound TR from above; below that bound the plan takes the SMALLEST TR >= 2
// whose grid still is at most one workgroup per CU (256), because on the 14 x 14 and 7 x 7 maps at batch 32 whole-image
// strips leave 32 workgroups on 256 CUs. TR = 1 is not taken where 2 fits: it recomputes the expand three times. No
// second grid dimension over cout. Resources per model layer: profiles/mobilenet_block.txt.
#include <cstdio>
#include <cstdlib>

#include "common.h"
#include "kernels.h"
#include "patch3x3.h"

namespace hcb {

namespace {

constexpr int MB_MC = 32;      // expanded channels per chunk: one K step of the project MFMA
constexpr int MB_XIT = 6;      // x-patch vectors per thread and 32-channel plane: x_pix <= 384
constexpr int MB_T1 = 6;       // expand pixel tiles per wave: x_pix <= 16 * 4 * MB_T1
constexpr int MB_NK1 = 5;      // K planes of the expand: cin <= 160
constexpr int MB_WE = 3;       // expand-weight vectors per thread and chunk: 32 rows x MB_NK1 planes x 4 / 256
constexpr int MB_WP = 5;       // project-weight vectors per thread and chunk: cout <= 320
constexpr int MB_ACC = 20;     // project accumulator tiles per wave (J x I)
constexpr int MB_GRID = 256;   // workgroups the strip rule aims below: one per CU
constexpr int MB_DWF = MB_MC * 9;  // depthwise weights of a chunk (floats)

__device__ __forceinline__ float relu6f(float v) { return fminf(fmaxf(v, 0.f), 6.f); }

template <int J, int I>
__global__ __launch_bounds__(256) void mbconv_block_kernel(MbconvBlockParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id_uniform();
  const int frow = lane & 15, fq = lane >> 4;
  const int v = tid & 3;  // the thread's 16-byte column of every unit it stages or filters (256 % 4 == 0)
  const int midr = p.nch * MB_MC, coutr = p.nct * 16;
  const bool expand = p.we != nullptr;
  float* coef1 = reinterpret_cast<float*>(smem);  // [2][midr]: scale, shift of BN1 (zeros past mid)
  float* coef2 = coef1 + 2 * midr;                // [2][midr]: of BN2
  float* coef3 = coef2 + 2 * midr;                // [2][coutr]: of BN3
  float* dwb = coef3 + 2 * coutr;                 // [2][MB_DWF]
  char* xpatch = reinterpret_cast<char*>(dwb + 2 * MB_DWF);
  const uint32_t xplane_b = (uint32_t)p.x_pix * 64u;
  char* h1 = xpatch + (size_t)p.nkx * xplane_b;
  const uint32_t h1_b = (uint32_t)p.h1_pix * 64u;
  char* h2 = h1 + h1_b;
  char* web = h2 + (size_t)p.h2_pix * 64u;  // [2][nk1 planes][32 units]
  const uint32_t we_b = (uint32_t)p.nk1 * 2048u;
  char* wpb = web + 2 * (size_t)we_b;  // [2][coutr units]
  const uint32_t wp_b = (uint32_t)coutr * 64u;
  const int s = p.stride, W = p.W, HW = p.HW, Q = p.Q;

  const int n = blockIdx.x / p.strips_per_img;
  const int r0 = (blockIdx.x - n * p.strips_per_img) * p.TR;  // first output row
  const int rows = min(p.TR, p.P - r0);
  const int h0 = r0 * s - p.pt;                   // image row of patch row 0
  const int M1 = ((rows - 1) * s + 3) * W, npt1 = (M1 + 15) >> 4;  // patch pixels the strip reads
  const int M2 = rows * Q, npt2 = (M2 + 15) >> 4;

  const __amdgpu_buffer_rsrc_t xr = make_rsrc(p.x, p.x_bytes);
  const __amdgpu_buffer_rsrc_t wer = make_rsrc(p.we, p.we_bytes), wpr = make_rsrc(p.wp, p.wp_bytes);
  const __amdgpu_buffer_rsrc_t wdr = make_rsrc(p.wd, p.wd_bytes);

  // ---- weights of chunk g: global -> registers (gloadw) -> LDS buffer b (lstorew)
  u32x4 wve[MB_WE], wvp[MB_WP], wvd = u32x4{0u, 0u, 0u, 0u};
  auto gloadw = [&](int g) {
    if (expand) {
#pragma unroll
      for (int it = 0; it < MB_WE; ++it) {
        const int unit = (it * 256 + tid) >> 2;
        const int row = g * MB_MC + (unit & 31), k = (unit >> 5) * 32 + v * 8;
        const bool ok = unit < p.nk1 * 32 && row < p.mid && k < p.cin;
        wve[it] = buf_load16(wer, ok ? (uint32_t)(row * p.Kpad1 + k) * 2u : HCB_OOB);
      }
    }
#pragma unroll
    for (int it = 0; it < MB_WP; ++it) {
      const int row = (it * 256 + tid) >> 2, k = g * MB_MC + v * 8;
      wvp[it] = buf_load16(wpr, (row < p.cout && k < p.mid) ? (uint32_t)(row * p.Kpad2 + k) * 2u : HCB_OOB);
    }
    // (channels past mid of a last partial chunk lie past wd_bytes: the range check returns zeros)
    if (tid < MB_DWF / 4) wvd = buf_load16(wdr, (uint32_t)(g * MB_DWF + tid * 4) * 4u);
  };
  auto lstorew = [&](int b) {
    if (expand) {
#pragma unroll
      for (int it = 0; it < MB_WE; ++it) {
        const int unit = (it * 256 + tid) >> 2;
        if (unit < p.nk1 * 32)
          *reinterpret_cast<u32x4*>(web + (size_t)b * we_b + (unit >> 5) * 2048 + patch_off(unit & 31, v)) = wve[it];
      }
    }
#pragma unroll
    for (int it = 0; it < MB_WP; ++it) {
      const int row = (it * 256 + tid) >> 2;
      if (row < coutr) *reinterpret_cast<u32x4*>(wpb + (size_t)b * wp_b + patch_off(row, v)) = wvp[it];
    }
    if (tid < MB_DWF / 4) *reinterpret_cast<u32x4*>(dwb + b * MB_DWF + tid * 4) = wvd;
  };

  gloadw(0);
  // ---- the raw x patch, once: plane c = channels 32 c .. 32 c + 31, rows outside the image and channels past cin zero
  for (int c = 0; c < p.nkx; ++c) {
    const int cc = c * 32 + v * 8;
    u32x4 xv[MB_XIT];
#pragma unroll
    for (int it = 0; it < MB_XIT; ++it) {
      const int pp = (it * 256 + tid) >> 2;
      const int r = pp / W, col = pp - r * W;
      const int h = h0 + r;
      const bool ok = cc < p.cin && pp < M1 && (unsigned)h < (unsigned)p.H;
      xv[it] = buf_load16(xr, ok ? (uint32_t)((((size_t)(n * p.H + h) * W + col) * p.ldx + cc) * 2u) : HCB_OOB);
    }
#pragma unroll
    for (int it = 0; it < MB_XIT; ++it) {
      const int pp = (it * 256 + tid) >> 2;
      if (pp < M1) *reinterpret_cast<u32x4*>(xpatch + (size_t)c * xplane_b + patch_off(pp, v)) = xv[it];
    }
  }
  // BN coefficients from the live vectors (inf_coeff's arithmetic); zeros past mid / cout
  for (int c = tid; c < 2 * midr + coutr; c += 256) {
    const int l = c < midr ? 0 : c < 2 * midr ? 1 : 2;
    const int k = c - (l == 2 ? 2 * midr : l * midr);
    float sc = 0.f, sh = 0.f;
    if (k < (l == 2 ? p.cout : p.mid) && (l != 0 || expand)) {
      const float g = l == 0 ? p.gamma1[k] : l == 1 ? p.gamma2[k] : p.gamma3[k];
      const float b = l == 0 ? p.beta1[k] : l == 1 ? p.beta2[k] : p.beta3[k];
      const float m = l == 0 ? p.mean1[k] : l == 1 ? p.mean2[k] : p.mean3[k];
      const float var = l == 0 ? p.var1[k] : l == 1 ? p.var2[k] : p.var3[k];
      sc = g * (1.f / sqrtf(var + (l == 0 ? p.eps1 : l == 1 ? p.eps2 : p.eps3)));
      sh = b - m * sc;
    }
    float* dst = l == 0 ? coef1 : l == 1 ? coef2 : coef3;
    dst[k] = sc;
    dst[(l == 2 ? coutr : midr) + k] = sh;
  }
  // the h1 patch starts as zeros: its border columns are never written again
  for (uint32_t i = (uint32_t)tid * 16u; i < h1_b; i += 4096u) *reinterpret_cast<u32x4*>(h1 + i) = u32x4{0u, 0u, 0u, 0u};
  lstorew(0);
  __syncthreads();

  // this lane's pixel of expand tile i: its x-patch offset (clamped into the strip), its h1 unit (-1: no pixel), and
  // whether its row lies in the image
  uint32_t xo[MB_T1];
  int hu[MB_T1];
  uint32_t inimg = 0;
#pragma unroll
  for (int i = 0; i < MB_T1; ++i) {
    const int o = (wave + 4 * i) * 16 + frow;
    const int oc = min(o, M1 - 1);
    const int r = oc / W, col = oc - r * W;
    xo[i] = patch_off(oc, fq);
    hu[i] = o < M1 ? r * HW + col + 1 : -1;
    inimg |= (unsigned)(h0 + r) < (unsigned)p.H ? 1u << i : 0u;
  }

  const int cw = p.cw, cq = wave % cw, pq = wave / cw, npw = 4 / cw;  // project: column tiles cq + cw j, pixel tiles pq + npw i
  f32x4 acc2[J][I];
#pragma unroll
  for (int j = 0; j < J; ++j)
#pragma unroll
    for (int i = 0; i < I; ++i) acc2[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int g = 0; g < p.nch; ++g) {
    if (g + 1 < p.nch) gloadw(g + 1);
    // ---- step 1: the h1 chunk patch
    if (expand) {
      f32x4 acc1[MB_T1][2];
#pragma unroll
      for (int i = 0; i < MB_T1; ++i) acc1[i][0] = acc1[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
      const char* wb = web + (size_t)(g & 1) * we_b;
      for (int k = 0; k < p.nk1; ++k) {
        const u32x4 a0 = *reinterpret_cast<const u32x4*>(wb + k * 2048 + patch_off(frow, fq));
        const u32x4 a1 = *reinterpret_cast<const u32x4*>(wb + k * 2048 + patch_off(16 + frow, fq));
        const char* pb = xpatch + (size_t)k * xplane_b;
#pragma unroll
        for (int i = 0; i < MB_T1; ++i) {
          if (wave + 4 * i >= npt1) continue;  // (wave-uniform)
          const u32x4 bb = *reinterpret_cast<const u32x4*>(pb + xo[i]);
          acc1[i][0] = mfma16(__builtin_bit_cast(act16x8, a0), __builtin_bit_cast(act16x8, bb), acc1[i][0]);
          acc1[i][1] = mfma16(__builtin_bit_cast(act16x8, a1), __builtin_bit_cast(act16x8, bb), acc1[i][1]);
        }
      }
      // BN1 + ReLU6, one rounding: lane = pixel frow, channels j .. j + 3 of the chunk
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        const int j = ct * 16 + fq * 4;
        const f32x4 sc = *reinterpret_cast<const f32x4*>(coef1 + g * MB_MC + j);
        const f32x4 sh = *reinterpret_cast<const f32x4*>(coef1 + midr + g * MB_MC + j);
#pragma unroll
        for (int i = 0; i < MB_T1; ++i) {
          if (wave + 4 * i >= npt1 || hu[i] < 0) continue;
          const bool in = (inimg >> i) & 1u;
          float f[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) f[e] = in ? relu6f(acc1[i][ct][e] * sc[e] + sh[e]) : 0.f;
          u32x2 o2;
          o2[0] = pack2(f[0], f[1]);
          o2[1] = pack2(f[2], f[3]);
          *reinterpret_cast<u32x2*>(h1 + patch_off(hu[i], j >> 3) + (fq & 1) * 8) = o2;
        }
      }
    } else {
      const char* pb = xpatch + (size_t)g * xplane_b;
      for (int pp = tid >> 2; pp < M1; pp += 64) {
        const int r = pp / W, col = pp - r * W;
        *reinterpret_cast<u32x4*>(h1 + patch_off(r * HW + col + 1, v)) = *reinterpret_cast<const u32x4*>(pb + patch_off(pp, v));
      }
    }
    __syncthreads();

    // ---- step 2: depthwise 3x3 + BN2 + ReLU6 into the h2 tile
    {
      float wd[72];
      const f32x4* ws = reinterpret_cast<const f32x4*>(dwb + (g & 1) * MB_DWF + v * 72);
#pragma unroll
      for (int q = 0; q < 18; ++q) {
        const f32x4 t = ws[q];
#pragma unroll
        for (int e = 0; e < 4; ++e) wd[q * 4 + e] = t[e];
      }
      float sc[8], sh[8];
      bn_coef_load8(coef2, midr, g * MB_MC + v * 8, sc, sh);
      for (int pix = tid >> 2; pix < M2; pix += 64) {
        const int orow = pix / Q, ocol = pix - orow * Q;
        const int base = orow * s * HW + ocol * s - p.pl + 1;
        float a[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = 0.f;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          const u32x4 hv = *reinterpret_cast<const u32x4*>(h1 + patch_off(base + (tap / 3) * HW + tap % 3, v));
          float f[8];
          unpack8(hv, f);
#pragma unroll
          for (int e = 0; e < 8; ++e) a[e] = fmaf(f[e], wd[e * 9 + tap], a[e]);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = relu6f(a[e] * sc[e] + sh[e]);
        *reinterpret_cast<u32x4*>(h2 + patch_off(pix, v)) = pack8(a);
      }
    }
    if (g + 1 < p.nch) lstorew((g + 1) & 1);
    __syncthreads();

    // ---- step 3: project, accumulated across the chunks
    {
      const char* wb = wpb + (size_t)(g & 1) * wp_b;
      u32x4 a[J];
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const int ct = min(cq + cw * j, p.nct - 1);
        a[j] = *reinterpret_cast<const u32x4*>(wb + patch_off(ct * 16 + frow, fq));
      }
#pragma unroll
      for (int i = 0; i < I; ++i) {
        const int pt = pq + npw * i;
        if (pt >= npt2) continue;  // (wave-uniform)
        const u32x4 bb = *reinterpret_cast<const u32x4*>(h2 + patch_off(min(pt * 16 + frow, M2 - 1), fq));
#pragma unroll
        for (int j = 0; j < J; ++j) {
          if (cq + cw * j >= p.nct) continue;  // (wave-uniform)
          acc2[j][i] = mfma16(__builtin_bit_cast(act16x8, a[j]), __builtin_bit_cast(act16x8, bb), acc2[j][i]);
        }
      }
    }
  }

  // ---- BN3, + res in fp32, one rounding; lane = pixel frow, channels co .. co + 3 (only below cout)
  const size_t m0 = ((size_t)n * p.P + r0) * Q;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int co = (cq + cw * j) * 16 + fq * 4;
    if (co >= p.cout) continue;
    const f32x4 sc = *reinterpret_cast<const f32x4*>(coef3 + co);
    const f32x4 sh = *reinterpret_cast<const f32x4*>(coef3 + coutr + co);
#pragma unroll
    for (int i = 0; i < I; ++i) {
      const int o = (pq + npw * i) * 16 + frow;
      if (o >= M2) continue;
      float f[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) f[e] = acc2[j][i][e] * sc[e] + sh[e];
      if (p.res != nullptr) {
        const u32x2 rv = *reinterpret_cast<const u32x2*>(reinterpret_cast<const uint16_t*>(p.res) + (m0 + o) * p.ldr + co);
        f[0] += act2f((uint16_t)(rv[0] & 0xffffu));
        f[1] += act2f((uint16_t)(rv[0] >> 16));
        f[2] += act2f((uint16_t)(rv[1] & 0xffffu));
        f[3] += act2f((uint16_t)(rv[1] >> 16));
      }
      u32x2 o2;
      o2[0] = pack2(f[0], f[1]);
      o2[1] = pack2(f[2], f[3]);
      *reinterpret_cast<u32x2*>(reinterpret_cast<uint16_t*>(p.out) + (m0 + o) * p.ldo + co) = o2;
    }
  }
}

struct MbPlan {
  int P, Q, pt, pl, TR, HW, xpix, h1pix, h2pix, nk1, nkx, nch, nct, cw, J;
  size_t lds;
};

// strip rows, tile split, patch sizes and LDS bytes for this problem; false for a shape the kernel does not take or
// one whose one-row strip exceeds the tile or LDS budget
bool mb_plan(int N, int H, int W, int cin, int mid, int cout, int s, bool expand, MbPlan* pl) {
  if (N < 1 || H < 1 || W < 1 || !(s == 1 || s == 2)) return false;
  if (cin < 8 || mid < 8 || cout < 8 || cin % 8 || mid % 8 || cout % 8) return false;
  if (!expand && mid != cin) return false;
  if (cout > 16 * 4 * (MB_ACC / 4) || (expand && cin > 32 * MB_NK1)) return false;
  pl->nct = (cout + 15) / 16;
  pl->cw = pl->nct >= 4 ? 4 : pl->nct >= 2 ? 2 : 1;
  const int j = (pl->nct + pl->cw - 1) / pl->cw;
  pl->J = j == 4 ? 5 : j;  // instantiated: (1, 20), (2, 10), (3, 6), (5, 4)
  const int I = MB_ACC / pl->J;
  pl->nch = (mid + MB_MC - 1) / MB_MC;
  pl->nk1 = expand ? (cin + 31) / 32 : 0;
  pl->nkx = expand ? pl->nk1 : pl->nch;
  same3(H, s, &pl->P, &pl->pt);
  same3(W, s, &pl->Q, &pl->pl);
  pl->HW = W + 2;
  int best = 0;
  for (int TR = 1; TR <= pl->P; ++TR) {
    const int IR = (TR - 1) * s + 3;
    const int xpix = IR * W, h1pix = IR * pl->HW, h2pix = TR * pl->Q;
    const size_t lds = (size_t)(4 * pl->nch * MB_MC + 2 * pl->nct * 16 + 2 * MB_DWF) * 4 +
                       ((size_t)pl->nkx * xpix + h1pix + h2pix + 2 * 32 * pl->nk1 + 2 * 16 * pl->nct) * 64;
    if (xpix > 16 * 4 * MB_T1 || xpix * 4 > MB_XIT * 256 || h2pix > 16 * I * (4 / pl->cw) || lds > PATCH_LDS_LIMIT) break;
    best = TR;
    pl->TR = TR; pl->xpix = xpix; pl->h1pix = h1pix; pl->h2pix = h2pix; pl->lds = lds;
    if (TR >= 2 && (int64_t)N * ((pl->P + TR - 1) / TR) <= MB_GRID) break;  // the smallest TR >= 2 that fills one wave of CUs
  }
  return best > 0;
}

template <int J, int I>
void mb_launch(const MbconvBlockParams& p, dim3 grid, size_t lds, hipStream_t st) {
  launch_big_lds(mbconv_block_kernel<J, I>, grid, lds, st, p, "mbconv_block");
}

}  // namespace

bool mbconv_block_fits(int N, int H, int W, int cin, int mid, int cout, int stride, bool expand) {
  MbPlan pl;
  return mb_plan(N, H, W, cin, mid, cout, stride, expand, &pl);
}

void launch_mbconv_block(const MbconvBlockParams& p0, hipStream_t st) {
  MbconvBlockParams p = p0;
  MbPlan pl;
  if (!mb_plan(p.N, p.H, p.W, p.cin, p.mid, p.cout, p.stride, p.we != nullptr, &pl)) {  // (the binding refuses it by name first)
    fprintf(stderr, "hcb mbconv_block: %d x %d x %d -> %d -> %d, stride %d does not fit\n", p.H, p.W, p.cin, p.mid, p.cout,
            p.stride);
    abort();
  }
  p.P = pl.P; p.Q = pl.Q; p.pt = pl.pt; p.pl = pl.pl; p.TR = pl.TR; p.HW = pl.HW; p.x_pix = pl.xpix;
  p.h1_pix = pl.h1pix; p.h2_pix = pl.h2pix; p.nk1 = pl.nk1; p.nkx = pl.nkx; p.nch = pl.nch; p.nct = pl.nct; p.cw = pl.cw;
  p.strips_per_img = (p.P + p.TR - 1) / p.TR;
  const dim3 grid((unsigned)(p.N * p.strips_per_img));
  if (pl.J == 1)
    mb_launch<1, 20>(p, grid, pl.lds, st);
  else if (pl.J == 2)
    mb_launch<2, 10>(p, grid, pl.lds, st);
  else if (pl.J == 3)
    mb_launch<3, 6>(p, grid, pl.lds, st);
  else
    mb_launch<5, 4>(p, grid, pl.lds, st);
}

}  // namespace hcb
