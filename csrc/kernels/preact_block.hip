// The whole pre-activation basic block of the CIFAR ResNet-v2, 16-bit inference, in ONE launch on gfx950:
//   a1  = relu(bn1(x))                       moving statistics
//   z1  = conv3x3_SAME(stride s)(a1)         w1 [Nout][Kpad1]
//   a2  = relu(bn2(z1))                      conv1's BN, moving statistics
//   out = conv3x3_SAME(1)(a2) + res          w2 [Nout][Kpad2]; no bias, no ReLU after the add
// x [N][H][W] (row stride ldx), res / out [N][P][Q] (row strides ldr / ldo), C_in and Nout in {16, 32, 64}, s in
// {1, 2}. a1, z1 and a2 never leave the chip. Both pads belong to the ACTIVATED maps: out-of-image positions of a1
// and a2 are zero, not relu(shift). A sibling of preact3x3.hip (whose kernel stays the training / fp32 form): the
// 64-byte LDS unit, XOR swizzle and patch store of patch3x3.h, the same tap addressing, column tiles over the waves.
//
// Work split. A workgroup of 4 waves owns a strip of TR whole output rows of one image; wave w computes column tile
// w % NCT (NCT = Nout / 16) of the pixel tiles w / NCT + k * (4 / NCT) in both phases.
//
// Phase 1, conv1 into LDS. The raw x patch -- ((TR + 1) s + 3) x ((Q - 1) s + 3) pixels, ALL of its 32-channel
// chunks at once (it is at most 27 KiB) -- is loaded with range-checked 16-byte buffer loads, normalised and
// ReLU'd in fp32 registers, its halo selected to zero, and stored swizzled. conv1 is computed for the strip's rows
// and ONE row above and below (recomputed per strip; rows outside the image are skipped, not computed), all Q
// columns, so no column halo is ever computed: up to 3 pixel tiles per wave. The fp32 accumulators get BN2's
// scale / shift and the ReLU, are rounded to the 16-bit type once, and go to the a2 patch in LDS: (TR + 2) x (Q + 2)
// pixels x Nout channels in 32-channel planes of the same swizzled units. The patch is zeroed at kernel start, so
// its border columns, its out-of-image rows and (Nout = 16) the upper half of its one K chunk are zero.
//
// Phase 2, conv2 from LDS. The nine taps read the a2 patch at (orow + ty, ocol + tx); up to 2 pixel tiles per
// wave. The accumulators get res added in fp32 (8-byte loads at the store addresses, issued before the MFMAs) and
// leave as 16-bit. Every element of res is read by the thread that writes the same element of out.
//
// Weights. The two packs do not fit LDS together at 64 -> 64 (2 x 72 KiB), so they pass per 32-channel K chunk
// (9 taps x Nout rows x 64 bytes) through ONE pair of buffers as a sequence: conv1's chunks, then conv2's. Chunk
// g + 1 is loaded global -> registers before the MFMAs of chunk g and stored to buffer (g + 1) & 1 after them, one
// barrier per chunk -- so conv2's first chunk is in flight while conv1's last MFMAs run, and the barrier that
// publishes it also publishes the a2 patch.
//
// BN scale / shift of both layers are derived at kernel start from the live parameter vectors with the inference
// epilogue's arithmetic (igemm_epilogue.h inf_coeff), so a graph replay sees parameters that changed since
// capture. No statistics, no atomics, no memset, no scratch, nothing relies on zeroed memory: every output element
// is one thread's fixed-order sum, bitwise reproducible by construction.
//
// Dynamic LDS = 8 * (C32 + N32) + 64 * (nc1 * x_pix + nc2 * a2_pix + 2 * 9 * Nout) bytes (C32 / N32 = C_in / Nout
// rounded up to 32, nc = their chunk counts). Resources per instantiation: profiles/resnet_cifar_v2_block.txt.
#include <cstdio>
#include <cstdlib>

#include "common.h"
#include "kernels.h"
#include "patch3x3.h"

namespace hcb {

namespace {

constexpr int PB_MAXIT = 7;  // x-patch vectors (8 channels of one pixel) per thread and chunk
constexpr int PB_T1 = 3;     // 16-pixel MFMA tiles per wave, phase 1: (TR + 2) * Q <= 48 * (4 / NCT)
constexpr int PB_T2 = 2;     // phase 2: TR * Q <= 32 * (4 / NCT)
constexpr size_t PB_LDS_MAX = 160 * 1024;

template <int NCT>
__global__ __launch_bounds__(256) void preact_block_kernel(PreactBlockParams p) {
  constexpr int NW = 16 * NCT;                   // output channels of both convs
  constexpr int WUNITS = 9 * NW;                 // unit = tap * NW + row
  constexpr uint32_t WBYTES = WUNITS * 64u;
  constexpr int WIT = (WUNITS * 4 + 255) / 256;  // weight vectors per thread and chunk
  constexpr int NPW = 4 / NCT;                   // waves that share a column tile
  constexpr int NC2 = (NW + 31) / 32;            // K chunks of conv2
  constexpr int Nr = NC2 * 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id_uniform();
  const int frow = lane & 15, fq = lane >> 4;
  const int ct = wave % NCT, pw = wave / NCT;  // the wave's column tile, its first pixel tile
  const int Cr = (p.C + 31) & ~31, nc1 = Cr >> 5;
  float* coef1 = reinterpret_cast<float*>(smem);  // [2][Cr]: scale, shift of BN1 (zeros past C)
  float* coef2 = coef1 + 2 * Cr;                  // [2][Nr]: of BN2
  char* xpatch = smem + (size_t)(2 * Cr + 2 * Nr) * 4;
  const uint32_t patch_b = (uint32_t)p.patch_pix * 64u;
  char* a2 = xpatch + (size_t)nc1 * patch_b;
  const uint32_t a2_b = (uint32_t)p.a2_pix * 64u;
  char* wbuf = a2 + (size_t)NC2 * a2_b;  // [2][WBYTES]
  const int s = p.stride;
  const int v = tid & 3;  // the thread's 16-byte column of every unit it stages (256 % 4 == 0)

  const int n = blockIdx.x / p.strips_per_img;
  const int r0 = (blockIdx.x - n * p.strips_per_img) * p.TR;  // first output row
  const int rows = min(p.TR, p.P - r0);
  const int ra = max(r0 - 1, 0), rb = min(r0 + rows + 1, p.P);  // conv1 rows [ra, rb): the strip and its halo, in the image
  const int M1 = (rb - ra) * p.Q, nt1 = (M1 + 15) >> 4;
  const int M2 = rows * p.Q, nt2 = (M2 + 15) >> 4;
  const int h0 = (r0 - 1) * s - p.pt, w0 = -p.pl;  // image row / column of x-patch pixel (0, 0)

  const __amdgpu_buffer_rsrc_t xr = make_rsrc(p.x, p.x_bytes);
  const __amdgpu_buffer_rsrc_t w1r = make_rsrc(p.w1, p.w1_bytes), w2r = make_rsrc(p.w2, p.w2_bytes);

  // ---- weights: chunk g of the sequence (conv1's nc1 chunks, then conv2's NC2) global -> registers -> buffer g & 1
  u32x4 wv[WIT];
  auto gloadw_from = [&](__amdgpu_buffer_rsrc_t wr, int C, int Kpad, int c0) {
    const int cc = c0 + v * 8;
    const bool cok = cc < C;
#pragma unroll
    for (int it = 0; it < WIT; ++it) {
      const int unit = (it * 256 + tid) >> 2;
      const int tap = unit / NW, row = unit - tap * NW;
      wv[it] = buf_load16(wr, (cok && unit < WUNITS) ? (uint32_t)(row * Kpad + tap * C + cc) * 2u : HCB_OOB);
    }
  };
  auto gloadw = [&](int g) {
    if (g < nc1)
      gloadw_from(w1r, p.C, p.Kpad1, g * 32);
    else
      gloadw_from(w2r, NW, p.Kpad2, (g - nc1) * 32);
  };
  auto lstorew = [&](int b) {
    char* wb = wbuf + (size_t)b * WBYTES;
#pragma unroll
    for (int it = 0; it < WIT; ++it) {
      const int unit = (it * 256 + tid) >> 2;
      if (unit < WUNITS) *reinterpret_cast<u32x4*>(wb + patch_off(unit, v)) = wv[it];
    }
  };

  // ---- the x patch: chunk c global -> registers (xload), BN1 + ReLU, halo to zero -> LDS (xstore)
  Act8<uint16_t> xv[PB_MAXIT];
  uint32_t xin = 0;  // bit it: vector `it` lies inside the image and below C
  auto xload = [&](int c) {
    const int cc = c * 32 + v * 8;
    const bool cok = cc < p.C;
    xin = 0;
#pragma unroll
    for (int it = 0; it < PB_MAXIT; ++it) {
      const int pp = (it * 256 + tid) >> 2;
      const int r = pp / p.PW, col = pp - r * p.PW;
      const int h = h0 + r, w = w0 + col;
      const bool ok = cok && pp < p.patch_pix && (unsigned)h < (unsigned)p.H && (unsigned)w < (unsigned)p.W;
      xv[it].load(xr, ok ? (uint32_t)((((size_t)(n * p.H + h) * p.W + w) * p.ldx + cc) * 2u) : HCB_OOB);
      xin |= ok ? 1u << it : 0u;
    }
  };
  auto xstore = [&](int c) {
    char* pb = xpatch + (size_t)c * patch_b;
    float sc[8], sh[8];
    bn_coef_load8(coef1, Cr, c * 32 + v * 8, sc, sh);
#pragma unroll
    for (int it = 0; it < PB_MAXIT; ++it) {
      const int pp = (it * 256 + tid) >> 2;
      if (pp < p.patch_pix) bnrelu_store<uint16_t>(pb, patch_b, patch_off(pp, v), xv[it], (xin >> it) & 1u, sc, sh);
    }
  };

  gloadw(0);
  xload(0);
  // BN coefficients from the live vectors (inf_coeff's arithmetic), and the zeroed a2 patch
  for (int c = tid; c < Cr + Nr; c += 256) {
    const bool one = c < Cr;
    const int k = one ? c : c - Cr;
    float sc = 0.f, sh = 0.f;
    if (k < (one ? p.C : NW)) {
      const float g = one ? p.gamma1[k] : p.gamma2[k], b = one ? p.beta1[k] : p.beta2[k];
      const float m = one ? p.mean1[k] : p.mean2[k], var = one ? p.var1[k] : p.var2[k];
      sc = g * (1.f / sqrtf(var + (one ? p.eps1 : p.eps2)));
      sh = b - m * sc;
    }
    float* dst = one ? coef1 : coef2;
    dst[k] = sc;
    dst[(one ? Cr : Nr) + k] = sh;
  }
  for (uint32_t i = (uint32_t)tid * 16u; i < NC2 * a2_b; i += 4096u) *reinterpret_cast<u32x4*>(a2 + i) = u32x4{0u, 0u, 0u, 0u};
  __syncthreads();
  xstore(0);
  for (int c = 1; c < nc1; ++c) {
    xload(c);
    xstore(c);
  }
  lstorew(0);
  __syncthreads();

  const uint32_t a0 = patch_off(ct * 16 + frow, fq);  // this lane's weight fragment of tap 0; tap t: + t * NW * 64

  // ---- phase 1: conv1 of rows [ra, rb) from the x patch
  f32x4 acc1[PB_T1];
  int ub1[PB_T1];  // x-patch unit of tap (0, 0) of this lane's pixel of tile ti (clamped into the strip)
#pragma unroll
  for (int ti = 0; ti < PB_T1; ++ti) {
    acc1[ti] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int o = min((pw + NPW * ti) * 16 + frow, M1 - 1);
    const int rr = o / p.Q, col = o - rr * p.Q;
    ub1[ti] = (ra + rr - (r0 - 1)) * s * p.PW + col * s;
  }
  for (int c = 0; c < nc1; ++c) {
    gloadw(c + 1);  // (conv2's first chunk after conv1's last)
    const char* pb = xpatch + (size_t)c * patch_b;
    const char* wb = wbuf + (size_t)(c & 1) * WBYTES;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const u32x4 a = *reinterpret_cast<const u32x4*>(wb + a0 + tap * (NW * 64));
#pragma unroll
      for (int ti = 0; ti < PB_T1; ++ti) {
        if (pw + NPW * ti >= nt1) continue;  // (wave-uniform)
        const u32x4 bb = *reinterpret_cast<const u32x4*>(pb + patch_off(ub1[ti] + (tap / 3) * p.PW + tap % 3, fq));
        acc1[ti] = mfma16(__builtin_bit_cast(act16x8, a), __builtin_bit_cast(act16x8, bb), acc1[ti]);
      }
    }
    if (c + 1 == nc1) {
      // BN2 + ReLU, one rounding to 16 bits, into the a2 patch: lane = pixel frow, channels j .. j + 3
      const int j = ct * 16 + fq * 4;
      const f32x4 sc = *reinterpret_cast<const f32x4*>(coef2 + j);
      const f32x4 sh = *reinterpret_cast<const f32x4*>(coef2 + Nr + j);
      char* ab = a2 + (size_t)(j >> 5) * a2_b + ((j >> 2) & 1) * 8;
#pragma unroll
      for (int ti = 0; ti < PB_T1; ++ti) {
        const int o = (pw + NPW * ti) * 16 + frow;
        if (o >= M1) continue;
        const int rr = o / p.Q, col = o - rr * p.Q;
        const int unit = (ra + rr - (r0 - 1)) * p.AW + col + 1;
        float f[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) f[e] = fmaxf(acc1[ti][e] * sc[e] + sh[e], 0.f);
        u32x2 o2;
        o2[0] = pack2(f[0], f[1]);
        o2[1] = pack2(f[2], f[3]);
        *reinterpret_cast<u32x2*>(ab + patch_off(unit, (j & 31) >> 3)) = o2;
      }
    }
    lstorew((c + 1) & 1);
    __syncthreads();
  }

  // ---- phase 2: conv2 of the strip's rows from the a2 patch, + res
  const size_t m0 = ((size_t)n * p.P + r0) * p.Q;
  const int jo = ct * 16 + fq * 4;
  f32x4 acc2[PB_T2];
  int ub2[PB_T2];
  u32x2 rv[PB_T2];
#pragma unroll
  for (int ti = 0; ti < PB_T2; ++ti) {
    acc2[ti] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int o = (pw + NPW * ti) * 16 + frow;
    rv[ti] = u32x2{0u, 0u};
    if (o < M2) rv[ti] = *reinterpret_cast<const u32x2*>(reinterpret_cast<const uint16_t*>(p.res) + (m0 + o) * p.ldr + jo);
    const int oc = min(o, M2 - 1);
    const int orow = oc / p.Q, ocol = oc - orow * p.Q;
    ub2[ti] = orow * p.AW + ocol;
  }
#pragma unroll
  for (int c = 0; c < NC2; ++c) {
    const int g = nc1 + c;
    if (c + 1 < NC2) gloadw(g + 1);
    const char* pb = a2 + (size_t)c * a2_b;
    const char* wb = wbuf + (size_t)(g & 1) * WBYTES;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const u32x4 a = *reinterpret_cast<const u32x4*>(wb + a0 + tap * (NW * 64));
#pragma unroll
      for (int ti = 0; ti < PB_T2; ++ti) {
        if (pw + NPW * ti >= nt2) continue;  // (wave-uniform)
        const u32x4 bb = *reinterpret_cast<const u32x4*>(pb + patch_off(ub2[ti] + (tap / 3) * p.AW + tap % 3, fq));
        acc2[ti] = mfma16(__builtin_bit_cast(act16x8, a), __builtin_bit_cast(act16x8, bb), acc2[ti]);
      }
    }
    if (c + 1 < NC2) {
      lstorew((g + 1) & 1);
      __syncthreads();
    }
  }
#pragma unroll
  for (int ti = 0; ti < PB_T2; ++ti) {
    const int o = (pw + NPW * ti) * 16 + frow;
    if (o >= M2) continue;
    const float r0f = act2f((uint16_t)(rv[ti][0] & 0xffffu)), r1f = act2f((uint16_t)(rv[ti][0] >> 16));
    const float r2f = act2f((uint16_t)(rv[ti][1] & 0xffffu)), r3f = act2f((uint16_t)(rv[ti][1] >> 16));
    u32x2 o2;
    o2[0] = pack2(acc2[ti][0] + r0f, acc2[ti][1] + r1f);
    o2[1] = pack2(acc2[ti][2] + r2f, acc2[ti][3] + r3f);
    *reinterpret_cast<u32x2*>(reinterpret_cast<uint16_t*>(p.out) + (m0 + o) * p.ldo + jo) = o2;
  }
}

struct PbPlan {
  int nct, TR, P, Q, pt, pl, PW, pix, AW, a2pix;
  size_t lds;
};

// strip rows, patch sizes and LDS bytes for this problem; false for a shape the kernel does not take or one whose
// one-row strip exceeds the tile, staging or LDS budget
bool pb_plan(int H, int W, int C, int Nout, int s, PbPlan* pl) {
  if (!(C == 16 || C == 32 || C == 64) || !(Nout == 16 || Nout == 32 || Nout == 64) || !(s == 1 || s == 2)) return false;
  if (H < 1 || W < 1) return false;
  pl->nct = Nout / 16;
  const int npw = 4 / pl->nct;
  same3(H, s, &pl->P, &pl->pt);
  same3(W, s, &pl->Q, &pl->pl);
  const int Cr = (C + 31) & ~31, Nr = (Nout + 31) & ~31;
  pl->PW = (pl->Q - 1) * s + 3;
  pl->AW = pl->Q + 2;
  int TR = 16 * PB_T2 * npw / pl->Q;
  if (TR > pl->P) TR = pl->P;
  for (; TR >= 1; --TR) {
    if ((TR + 2) * pl->Q > 16 * PB_T1 * npw) continue;
    const int pix = ((TR + 1) * s + 3) * pl->PW, a2pix = (TR + 2) * pl->AW;
    const size_t lds = (size_t)(2 * Cr + 2 * Nr) * 4 +
                       ((size_t)(Cr / 32) * pix + (size_t)(Nr / 32) * a2pix + (size_t)2 * 9 * Nout) * 64;
    if (pix * 4 <= PB_MAXIT * 256 && lds <= PB_LDS_MAX) {
      pl->TR = TR;
      pl->pix = pix;
      pl->a2pix = a2pix;
      pl->lds = lds;
      return true;
    }
  }
  return false;
}

}  // namespace

bool preact_block_fits(int N, int H, int W, int C, int Nout, int stride) {
  PbPlan pl;
  return N >= 1 && pb_plan(H, W, C, Nout, stride, &pl);
}

void launch_preact_block(const PreactBlockParams& p0, hipStream_t st) {
  PreactBlockParams p = p0;
  PbPlan pl;
  if (!pb_plan(p.H, p.W, p.C, p.Nout, p.stride, &pl)) {  // (the binding refuses it by name first)
    fprintf(stderr, "hcb preact_block: %d x %d x %d -> %d, stride %d does not fit\n", p.H, p.W, p.C, p.Nout, p.stride);
    abort();
  }
  p.P = pl.P; p.Q = pl.Q; p.pt = pl.pt; p.pl = pl.pl; p.TR = pl.TR; p.PW = pl.PW; p.patch_pix = pl.pix;
  p.AW = pl.AW; p.a2_pix = pl.a2pix;
  p.strips_per_img = (p.P + p.TR - 1) / p.TR;
  const dim3 grid((unsigned)(p.N * p.strips_per_img));
  if (pl.nct == 1)
    launch_big_lds(preact_block_kernel<1>, grid, pl.lds, st, p, "preact_block");
  else if (pl.nct == 2)
    launch_big_lds(preact_block_kernel<2>, grid, pl.lds, st, p, "preact_block");
  else
    launch_big_lds(preact_block_kernel<4>, grid, pl.lds, st, p, "preact_block");
}

}  // namespace hcb
