// Weight gradient of the ResNet-v2 pre-activation conv on gfx950, with BatchNorm and ReLU applied on the way in:
//   dw[n][r][t][c] += sum_{img, p, q} dz[img][p][q][n] * a[img][p s + r - pt][q s + t - pl][c]
//   a = relu(x * sc + sh),  sc = gamma * invstd,  sh = beta - mean * sc,  a = 0 outside the image
// x = the block's raw input [N][H][W][ldx], dz = the gradient of conv1's raw output [N][P][Q][ldz] (P = ceil(H / s)),
// C_in and Nout each 16, 32 or 64, stride s = 1 or 2 with TF's 'SAME' pads (pt, pl), mean / invstd the moments the
// forward kernel (preact3x3.hip) saved. The normalised operand is never written: the unfused chain (bn_forward_acc
// writes it, conv_wgrad reads it back through a GEMM tiled for wide outputs) moves the block input three times,
// this kernel once. A sibling of dense3x3_wgrad.hip, which stays the one-row-tile, stride-1, 16-channel-slot kernel.
//
// Work split: the reduction runs over all N * P * Q output pixels, so the grid is (32-channel chunks of C_in) x
// (pixel slabs). A workgroup of 4 waves owns ONE chunk, walks the strips of its slab and multiplies each patch
// against ALL Nout columns of dz: the NRT = Nout / 16 row tiles go over the waves and over per-wave accumulators,
// never over a grid dimension (which would stage and normalise the same patch again). A strip is TR whole output
// rows of one image, TR * Q <= 128 pixels = at most 4 MFMA K blocks of 32 pixels. With NH = the 16-channel halves
// of the chunk that exist (C_in = 16: one; the other half is neither staged nor multiplied, and the patch unit
// shrinks to 32 bytes) a chunk has U = NRT * NH (row tile, half) units of 9 tap tiles each:
//   U = 1 (16 -> 16)            wave = K quarter: 4 waves x 9 tiles, K blocks kh, kh + 4, ...
//   U = 2 (16 -> 32, 32 -> 16)  wave = (unit, K half): 9 tiles, K blocks kh, kh + 2
//   U = 4 (32 -> 32, 16 -> 64)  wave = unit: 9 tiles, every K block
//   U = 8 (32 | 64 -> 64)       wave = row tile, both halves: 18 tiles = 72 accumulator registers, the dz fragment
//                               of a K block is read once and serves 18 taps
// so on the model's five layers (32 x 32 x 16 -> 16 and -> 32 / 2: 128-pixel strips = 4 K blocks; 16 x 16 x 32 -> 32;
// 16 x 16 x 32 -> 64 / 2; 8 x 8 x 64 -> 64) no wave idles.
// Per strip:
//   global -> registers   the chunk's input patch, ((TR - 1) s + 3) x ((Q - 1) s + 3) pixels x 16 NH channels, and the
//                         strip of dz, TR * Q pixels x Nout channels: range-checked 16-byte raw buffer loads (pixels
//                         outside the image / past the strip's end: the out-of-range offset, zeros).
//   registers -> LDS      BN + ReLU in fp32 in the forward's fmaxf(f * sc + sh, 0.f) form (a thread's 8 channels never
//                         change: sc / sh live in registers), halo pixels SELECTED to zero, not normalised; then
//                         16-bit, or on the fp32 path the bf16 hi / mid / lo split into three tiles, dz likewise.
//                         Patch unit = 32 NH bytes per pixel, its 16-byte columns XOR-swizzled with bits 2.. of the unit
//                         index (patch3x3.h: the shared unit, swizzle and patch store); dz rows are 2 Nout bytes, their 32-byte tile columns
//                         XOR-swizzled with the pixel index.
//   LDS -> MFMA           v_mfma_f32_16x16x32 (bf16, or f16 in the HCB_F16 build) with the OUTPUT PIXEL as K: A = 16
//                         dz channels, B = 16 input channels. Both operands are pixel-major in LDS and are read K-major
//                         with ds_read_b64_tr_b16; for the patch each lane supplies the address of its own tap pixel
//                         (p s + r, q s + t), so stride 2 and the row wrap are address patterns. Pixels past the
//                         strip's end (partial last K block) are clamped into the strip and meet zero dz rows.
//                         fp32: six products per fragment pair, small terms first, as conv_p3 orders them.
// Both LDS buffers (patch + dz) are doubled: strip i + 1 is loaded before the MFMAs of strip i, transformed and stored
// after them, one barrier per strip. Where the doubled buffers of even a one-row strip miss the 160 KiB (no model
// shape) the plan single-buffers. LDS-DMA is not usable: the data changes on its way.
//
// After its slab the workgroup adds the K-split waves' tiles through LDS in kh order and stores the chunk's
// [Nout][9][32] partial into the caller's workspace [slabs][Nout][9][C32]. wgrad_fold_kernel (patch3x3.h) sums the slabs in a
// fixed order and does the single dw += per element. No atomics, no memset, no reliance on zeroed memory: every
// workspace element that is read was written by the launch before. Bitwise reproducible in every mode.
// Slab rule (a function of the shape alone, not of the dtype or device): as many slabs as keep
//   partial floats written <= (operand elements read) / 2     (16-bit: partial bytes <= operand bytes)
// with at least two strips per slab and at most 256 workgroups. The dense kernel's "about 256 workgroups" alone would
// write 9 MiB of partials for the 2 MiB of operands of the 8 x 8 x 64 layer at batch 128 (bf16); this rule gives
// 256 / 128 / 86 / 32 / 2 x 19 workgroups and 4.5 / 4.5 / 3.0 / 2.3 / 2.7 MiB of workspace on the five layers.
// Measured (profiles/resnet_cifar_v2_wgrad.txt): the two 64-column layers, with 32 and 38 workgroups of 4 and 7
// strips each, are the ones that lose against the unfused chain; the rule is the first thing to revisit.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; no scratch and no LDS-DMA in any of the 12
// instantiations of either build; the bf16 and fp16 builds agree), VGPRs + AGPRs by (Nout, halves):
//             16, 1     16, 2     32, 1     32, 2     64, 1     64, 2
//   16-bit:  142 + 36  116 + 36  124 + 36  128 + 36  140 + 36  144 + 72
//   fp32:    198 + 36  170 + 36  182 + 36  186 + 36  207 + 36  209 + 72
//   fold: 14 VGPRs, 1088 bytes of static LDS
// dynamic LDS = nbuf * planes * (patch_pix * 32 NH + round_up(TR * Q, 32) * 2 Nout) bytes, planes = 3 on fp32.
#include <cstdio>
#include <cstdlib>

#include "common.h"
#include "kernels.h"
#define PATCH3X3_WGRAD_FOLD
#include "patch3x3.h"

namespace hcb {

namespace {

constexpr int PW_MAXIT = 8;            // patch vectors (8 channels of one pixel) per thread and strip at most
constexpr int PW_STRIP = 128;          // output pixels of a strip at most
constexpr size_t PW_LDS_MAX = 160 * 1024;
constexpr int PW_TARGET_WGS = 256;

// NRT: row tiles (16 dz channels each), NH: 16-channel halves of the chunk that exist
template <typename T, int NRT, int NH>
__global__ __launch_bounds__(256) void preact_wgrad_kernel(PreactWgradParams p) {
  constexpr bool F32 = sizeof(T) == 4;
  constexpr int NPL = F32 ? 3 : 1;
  constexpr uint32_t E = Act8<T>::ESZ;
  constexpr int U = NRT * NH;            // (row tile, half) units of the chunk
  constexpr int WU = U < 4 ? U : 4;      // waves side by side over the units
  constexpr int KS = 4 / WU;             // waves that split the K blocks of a unit
  constexpr int UPW = U / WU;            // units per wave (2: both halves of one row tile)
  constexpr int NKI = (PW_STRIP / 32) / KS;
  constexpr int VPP = 2 * NH;            // 16-byte vectors per patch pixel
  constexpr uint32_t UB = 16u * VPP;
  constexpr int ZVP = 2 * NRT;           // 16-byte vectors per dz pixel
  constexpr uint32_t ZROW = 32u * NRT;
  constexpr int ZIT = NRT;               // dz vectors per thread: 128 pixels * ZVP / 256
  static_assert(UPW == 1 || (WU == NRT && UPW == NH), "two units per wave share their row tile");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id_uniform();
  const int li = lane & 15, g = lane >> 4, q4 = li >> 2, p4 = li & 3;
  const int ug = wave % WU, kh = wave / WU;
  const int rt = ug % NRT, hf0 = ug / NRT;  // unit j of the wave: row tile rt, half hf0 + j
  const int nchunks = (p.C + 31) >> 5;
  const int chunk = blockIdx.x % nchunks, slab = blockIdx.x / nchunks;
  const int c0 = chunk * 32;
  const int s_beg = slab * p.strips_per_slab, s_end = min(s_beg + p.strips_per_slab, p.nstrips);
  const uint32_t patch_b = (uint32_t)p.patch_pix * UB;
  const uint32_t dz_b = (uint32_t)p.zpix * ZROW;
  const uint32_t buf_b = NPL * (patch_b + dz_b);
  const int s = p.stride;

  const __amdgpu_buffer_rsrc_t xr = make_rsrc(p.x, p.x_bytes);
  const __amdgpu_buffer_rsrc_t zr = make_rsrc(p.dz, p.dz_bytes);

  // ---- the thread's 8 channels (16-byte column v of every unit it stages) and their BN coefficients
  // (c0 + 8 v + 7 < C_in always: C_in = 16 stages two columns, 32 and 64 are whole chunks)
  const int v = tid % VPP;
  const int cc = c0 + v * 8;
  float sc[8], sh[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    sc[e] = p.gamma[cc + e] * p.invstd[cc + e];
    sh[e] = p.beta[cc + e] - p.mean[cc + e] * sc[e];
  }

  // the patch vectors this thread stages: patch row (or far outside: a halo column, a vector past the patch),
  // byte offset relative to image pixel (h0, 0) of the strip's image, and LDS place
  int prow[PW_MAXIT], poff[PW_MAXIT];
  uint32_t plds[PW_MAXIT];
#pragma unroll
  for (int it = 0; it < PW_MAXIT; ++it) {
    const int pp = (it * 256 + tid) / VPP;
    const int r = pp / p.PW, c = pp - r * p.PW;
    const bool in = pp < p.patch_pix;
    const bool ok = in && (unsigned)(c - p.pl) < (unsigned)p.W;
    prow[it] = ok ? r : -0x10000;
    poff[it] = ((r * p.W + c - p.pl) * p.ldx + cc) * (int)E;
    plds[it] = in ? patch_off<VPP>(pp, v) : HCB_OOB;
  }
  // the dz vectors this thread stages: pixel zp of the strip, channels 8 zv .. + 7
  int zpx[ZIT], zoff[ZIT];
  uint32_t zlds[ZIT];
#pragma unroll
  for (int j = 0; j < ZIT; ++j) {
    const int idx = j * 256 + tid;
    const int zp = idx / ZVP, zv = idx - zp * ZVP;
    zpx[j] = zp;
    zoff[j] = (zp * p.ldz + zv * 8) * (int)E;
    zlds[j] = zp < p.zpix ? (uint32_t)zp * ZROW + (uint32_t)(((zv >> 1) ^ (zp & (NRT - 1))) << 5) + (uint32_t)(zv & 1) * 16u
                          : HCB_OOB;
  }
  // this lane's part of the A fragment of K block 0, plane 0: pixel 8 g + q4 (and + 4), dz channels 16 rt + 4 p4 .. + 3
  const uint32_t aaddr = (uint32_t)(8 * g + q4) * ZROW + (uint32_t)((rt ^ (q4 & (NRT - 1))) << 5) + (uint32_t)p4 * 8u;
  const uint32_t bsub = (uint32_t)(p4 & 1) * 8u;

  f32x4 acc[UPW][9];
#pragma unroll
  for (int j = 0; j < UPW; ++j)
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  Act8<T> xv[PW_MAXIT], zv[ZIT];
  uint32_t okmask = 0;
  auto gload = [&](int strip) {
    const int n = strip / p.strips_per_img;
    const int r0 = (strip - n * p.strips_per_img) * p.TR;  // first output row
    const int npix = min(p.TR, p.P - r0) * p.Q;
    const int h0 = r0 * s - p.pt;                           // image row of patch row 0
    const int base = (n * p.H + h0) * p.W * p.ldx * (int)E;
    const int m0 = (n * p.P + r0) * p.Q;
    okmask = 0;
#pragma unroll
    for (int it = 0; it < PW_MAXIT; ++it) {
      if (it >= p.nit) continue;  // (uniform)
      const bool ok = (unsigned)(h0 + prow[it]) < (unsigned)p.H;
      okmask |= (uint32_t)ok << it;
      xv[it].load(xr, ok ? (uint32_t)(base + poff[it]) : HCB_OOB);
    }
#pragma unroll
    for (int j = 0; j < ZIT; ++j) zv[j].load(zr, zpx[j] < npix ? (uint32_t)(m0 * p.ldz * (int)E + zoff[j]) : HCB_OOB);
  };
  auto lstore = [&](int b) {
    char* pb = smem + (size_t)b * buf_b;
    char* zb = pb + NPL * patch_b;
#pragma unroll
    for (int it = 0; it < PW_MAXIT; ++it) {
      if (it >= p.nit || plds[it] == HCB_OOB) continue;
      bnrelu_store<T>(pb, patch_b, plds[it], xv[it], (okmask >> it) & 1u, sc, sh);
    }
#pragma unroll
    for (int j = 0; j < ZIT; ++j) {
      if (zlds[j] == HCB_OOB) continue;
      if constexpr (F32) {
        u32x4 hi, mid, lo;
        split3_8(zv[j].a, zv[j].b, hi, mid, lo);
        *reinterpret_cast<u32x4*>(zb + zlds[j]) = hi;
        *reinterpret_cast<u32x4*>(zb + dz_b + zlds[j]) = mid;
        *reinterpret_cast<u32x4*>(zb + 2 * dz_b + zlds[j]) = lo;
      } else {
        *reinterpret_cast<u32x4*>(zb + zlds[j]) = zv[j].v;
      }
    }
  };

  const bool dbl = p.nbuf == 2;
  gload(s_beg);  // (no slab is empty: the plan)
  lstore(0);
  __syncthreads();
  for (int strip = s_beg; strip < s_end; ++strip) {
    const bool more = strip + 1 < s_end;
    if (more) gload(strip + 1);
    {
      const int n = strip / p.strips_per_img;
      const int r0 = (strip - n * p.strips_per_img) * p.TR;
      const int npix = min(p.TR, p.P - r0) * p.Q;
      const int nkb = (npix + 31) >> 5;
      const char* pb = smem + (dbl ? (size_t)((strip - s_beg) & 1) * buf_b : 0);
      const char* zb = pb + NPL * patch_b;
#pragma unroll
      for (int ki = 0; ki < NKI; ++ki) {
        const int kb = kh + KS * ki;
        if (kb >= nkb) continue;  // (wave-uniform)
        u32x4 a[NPL];
#pragma unroll
        for (int t = 0; t < NPL; ++t) {
          const char* ap = zb + t * dz_b + kb * (32 * ZROW) + aaddr;
          a[t] = frag_tr16(ap, ap + 4 * ZROW);
        }
        // the patch units of this lane's two pixels at tap (0, 0); pixels past the strip clamp into it
        int unit[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int o = min(kb * 32 + 8 * g + 4 * h + q4, npix - 1);
          const int orow = o / p.Q;
          unit[h] = orow * s * p.PW + (o - orow * p.Q) * s;
        }
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          const int d = (tap / 3) * p.PW + tap % 3;
#pragma unroll
          for (int j = 0; j < UPW; ++j) {
            const int bcol = (hf0 + j) * 2 + (p4 >> 1);
            const uint32_t o0 = patch_off<VPP>(unit[0] + d, bcol) + bsub, o1 = patch_off<VPP>(unit[1] + d, bcol) + bsub;
            u32x4 bb[NPL];
#pragma unroll
            for (int t = 0; t < NPL; ++t) bb[t] = frag_tr16(pb + t * patch_b + o0, pb + t * patch_b + o1);
            mfma_acc<F32>(a, bb, acc[j][tap]);
          }
        }
      }
    }
    if (more) {
      if (!dbl) __syncthreads();  // one buffer: every wave is done reading it
      lstore(dbl ? (strip + 1 - s_beg) & 1 : 0);
    }
    __syncthreads();
  }

  // ---- K-split waves: the kh >= 1 tiles -> LDS -> added to the kh = 0 tiles in kh order (every wave is past the
  // loop's last barrier)
  if constexpr (KS > 1) {
    f32x4* red = reinterpret_cast<f32x4*>(smem);
    if (kh > 0) {
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) red[(((kh - 1) * WU + ug) * 9 + tap) * 64 + lane] = acc[0][tap];
    }
    __syncthreads();
    if (kh > 0) return;  // (wave-uniform)
#pragma unroll
    for (int k = 1; k < KS; ++k)
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const f32x4 o = red[(((k - 1) * WU + ug) * 9 + tap) * 64 + lane];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[0][tap][e] += o[e];
      }
  }
  // lane: dz channels 16 rt + 4 g .. + 3 (rows), input channel c0 + 16 hf + li
  const int C32 = nchunks * 32;
#pragma unroll
  for (int j = 0; j < UPW; ++j) {
    float* dst = p.ws + ((size_t)slab * p.Nout + rt * 16 + g * 4) * 9 * C32 + c0 + (hf0 + j) * 16 + li;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int e = 0; e < 4; ++e) dst[((size_t)e * 9 + tap) * C32] = acc[j][tap][e];
  }
}

template <typename T, int NRT>
void pw_launch_h(const PreactWgradParams& p, dim3 grid, size_t lds, hipStream_t st) {
  if (p.C == 16)
    launch_big_lds(preact_wgrad_kernel<T, NRT, 1>, grid, lds, st, p, "preact_conv3x3_wgrad");
  else
    launch_big_lds(preact_wgrad_kernel<T, NRT, 2>, grid, lds, st, p, "preact_conv3x3_wgrad");
}

template <typename T>
void pw_launch_t(const PreactWgradParams& p, dim3 grid, size_t lds, hipStream_t st) {
  if (p.Nout == 16)
    pw_launch_h<T, 1>(p, grid, lds, st);
  else if (p.Nout == 32)
    pw_launch_h<T, 2>(p, grid, lds, st);
  else
    pw_launch_h<T, 4>(p, grid, lds, st);
}

}  // namespace

bool preact_conv3x3_wgrad_plan(int N, int H, int W, int C, int Nout, int s, bool f32, PreactWgradPlan* out) {
  if (!(C == 16 || C == 32 || C == 64) || !(Nout == 16 || Nout == 32 || Nout == 64) || !(s == 1 || s == 2)) return false;
  if (N < 1 || H < 1 || W < 1) return false;
  PreactWgradPlan pl{};
  same3(H, s, &pl.P, &pl.pt);
  same3(W, s, &pl.Q, &pl.pl);
  if (pl.Q > PW_STRIP) return false;
  const int vpp = C == 16 ? 2 : 4, nrt = Nout / 16, nchunks = (C + 31) / 32;
  const int u = nrt * (vpp / 2), wu = u < 4 ? u : 4, ks = 4 / wu;
  const size_t red = (size_t)(ks - 1) * wu * 9 * 1024;  // the K-split waves' tiles on their way to the kh = 0 waves
  pl.PW = (pl.Q - 1) * s + 3;
  for (int nbuf = 2; nbuf >= 1; --nbuf) {
    int TR = PW_STRIP / pl.Q;
    if (TR > pl.P) TR = pl.P;
    for (; TR >= 1; --TR) {
      const int pix = ((TR - 1) * s + 3) * pl.PW;
      const int zpix = (TR * pl.Q + 31) & ~31;
      size_t lds = (size_t)nbuf * (f32 ? 3 : 1) * ((size_t)pix * 16 * vpp + (size_t)zpix * 32 * nrt);
      if (lds < red) lds = red;
      if (pix * vpp > PW_MAXIT * 256 || lds > PW_LDS_MAX) continue;
      pl.TR = TR;
      pl.patch_pix = pix;
      pl.nit = (pix * vpp + 255) / 256;
      pl.zpix = zpix;
      pl.nbuf = nbuf;
      pl.strips_per_img = (pl.P + TR - 1) / TR;
      pl.nstrips = N * pl.strips_per_img;
      // slabs: partial floats written <= operand elements read / 2, >= 2 strips per slab, <= 256 workgroups
      const int64_t part = (int64_t)Nout * 9 * nchunks * 32;
      const int64_t oper = (int64_t)N * H * W * C + (int64_t)nchunks * N * pl.P * pl.Q * Nout;
      int64_t slabs = oper / (2 * part);
      if (slabs > PW_TARGET_WGS / nchunks) slabs = PW_TARGET_WGS / nchunks;
      if (slabs > pl.nstrips / 2) slabs = pl.nstrips / 2;
      if (slabs < 1) slabs = 1;
      pl.strips_per_slab = (int)((pl.nstrips + slabs - 1) / slabs);
      pl.nslabs = (pl.nstrips + pl.strips_per_slab - 1) / pl.strips_per_slab;  // no empty slab
      pl.lds_bytes = lds;
      pl.ws_floats = (int64_t)pl.nslabs * part;
      *out = pl;
      return true;
    }
  }
  return false;
}

void launch_preact_conv3x3_wgrad(const PreactWgradParams& p0, hipStream_t st, bool f32) {
  PreactWgradParams p = p0;
  PreactWgradPlan pl;
  if (!preact_conv3x3_wgrad_plan(p.N, p.H, p.W, p.C, p.Nout, p.stride, f32, &pl)) {  // (the binding refuses it by name first)
    fprintf(stderr, "hcb preact_conv3x3_wgrad: %d x %d x %d -> %d, stride %d does not fit\n", p.H, p.W, p.C, p.Nout, p.stride);
    abort();
  }
  p.P = pl.P; p.Q = pl.Q; p.pt = pl.pt; p.pl = pl.pl; p.TR = pl.TR; p.PW = pl.PW; p.patch_pix = pl.patch_pix;
  p.nit = pl.nit; p.zpix = pl.zpix; p.nbuf = pl.nbuf; p.strips_per_img = pl.strips_per_img; p.nstrips = pl.nstrips;
  p.strips_per_slab = pl.strips_per_slab; p.nslabs = pl.nslabs;
  const dim3 grid((unsigned)(((p.C + 31) / 32) * pl.nslabs));
  if (f32)
    pw_launch_t<float>(p, grid, pl.lds_bytes, st);
  else
    pw_launch_t<uint16_t>(p, grid, pl.lds_bytes, st);
  const int total = p.Nout * 9 * p.C;
  hipLaunchKernelGGL(wgrad_fold_kernel, dim3((unsigned)((total + 15) / 16)), dim3(256), 0, st, p.ws, p.dw, p.C, p.ldw,
                     p.nslabs, p.Nout, p.Nout);
}

}  // namespace hcb
