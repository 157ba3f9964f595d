// Weight gradient of the DenseNet dense layer on gfx950, with BatchNorm and ReLU applied on the way in:
//   dw[n][r][s][c] += sum_{img, oh, ow} dz[img][oh][ow][n] * a[img][oh + r - 1][ow + s - 1][c]
//   a = relu(x * sc + sh),  sc = gamma * invstd,  sh = beta - mean * sc,  a = 0 outside the image
// x = channels [0, C) of the raw concat buffer, dz = the layer's 16-channel slot of the block's gradient
// buffer, mean / invstd the statistics the forward kernel (dense3x3.hip) published. The normalised operand
// is never written: the unfused chain (BN apply writes it for all C channels, conv_wgrad reads it back
// through a GEMM tiled for wide outputs) moves the layer's input three times, this kernel once.
//
// Work split: the reduction runs over all N * H * W pixels, so the grid is (32-channel chunks) x (pixel
// slabs). A workgroup of 4 waves owns ONE chunk and walks the strips of its slab; a strip is TR whole
// rows of one image (TR * W <= 128 pixels = at most 4 MFMA K blocks of 32 pixels). Per strip:
//   global -> registers   the chunk's input patch, (TR + 2) x (W + 2) pixels x 32 channels, 16-byte raw
//                         buffer loads (pixels outside the image and channels past C: the out-of-range
//                         offset), and the strip of dz, 128 pixels x 16 channels, one 8-channel vector
//                         per thread (pixels past the strip's end out of range: zeros).
//   registers -> LDS      BN + ReLU in fp32 in the forward's fmaxf(f * sc + sh, 0.f) form (the thread's 8
//                         channels never change: their sc / sh live in registers), halo pixels SELECTED
//                         to zero; then 16-bit, or on the fp32 path the bf16 hi / mid / lo split into
//                         three tiles (patch3x3.h: the shared unit, swizzle and patch store). dz takes the
//                         same split in registers; dz rows are 32 bytes (16 channels of one pixel), unswizzled.
//   LDS -> MFMA           v_mfma_f32_16x16x32 (bf16, or f16 in the HCB_F16 build) with the PIXEL index as
//                         K: A = 16 dz channels, B = 16 input channels. Both operands are pixel-major in
//                         LDS and are read K-major with the transposed read ds_read_b64_tr_b16: a lane
//                         supplies the address of pixel 8g + 4h + (li >> 2), channels 4 * (li & 3) .. + 3,
//                         and receives channel li of four consecutive pixels. For the patch the lane's
//                         address is that of the TAP's pixel (oh + r, ow + s) of the patch, so the row wrap
//                         of the strip inside the (W + 2)-wide patch is absorbed by the per-lane address;
//                         pixels past the strip's end (partial last K block) are clamped into the strip
//                         and meet zero dz rows. One accumulator tile per tap and 16-channel half.
//                         fp32: six products per fragment pair, small terms first, as conv_p3 orders them.
// Waves: wave = 2 * kh + hf owns the 9 tap tiles of channel half hf (36 accumulator registers) and the K
// blocks kh, kh + 2 of every strip, so the A fragment of a K block is read once per wave and serves nine
// taps. Both LDS buffers (patch + dz) are doubled: the loads of strip s + 1 are issued before the MFMAs
// of strip s, transformed and stored after them; one barrier per strip. LDS-DMA is not usable, the data
// changes on its way.
//
// After its slab the workgroup adds the kh = 1 waves' tiles to the kh = 0 waves' through LDS (fixed
// order) and stores the chunk's [16][9][32] partial into the caller's workspace [slabs][16][9][C32].
// wgrad_fold_kernel (patch3x3.h) then sums the slabs in a fixed order (16 interleaved slab sequences per element,
// each in slab order, added in sequence order) and does the single dw += per element of
// rows 0 .. Nout - 1; rows Nout..15 receive nothing. No atomics, no memset, no reliance on zeroed memory:
// every workspace element that is read was written by the launch before. The result is bitwise
// reproducible in every mode (deterministic mode changes nothing). The slab count is a function of the
// problem alone: about 256 workgroups, at least two strips per slab where the problem has them; the
// workspace then stays below 6 MiB at any C.
//
// Resources (hipcc -O3, gfx950; no scratch in either build or form):
//   16-bit: 90 VGPRs + 36 AGPRs (bf16 and fp16 builds), dynamic LDS = 2 * (patch_pix * 64 + 4096) bytes (>= 18 KiB)
//   fp32:   136 VGPRs + 36 AGPRs (both builds), dynamic LDS = 6 * (patch_pix * 64 + 4096) bytes (three tiles of each)
//   fold:   14 VGPRs, 1088 bytes of static LDS (the shared wgrad_fold_kernel)
// with patch_pix = (TR + 2) * (W + 2) <= 320 and TR = min(128 / W, 16, H) (8 x 8 maps: whole images, so that
// all four waves have a K block; 16 x 16: 8 rows; 32 x 32: 4 rows, 34 KiB / 101 KiB).
#include <cstdio>
#include <cstdlib>

#include "common.h"
#include "kernels.h"
#define PATCH3X3_WGRAD_FOLD
#include "patch3x3.h"

namespace hcb {

namespace {

constexpr int DW_MAXIT = 5;            // patch vectors (8 channels of one pixel) per thread and strip
constexpr int DW_STRIP = 128;          // pixels of a strip at most: one dz vector per thread
constexpr uint32_t DW_DZB = DW_STRIP * 32u;
constexpr uint32_t DW_RED_BYTES = 18 * 64 * 16;  // the kh = 1 waves' tiles on their way to the kh = 0 waves
constexpr size_t DW_LDS_MAX = 160 * 1024;
constexpr int DW_TARGET_WGS = 256;

template <typename T>
__global__ __launch_bounds__(256) void dense_wgrad_kernel(DenseWgradParams p) {
  constexpr bool F32 = sizeof(T) == 4;
  constexpr int NPL = F32 ? 3 : 1;
  constexpr uint32_t E = Act8<T>::ESZ;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id_uniform();
  const int li = lane & 15, g = lane >> 4, q4 = li >> 2, p4 = li & 3;
  const int hf = wave & 1, kh = wave >> 1;
  const int nchunks = (p.C + 31) >> 5;
  const int chunk = blockIdx.x % nchunks, slab = blockIdx.x / nchunks;
  const int c0 = chunk * 32;
  const bool live = c0 + hf * 16 < p.C;  // a half past C (C % 32 <= 16) multiplies nothing: its tiles stay zero
  const int s_beg = slab * p.strips_per_slab, s_end = min(s_beg + p.strips_per_slab, p.nstrips);
  const uint32_t patch_b = (uint32_t)p.patch_pix * 64u;
  const uint32_t buf_b = NPL * (patch_b + DW_DZB);
  const int W2 = p.W + 2;

  const __amdgpu_buffer_rsrc_t xr = make_rsrc(p.x, p.x_bytes);
  const __amdgpu_buffer_rsrc_t zr = make_rsrc(p.dz, p.dz_bytes);

  // ---- the thread's 8 channels (16-byte column v of every unit it stages) and their BN coefficients
  const int v = tid & 3;
  const int cc = c0 + v * 8;
  const bool cok = cc < p.C;  // (C % 8 == 0: a vector lies wholly inside or outside)
  float sc[8], sh[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    sc[e] = sh[e] = 0.f;
    if (cok) {
      sc[e] = p.gamma[cc + e] * p.invstd[cc + e];
      sh[e] = p.beta[cc + e] - p.mean[cc + e] * sc[e];
    }
  }

  // the patch vectors this thread stages: patch row, byte offset relative to the strip's first pixel
  // (or out of range: a halo column, a channel past C, a vector past the patch) and LDS place
  int prow[DW_MAXIT], poff[DW_MAXIT];
  uint32_t plds[DW_MAXIT];
#pragma unroll
  for (int it = 0; it < DW_MAXIT; ++it) {
    const int pp = (it * 256 + tid) >> 2;
    const int r = pp / W2, c = pp - r * W2;
    const bool in = pp < p.patch_pix;
    const bool ok = in && cok && (unsigned)(c - 1) < (unsigned)p.W;
    prow[it] = ok ? r - 1 : -0x10000;  // (far outside every image)
    poff[it] = (((r - 1) * p.W + c - 1) * p.ldx + cc) * (int)E;
    plds[it] = in ? patch_off(pp, v) : HCB_OOB;
  }
  // the dz vector this thread stages: pixel tid >> 1 of the strip, channels 8 * (tid & 1) .. + 7
  const int zpix = tid >> 1;
  const int zoff = (zpix * p.ldz + (tid & 1) * 8) * (int)E;
  const uint32_t zlds = (uint32_t)tid * 16u;
  // this lane's part of the A fragment of K block 0, plane 0 (K block kb: + kb * 1024)
  const uint32_t aaddr = (uint32_t)((8 * g + q4) * 32 + p4 * 8);
  const int bcol = hf * 2 + (p4 >> 1);
  const uint32_t bsub = (uint32_t)(p4 & 1) * 8u;

  f32x4 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  Act8<T> xv[DW_MAXIT], zv;
  uint32_t okmask = 0;
  auto gload = [&](int strip) {
    const int n = strip / p.strips_per_img;
    const int h0 = (strip - n * p.strips_per_img) * p.TR;
    const int npix = min(p.TR, p.H - h0) * p.W;
    const int m0 = (n * p.H + h0) * p.W;
    const int base = m0 * p.ldx * (int)E;
    okmask = 0;
#pragma unroll
    for (int it = 0; it < DW_MAXIT; ++it) {
      const bool ok = (unsigned)(h0 + prow[it]) < (unsigned)p.H;
      okmask |= (uint32_t)ok << it;
      xv[it].load(xr, ok ? (uint32_t)(base + poff[it]) : HCB_OOB);
    }
    zv.load(zr, zpix < npix ? (uint32_t)(m0 * p.ldz * (int)E + zoff) : HCB_OOB);
  };
  auto lstore = [&](int b) {
    char* pb = smem + (size_t)b * buf_b;
    char* zb = pb + NPL * patch_b;
#pragma unroll
    for (int it = 0; it < DW_MAXIT; ++it)
      if (plds[it] != HCB_OOB) bnrelu_store<T>(pb, patch_b, plds[it], xv[it], (okmask >> it) & 1u, sc, sh);
    if constexpr (F32) {
      u32x4 hi, mid, lo;
      split3_8(zv.a, zv.b, hi, mid, lo);
      *reinterpret_cast<u32x4*>(zb + zlds) = hi;
      *reinterpret_cast<u32x4*>(zb + DW_DZB + zlds) = mid;
      *reinterpret_cast<u32x4*>(zb + 2 * DW_DZB + zlds) = lo;
    } else {
      *reinterpret_cast<u32x4*>(zb + zlds) = zv.v;
    }
  };

  if (s_beg < s_end) {
    gload(s_beg);
    lstore(0);
  }
  __syncthreads();
  for (int strip = s_beg; strip < s_end; ++strip) {
    const bool more = strip + 1 < s_end;
    if (more) gload(strip + 1);
    {
      const int n = strip / p.strips_per_img;
      const int h0 = (strip - n * p.strips_per_img) * p.TR;
      const int npix = min(p.TR, p.H - h0) * p.W;
      const int nkb = (npix + 31) >> 5;
      const char* pb = smem + (size_t)((strip - s_beg) & 1) * buf_b;
      const char* zb = pb + NPL * patch_b;
#pragma unroll
      for (int ki = 0; ki < 2; ++ki) {
        const int kb = kh + 2 * ki;
        if (kb >= nkb || !live) continue;  // (wave-uniform)
        u32x4 a[NPL];
#pragma unroll
        for (int t = 0; t < NPL; ++t) {
          const char* ap = zb + t * DW_DZB + kb * 1024 + aaddr;
          a[t] = frag_tr16(ap, ap + 128);
        }
        // the patch units of this lane's two pixels at tap (0, 0); pixels past the strip clamp into it
        int unit[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int o = min(kb * 32 + 8 * g + 4 * h + q4, npix - 1);
          const int orow = o / p.W;
          unit[h] = orow * W2 + (o - orow * p.W);
        }
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          const int d = (tap / 3) * W2 + tap % 3;
          const uint32_t o0 = patch_off(unit[0] + d, bcol) + bsub, o1 = patch_off(unit[1] + d, bcol) + bsub;
          u32x4 bb[NPL];
#pragma unroll
          for (int t = 0; t < NPL; ++t) bb[t] = frag_tr16(pb + t * patch_b + o0, pb + t * patch_b + o1);
          mfma_acc<F32>(a, bb, acc[tap]);
        }
      }
    }
    if (more) lstore((strip + 1 - s_beg) & 1);
    __syncthreads();
  }

  // ---- kh = 1 tiles -> LDS -> added to the kh = 0 tiles (every wave is past the loop's last barrier)
  f32x4* red = reinterpret_cast<f32x4*>(smem);
  if (kh == 1) {
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) red[(hf * 9 + tap) * 64 + lane] = acc[tap];
  }
  __syncthreads();
  if (kh == 1) return;  // (wave-uniform)
  // lane: dz channels 4 g .. + 3 (rows), input channel c0 + 16 hf + li
  const int C32 = nchunks * 32;
  float* dst = p.ws + ((size_t)slab * 16 + g * 4) * 9 * C32 + c0 + hf * 16 + li;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const f32x4 o = red[(hf * 9 + tap) * 64 + lane];
#pragma unroll
    for (int e = 0; e < 4; ++e) dst[((size_t)e * 9 + tap) * C32] = acc[tap][e] + o[e];
  }
}

}  // namespace

bool dense_conv3x3_wgrad_plan(int N, int H, int W, int C, bool f32, DenseWgradPlan* out) {
  if (N < 1 || H < 1 || W < 1 || C < 1 || W > DW_STRIP) return false;
  int TR = DW_STRIP / W;
  if (TR > 16) TR = 16;
  if (TR > H) TR = H;
  for (; TR >= 1; --TR) {
    const int pix = (TR + 2) * (W + 2);
    size_t lds = 2 * (size_t)(f32 ? 3 : 1) * ((size_t)pix * 64 + DW_DZB);
    if (lds < DW_RED_BYTES) lds = DW_RED_BYTES;
    if (pix * 4 > DW_MAXIT * 256 || lds > DW_LDS_MAX) continue;
    const int nchunks = (C + 31) / 32;
    const int spi = (H + TR - 1) / TR;
    const int nstrips = N * spi;
    int slabs = (DW_TARGET_WGS + nchunks - 1) / nchunks;
    if (slabs > nstrips / 2) slabs = nstrips / 2;
    if (slabs < 1) slabs = 1;
    const int sps = (nstrips + slabs - 1) / slabs;
    slabs = (nstrips + sps - 1) / sps;  // no empty slab
    out->TR = TR;
    out->patch_pix = pix;
    out->strips_per_img = spi;
    out->nstrips = nstrips;
    out->strips_per_slab = sps;
    out->nslabs = slabs;
    out->lds_bytes = lds;
    out->ws_floats = (int64_t)slabs * 16 * 9 * nchunks * 32;
    return true;
  }
  return false;
}

void launch_dense_conv3x3_wgrad(const DenseWgradParams& p0, hipStream_t st, bool f32) {
  DenseWgradParams p = p0;
  DenseWgradPlan pl;
  if (!dense_conv3x3_wgrad_plan(p.N, p.H, p.W, p.C, f32, &pl)) {  // (the binding refuses it by name first)
    fprintf(stderr, "hcb dense_conv3x3_wgrad: W = %d does not fit the LDS budget\n", p.W);
    abort();
  }
  p.TR = pl.TR;
  p.patch_pix = pl.patch_pix;
  p.strips_per_img = pl.strips_per_img;
  p.nstrips = pl.nstrips;
  p.strips_per_slab = pl.strips_per_slab;
  p.nslabs = pl.nslabs;
  const dim3 grid((unsigned)(((p.C + 31) / 32) * pl.nslabs));
  if (f32)
    launch_big_lds(dense_wgrad_kernel<float>, grid, pl.lds_bytes, st, p, "dense_conv3x3_wgrad");
  else
    launch_big_lds(dense_wgrad_kernel<uint16_t>, grid, pl.lds_bytes, st, p, "dense_conv3x3_wgrad");
  // the workspace has 16 rows per slab; rows Nout..15 of dw receive nothing
  const int total = p.Nout * 9 * p.C;
  hipLaunchKernelGGL(wgrad_fold_kernel, dim3((unsigned)((total + 15) / 16)), dim3(256), 0, st, p.ws, p.dw, p.C, p.ldw,
                     p.nslabs, 16, p.Nout);
}

}  // namespace hcb
