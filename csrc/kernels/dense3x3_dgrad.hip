// Data gradient of the DenseNet dense layer on gfx950, with the ReLU and BatchNorm backward applied to it
// before it ever reaches memory:
//   da[i][h][v][c] = sum_{r, s, n < Nout} dz[i][h + 1 - r][v + 1 - s][n] * w[n][r][s][c]     (dz = 0 outside the image)
//   g = da where x * sc + sh > 0, else 0        sc = gamma * invstd,  sh = beta - mean * sc
//   dbeta[c] = sum_pixels g      dgamma[c] = sum_pixels g * xhat,   xhat = (x - mean) * invstd
//   gin[i][h][v][c] += sc[c] * (g - dbeta[c] / M - xhat * dgamma[c] / M)
// x = channels [0, C) of the raw concat buffer, dz = the layer's 16-channel slot of the block's gradient
// buffer, gin = channels [0, C) of that same gradient buffer (the slot lies at or beyond C: the binding
// checks that the bytes are disjoint, so halo pixels of dz may be read while other workgroups update gin),
// w the fp32 master kernel [16][3][3][C]. da is never stored: the unfused chain (the data-gradient GEMM writes
// it, bn_bwd_reduce_acc reads it and x, bn_bwd_apply_acc reads it, x and gin again) makes seven passes over
// [N, H, W, C] tensors, this file four (x twice, gin read and written). The product itself has K = 144.
//
// Three launches: REDUCE, fold, APPLY. REDUCE and APPLY are one template and compute da with the same
// instruction sequence, so the mask and the values of the two passes are bitwise the same.
//
// Work split (as dense3x3_wgrad.hip): grid = (32-channel chunks) x (pixel slabs); a workgroup of 4 waves owns
// ONE chunk and walks the strips of its slab; a strip is TR whole rows of one image, TR * W <= 128 pixels =
// 8 MFMA tiles of 16 pixels. Wave w owns tiles w and w + 4 and both 16-channel halves of the chunk: four
// accumulator tiles.
//   weights   once per workgroup: the chunk's slice 9 taps x 16 n x 32 c of the fp32 master (rows >= Nout and
//             channels >= C read as zeros) is converted to 16-bit -- or split into bf16 hi / mid / lo planes on
//             the fp32 path -- and kept in LDS as [tap][c][n], 32-byte rows, for the whole slab. A tenth,
//             all-zero tap fills the second half of the last K block. No weight pack is needed.
//   dz patch  per strip: (TR + 2) x (W + 2) pixels x 16 channels, 32-byte rows, 16-byte raw buffer loads (halo
//             pixels and pixels outside the image: the out-of-range offset, zeros); fp32: split into three
//             planes on the way into LDS. Double-buffered: the loads of strip s + 1 are issued before the
//             MFMAs of strip s and stored after its epilogue; one barrier per strip.
//   MFMA      v_mfma_f32_16x16x32 (bf16, or f16 in the HCB_F16 build). K block = a pair of taps x 16 dz
//             channels: lanes 0..31 supply tap 2 kb, lanes 32..63 tap 2 kb + 1; nine taps = five K blocks. A =
//             weights with the chunk's channels as rows (a 16-byte read of one [tap][c] row), B = 16 pixels: the
//             lane's 16-byte read goes to the address of ITS pixel shifted by ITS tap inside the patch, so the
//             row wrap of the strip inside the (W + 2)-wide patch is absorbed by the per-lane address. A lane
//             ends with 4 consecutive channels of one pixel, the forward kernel's store shape. fp32: six
//             products per fragment pair, small terms first (patch3x3.h: mfma_acc, shared with the family).
//   epilogue  x (and gin on APPLY) of the lane's 4 channels x 4 tiles are loaded straight into registers
//             before the MFMAs (8 or 16 bytes per access; the 4 lanes of a pixel cover 32 or 64 contiguous
//             bytes per half); sc, sh, mean, invstd of the lane's 8 channels live in registers.
//             REDUCE: sum g and sum g * xhat per lane over the slab, then across the 16 lanes of a channel
//             group by shuffles, across the waves through LDS in wave order; the chunk's [2][32] partial goes
//             into the caller's workspace [slabs][2][C32].
//             APPLY: the gin update, one 8- or 16-byte store per lane and tile.
// dense_dgrad_fold_kernel sums the slabs in a fixed order (16 interleaved slab sequences per element, each in
// slab order, added in sequence order) and OVERWRITES dbeta / dgamma, which APPLY then reads.
//
// No atomics, no memset, no reliance on zeroed memory: every workspace element that is read was written by
// the launch before. The result is bitwise reproducible in every mode (deterministic mode changes nothing).
// The slab count is a function of the problem alone: about 256 workgroups, at least two strips per slab
// where the problem has them. Pad channels (gamma = beta = 0, x = 0) have sc = sh = 0: the mask is false, g,
// dbeta and dgamma are exact zeros and gin receives + 0.
//
// Deviations from the first design: the weight fragments are re-read from LDS per strip (10 reads per wave
// beside the 10 patch reads) instead of living in registers (120 VGPRs on the fp32 path); x goes straight to
// registers, not through LDS; the chunk is 32 channels -- none of these was measured against its alternative.
// A target of 1024 workgroups instead of 256 was measured (profiles/densenet_dgrad.txt): mixed per layer, no
// change of the picture, so the target stays at the weight gradient's 256.
//
// Resources (hipcc -O3, gfx950, bf16 and fp16 builds alike; no scratch in either build or form):
//   16-bit: reduce 136 VGPRs + 16 AGPRs, apply 152 + 16, dynamic LDS = 11264 + 2 * patch_pix * 32 bytes
//   fp32:   reduce 176 VGPRs + 16 AGPRs, apply 192 + 16, dynamic LDS = 31744 + 6 * patch_pix * 32 bytes
//   fold:   16 VGPRs, 1088 bytes of static LDS
// with patch_pix = (TR + 2) * (W + 2) <= 390 and TR = min(128 / W, 16, H) (8 x 8 maps: whole images; 16 x 16: 8
// rows; 32 x 32: 4 rows, 24 KiB / 70 KiB).
#include <cstdio>
#include <cstdlib>

#include "common.h"
#include "kernels.h"
#include "patch3x3.h"

namespace hcb {

namespace {

constexpr int DG_MAXIT = 4;    // dz vectors (8 channels of one pixel) per thread and strip: patch_pix * 2 <= 4 * 256
constexpr int DG_STRIP = 128;  // pixels of a strip at most: 2 MFMA tiles per wave
constexpr int DG_TAPS = 10;    // nine taps and the zero tap that completes the fifth K block
constexpr uint32_t DG_WB = DG_TAPS * 32 * 32u;  // one plane of the chunk's weights: [tap][c] rows of 32 bytes
constexpr int DG_WVEC = DG_TAPS * 32 * 2;       // its 16-byte vectors
constexpr int DG_WIT = (DG_WVEC + 255) / 256;
constexpr uint32_t DG_RED_BYTES = 4 * 2 * 32 * 4;  // the waves' [2][32] sums on their way to the workspace
constexpr size_t DG_LDS_MAX = 160 * 1024;
constexpr int DG_TARGET_WGS = 256;

template <typename T, bool APPLY>
__global__ __launch_bounds__(256) void dense_dgrad_kernel(DenseDgradParams p) {
  constexpr bool F32 = sizeof(T) == 4;
  constexpr int NPL = F32 ? 3 : 1;
  constexpr uint32_t E = Act8<T>::ESZ;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id_uniform();
  const int frow = lane & 15, fq = lane >> 4;
  const int nchunks = (p.C + 31) >> 5;
  const int chunk = blockIdx.x % nchunks, slab = blockIdx.x / nchunks;
  const int c0 = chunk * 32;
  const int s_beg = slab * p.strips_per_slab, s_end = min(s_beg + p.strips_per_slab, p.nstrips);
  const uint32_t patch_b = (uint32_t)p.patch_pix * 32u;
  const uint32_t buf_b = NPL * patch_b;
  char* wl = smem;                                                  // [NPL][tap][c][n]
  float* red = reinterpret_cast<float*>(smem + NPL * DG_WB);        // [4 waves][2][32]
  char* bufs = smem + NPL * DG_WB + DG_RED_BYTES;                   // [2][NPL][patch_pix][16]
  const int W2 = p.W + 2;
  const __amdgpu_buffer_rsrc_t zr = make_rsrc(p.dz, p.dz_bytes);

  // ---- the chunk's weights: fp32 master -> 16-bit (or three planes) -> LDS [tap][c][n]. Consecutive threads
  // take consecutive channels, so each of a vector's 8 loads (8 rows n of the master) is coalesced
#pragma unroll
  for (int it = 0; it < DG_WIT; ++it) {
    const int vi = it * 256 + tid;
    if (vi >= DG_WVEC) continue;
    const int c = vi & 31, nh = (vi >> 5) & 1, tap = vi >> 6;
    float f[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int n = nh * 8 + e;
      const bool ok = tap < 9 && n < p.Nout && c0 + c < p.C;
      f[e] = ok ? p.w[(size_t)n * p.ldw + tap * p.C + c0 + c] : 0.f;
    }
    const uint32_t off = (uint32_t)(tap * 32 + c) * 32u + (uint32_t)nh * 16u;
    if constexpr (F32) {
      u32x4 a, bq, hi, mid, lo;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        a[e] = __float_as_uint(f[e]);
        bq[e] = __float_as_uint(f[4 + e]);
      }
      split3_8(a, bq, hi, mid, lo);
      *reinterpret_cast<u32x4*>(wl + off) = hi;
      *reinterpret_cast<u32x4*>(wl + DG_WB + off) = mid;
      *reinterpret_cast<u32x4*>(wl + 2 * DG_WB + off) = lo;
    } else {
      *reinterpret_cast<u32x4*>(wl + off) = pack8(f);
    }
  }

  // ---- the lane's channels c0 + 16 h + 4 fq + e and their coefficients (C % 8 == 0: a group of 4 lies wholly
  // inside or outside C; outside, sc = sh = 0 masks everything)
  const float inv_m = 1.f / (float)(p.N * p.H * p.W);
  bool cok[2];
  float sc[2][4], sh[2][4], mu[2][4], is[2][4], k1[2][4], k2[2][4];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int cc = c0 + 16 * h + 4 * fq;
    cok[h] = cc < p.C;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      sc[h][e] = sh[h][e] = mu[h][e] = is[h][e] = k1[h][e] = k2[h][e] = 0.f;
      if (cok[h]) {
        mu[h][e] = p.mean[cc + e];
        is[h][e] = p.invstd[cc + e];
        sc[h][e] = p.gamma[cc + e] * is[h][e];
        sh[h][e] = p.beta[cc + e] - mu[h][e] * sc[h][e];
        if constexpr (APPLY) {
          k1[h][e] = p.dbeta[cc + e] * inv_m;
          k2[h][e] = p.dgamma[cc + e] * inv_m;
        }
      }
    }
  }
  const bool live0 = c0 < p.C, live1 = c0 + 16 < p.C;  // a half past C multiplies nothing (block-uniform)

  // the dz vectors this thread stages: patch row, byte offset relative to the strip's first pixel (or out of
  // range: a halo column, a vector past the patch) and LDS place
  int prow[DG_MAXIT], poff[DG_MAXIT];
  uint32_t plds[DG_MAXIT];
#pragma unroll
  for (int it = 0; it < DG_MAXIT; ++it) {
    const int vi = it * 256 + tid;
    const int pp = vi >> 1, half = vi & 1;
    const int r = pp / W2, c = pp - r * W2;
    const bool in = pp < p.patch_pix;
    const bool ok = in && (unsigned)(c - 1) < (unsigned)p.W;
    prow[it] = ok ? r - 1 : -0x10000;  // (far outside every image)
    poff[it] = (((r - 1) * p.W + c - 1) * p.ldz + half * 8) * (int)E;
    plds[it] = in ? (uint32_t)pp * 32u + (uint32_t)half * 16u : HCB_OOB;
  }
  // the fragments this lane reads. B: its pixel of tile wave + 4 ti (clamped into a full strip: a pixel past
  // the strip's end computes on whatever the patch holds and is discarded by a select), shifted per K block
  // by the lane's tap 2 kb + (fq >> 1); the tenth tap reads tap 8's place and is selected to zero.
  // A: row 16 h + frow of that tap, n half fq & 1
  uint32_t bbase[2], boff[5];
#pragma unroll
  for (int ti = 0; ti < 2; ++ti) {
    const int o = min((wave + 4 * ti) * 16 + frow, p.TR * p.W - 1);
    const int orow = o / p.W;
    bbase[ti] = (uint32_t)(orow * W2 + (o - orow * p.W)) * 32u + (uint32_t)(fq & 1) * 16u;
  }
#pragma unroll
  for (int kb = 0; kb < 5; ++kb) {
    const int tap = min(2 * kb + (fq >> 1), 8);
    boff[kb] = (uint32_t)((2 - tap / 3) * W2 + 2 - tap % 3) * 32u;
  }
  const uint32_t a0 = (uint32_t)((fq >> 1) * 32 + frow) * 32u + (uint32_t)(fq & 1) * 16u;  // K block kb: + kb * 2048

  Act8<T> zv[DG_MAXIT];
  auto gload = [&](int strip) {
    const int n = strip / p.strips_per_img;
    const int h0 = (strip - n * p.strips_per_img) * p.TR;
    const int base = (n * p.H + h0) * p.W * p.ldz * (int)E;
#pragma unroll
    for (int it = 0; it < DG_MAXIT; ++it) {
      const bool ok = (unsigned)(h0 + prow[it]) < (unsigned)p.H;
      zv[it].load(zr, ok ? (uint32_t)(base + poff[it]) : HCB_OOB);
    }
  };
  auto lstore = [&](int b) {
    char* pb = bufs + (size_t)b * buf_b;
#pragma unroll
    for (int it = 0; it < DG_MAXIT; ++it) {
      if (plds[it] == HCB_OOB) continue;
      if constexpr (F32) {
        u32x4 hi, mid, lo;
        split3_8(zv[it].a, zv[it].b, hi, mid, lo);
        *reinterpret_cast<u32x4*>(pb + plds[it]) = hi;
        *reinterpret_cast<u32x4*>(pb + patch_b + plds[it]) = mid;
        *reinterpret_cast<u32x4*>(pb + 2 * patch_b + plds[it]) = lo;
      } else {
        *reinterpret_cast<u32x4*>(pb + plds[it]) = zv[it].v;
      }
    }
  };

  float s1[2][4], s2[2][4];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int e = 0; e < 4; ++e) s1[h][e] = s2[h][e] = 0.f;

  gload(s_beg);  // (no slab is empty)
  lstore(0);
  __syncthreads();
  for (int strip = s_beg; strip < s_end; ++strip) {
    const bool more = strip + 1 < s_end;
    if (more) gload(strip + 1);
    const int n = strip / p.strips_per_img;
    const int h0 = (strip - n * p.strips_per_img) * p.TR;
    const int npix = min(p.TR, p.H - h0) * p.W;
    const size_t m0 = ((size_t)n * p.H + h0) * p.W;

    // ---- x (and gin) of the lane's pixels and channels, in flight while the MFMAs run
    float xf[2][2][4], gf[2][2][4];
    bool val[2][2];
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
      const int o = (wave + 4 * ti) * 16 + frow;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        val[ti][h] = o < npix && cok[h];
        const int cc = c0 + 16 * h + 4 * fq;
#pragma unroll
        for (int e = 0; e < 4; ++e) xf[ti][h][e] = gf[ti][h][e] = 0.f;
        if (!val[ti][h]) continue;
        const T* xp = reinterpret_cast<const T*>(p.x) + (m0 + o) * p.ldx + cc;
        if constexpr (F32) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(xp);
#pragma unroll
          for (int e = 0; e < 4; ++e) xf[ti][h][e] = v[e];
        } else {
          const u32x2 v = *reinterpret_cast<const u32x2*>(xp);
#pragma unroll
          for (int e = 0; e < 4; ++e) xf[ti][h][e] = act2f((uint16_t)(v[e >> 1] >> (16 * (e & 1))));
        }
        if constexpr (APPLY) {
          const T* gp = reinterpret_cast<const T*>(p.gin) + (m0 + o) * p.ldg + cc;
          if constexpr (F32) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(gp);
#pragma unroll
            for (int e = 0; e < 4; ++e) gf[ti][h][e] = v[e];
          } else {
            const u32x2 v = *reinterpret_cast<const u32x2*>(gp);
#pragma unroll
            for (int e = 0; e < 4; ++e) gf[ti][h][e] = act2f((uint16_t)(v[e >> 1] >> (16 * (e & 1))));
          }
        }
      }
    }

    // ---- da of the strip: 5 K blocks x (2 tiles x 2 halves)
    f32x4 acc[2][2];
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int h = 0; h < 2; ++h) acc[ti][h] = f32x4{0.f, 0.f, 0.f, 0.f};
    const char* pb = bufs + (size_t)((strip - s_beg) & 1) * buf_b;
#pragma unroll
    for (int kb = 0; kb < 5; ++kb) {
      u32x4 a[2][NPL];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int t = 0; t < NPL; ++t)
          a[h][t] = *reinterpret_cast<const u32x4*>(wl + t * DG_WB + a0 + kb * 2048 + h * 512);
#pragma unroll
      for (int ti = 0; ti < 2; ++ti) {
        if ((wave + 4 * ti) * 16 >= npix) continue;  // (wave-uniform)
        u32x4 bb[NPL];
#pragma unroll
        for (int t = 0; t < NPL; ++t) {
          bb[t] = *reinterpret_cast<const u32x4*>(pb + t * patch_b + bbase[ti] + boff[kb]);
          if (kb == 4 && fq >= 2) bb[t] = u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          if (!(h == 0 ? live0 : live1)) continue;
          mfma_acc<F32>(a[h], bb, acc[ti][h]);
        }
      }
    }

    // ---- ReLU mask, then the sums or the gin update: lane = pixel frow of its tiles, channels 16 h + 4 fq .. + 3
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
      const int o = (wave + 4 * ti) * 16 + frow;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float out[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float x = xf[ti][h][e];
          const float pre = fmaf(x, sc[h][e], sh[h][e]);
          const float g = (val[ti][h] && pre > 0.f) ? acc[ti][h][e] : 0.f;
          const float xh = (x - mu[h][e]) * is[h][e];
          if constexpr (APPLY) {
            out[e] = gf[ti][h][e] + sc[h][e] * (g - k1[h][e] - xh * k2[h][e]);
          } else {
            s1[h][e] += g;
            s2[h][e] += g * xh;
          }
        }
        if constexpr (APPLY) {
          if (!val[ti][h]) continue;
          T* gp = reinterpret_cast<T*>(p.gin) + (m0 + o) * p.ldg + c0 + 16 * h + 4 * fq;
          if constexpr (F32) {
            *reinterpret_cast<f32x4*>(gp) = f32x4{out[0], out[1], out[2], out[3]};
          } else {
            u32x2 o2;
            o2[0] = pack2(out[0], out[1]);
            o2[1] = pack2(out[2], out[3]);
            *reinterpret_cast<u32x2*>(gp) = o2;
          }
        }
      }
    }
    if (more) lstore((strip + 1 - s_beg) & 1);
    __syncthreads();
  }

  if constexpr (!APPLY) {
    // lanes of one fq hold the same 8 channels: sum the 16 pixels, then the 4 waves in wave order
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          s1[h][e] += __shfl_xor(s1[h][e], o, 64);
          s2[h][e] += __shfl_xor(s2[h][e], o, 64);
        }
        if (frow == 0) {
          red[wave * 64 + 16 * h + 4 * fq + e] = s1[h][e];
          red[wave * 64 + 32 + 16 * h + 4 * fq + e] = s2[h][e];
        }
      }
    __syncthreads();
    if (tid < 64) {
      const float v = red[tid] + red[64 + tid] + red[128 + tid] + red[192 + tid];
      p.ws[((size_t)slab * 2 + (tid >> 5)) * (nchunks * 32) + c0 + (tid & 31)] = v;
    }
  }
}

// dbeta[c] = sum over the slabs of ws[slab][0][c], dgamma[c] of ws[slab][1][c], overwritten. A block folds 16
// consecutive elements: thread (sl, el) sums slabs sl, sl + 16, ... of element el in slab order, then the 16
// partial sums meet in LDS and are added in sl order -- a fixed order, whatever the device
__global__ __launch_bounds__(256) void dense_dgrad_fold_kernel(DenseDgradParams p) {
  __shared__ float part[16][17];
  const int el = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int idx = blockIdx.x * 16 + el;
  const bool ok = idx < 2 * p.C;
  const int k = ok ? idx / p.C : 0, c = ok ? idx - k * p.C : 0;
  float s = 0.f;
  if (ok) {
    const int C32 = (p.C + 31) & ~31;
    const float* src = p.ws + (size_t)k * C32 + c;
    for (int b = sl; b < p.nslabs; b += 16) s += src[(size_t)b * 2 * C32];
  }
  part[sl][el] = s;
  __syncthreads();
  if (sl != 0 || !ok) return;
  float t = part[0][el];
#pragma unroll
  for (int j = 1; j < 16; ++j) t += part[j][el];
  (k == 0 ? p.dbeta : p.dgamma)[c] = t;
}

template <typename T, bool APPLY>
void dg_launch(const DenseDgradParams& p, dim3 grid, size_t lds, hipStream_t st) {
  launch_big_lds(dense_dgrad_kernel<T, APPLY>, grid, lds, st, p, "dense_conv3x3_dgrad");
}

}  // namespace

bool dense_conv3x3_dgrad_plan(int N, int H, int W, int C, bool f32, DenseDgradPlan* out) {
  if (N < 1 || H < 1 || W < 1 || C < 1 || W > DG_STRIP) return false;
  int TR = DG_STRIP / W;
  if (TR > 16) TR = 16;
  if (TR > H) TR = H;
  for (; TR >= 1; --TR) {
    const int pix = (TR + 2) * (W + 2);
    const int npl = f32 ? 3 : 1;
    const size_t lds = (size_t)npl * DG_WB + DG_RED_BYTES + 2 * (size_t)npl * pix * 32;
    if (pix * 2 > DG_MAXIT * 256 || lds > DG_LDS_MAX) continue;
    const int nchunks = (C + 31) / 32;
    const int spi = (H + TR - 1) / TR;
    const int nstrips = N * spi;
    int slabs = (DG_TARGET_WGS + nchunks - 1) / nchunks;
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
    out->ws_floats = (int64_t)slabs * 2 * nchunks * 32;
    return true;
  }
  return false;
}

void launch_dense_conv3x3_dgrad(const DenseDgradParams& p0, hipStream_t st, bool f32) {
  DenseDgradParams p = p0;
  DenseDgradPlan pl;
  if (!dense_conv3x3_dgrad_plan(p.N, p.H, p.W, p.C, f32, &pl)) {  // (the binding refuses it by name first)
    fprintf(stderr, "hcb dense_conv3x3_dgrad: W = %d does not fit the LDS budget\n", p.W);
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
    dg_launch<float, false>(p, grid, pl.lds_bytes, st);
  else
    dg_launch<uint16_t, false>(p, grid, pl.lds_bytes, st);
  hipLaunchKernelGGL(dense_dgrad_fold_kernel, dim3((unsigned)((2 * p.C + 15) / 16)), dim3(256), 0, st, p);
  if (f32)
    dg_launch<float, true>(p, grid, pl.lds_bytes, st);
  else
    dg_launch<uint16_t, true>(p, grid, pl.lds_bytes, st);
}

}  // namespace hcb
