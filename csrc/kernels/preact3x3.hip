// Pre-activation conv of the CIFAR ResNet-v2 basic block on gfx950: BatchNorm -> ReLU -> conv 3x3 / stride 1
// or 2 / TF 'SAME' at 16 / 32 / 64 -> 16 / 32 / 64 channels, in ONE pass over the raw block input:
//   y = conv3x3_SAME(stride s)( relu( gamma * (x - mean) * invstd + beta ) )
// x and y are separate NHWC tensors (row strides ldx / ldy; 16-bit or plain fp32). The normalised operand is
// never written to memory, and y's per-channel statistics (what the BN after conv1 needs) leave with it.
// The padding belongs to the NORMALISED map: halo pixels are selected to zero after BN + ReLU. For stride 2
// on even sizes TF pads 0 on top / left and 1 on bottom / right (pt = pad_total / 2).
//
// Work split (a sibling of dense3x3.hip, which stays the narrow-output, in-place, stride-1 kernel). A
// workgroup of 4 waves owns a strip of TR whole OUTPUT rows of one image. The Nout / 16 MFMA column tiles go
// OVER THE WAVES, not over a second grid dimension: wave w computes column tile w % NCT for the pixel tiles
// w / NCT, w / NCT + 4 / NCT (two 16-pixel tiles per wave, so a strip has at most 128 / NCT output pixels).
// Why: the patch is loaded, normalised, split and stored to LDS by the workgroup that multiplies it, so a
// second grid dimension would repeat that staging -- the costly part of this memory-bound op -- Nout / 16
// times. And the strips shrink as the columns grow: at 8 x 8 x 64 a strip is 4 rows (32 pixels) and every
// wave has its tile pair, so batch 128 launches 256 full workgroups, where the dense kernel's split (all
// columns on every wave) would leave 128 - 256 workgroups with two idle waves each on that map. Only the
// fp32 form at Nout = 64 uses gridDim.y = 2 (two column tiles per workgroup): three planes of 9 x 64 x 32
// weights, doubled, do not fit the 160 KiB of LDS beside a patch.
//
// Per chunk of 32 input channels (one MFMA K; C_in = 16 fills half of it with zeros):
//   global -> registers   the input patch, ((TR - 1) s + 3) x ((Q - 1) s + 3) pixels x 32 channels (s TR + 2
//                         rows at stride 1; stride 2 needs one row less), range-checked 16-byte raw buffer
//                         loads: pixels outside the image and channels past C_in get the out-of-range
//                         offset. The chunk's weights, 9 taps x the workgroup's output rows x 32 channels of
//                         the [Nout][Kpad] pack (K = (tap, c): the ParamStore pack, or dense_pack's), likewise.
//   registers -> LDS      the family's patch store, 64-byte LDS unit and swizzle (patch3x3.h states them once;
//                         stride 1: a fragment's 16 units are consecutive and conflict-free; stride 2 reads
//                         every other unit: 2-way).
//   LDS -> MFMA           v_mfma_f32_16x16x32 (bf16, or f16 in the HCB_F16 build): A = the tap's 16 weight
//                         rows of the wave's column tile (read once per tap, used for both pixel tiles),
//                         B = 16 output pixels read from the resident patch at pixel (orow s + ty, ocol s +
//                         tx): stride 2 is an address pattern, not a second copy. An input element crosses
//                         global -> LDS once. fp32: six products per fragment pair, small terms first.
// The weights of a chunk stay resident in LDS for the whole strip. With two chunks (C_in = 64) both LDS
// buffers are doubled: chunk 1 is loaded before the MFMAs of chunk 0 and stored after them, one barrier per
// chunk; with one chunk there is one buffer. No LDS-DMA (the data changes on the way), no scratch.
//
// mean / invstd are finalised in the kernel from the R replicas of x's statistics accumulator (sum(v - K),
// sum((v - K)^2), filled by bn_stats_acc), with bn_apply_acc's arithmetic; block (0, 0) publishes them and
// updates the moving statistics. Inference passes the moving statistics in the same form (one replica).
// Output statistics: shifted sums of the fp32 accumulators, over the block's strips in registers, across
// lanes by shuffles, across the waves of a column tile through LDS in wave order, then ONE atomic add per
// channel and workgroup into replica blockIdx.x % R. Deterministic mode caps gridDim.x at R (the kernel
// strides over the strips), so every slot receives a single add: bitwise reproducible.
//
// Resources (hipcc -O3, gfx950; no scratch in any instantiation): see the table in README.md ("CIFAR-10
// ResNet-v2"); dynamic LDS = 8 * C32 + 512 + nbuf * planes * (patch_pix + 9 * rows) * 64 bytes, C32 = C_in rounded
// up to 32, nbuf = 2 with two chunks, planes = 3 on fp32, rows = the workgroup's output channels.
#include <cstdio>
#include <cstdlib>

#include "common.h"
#include "kernels.h"
#include "patch3x3.h"

namespace hcb {

namespace {

constexpr int PA_MAXIT = 5;  // patch vectors (8 channels of one pixel) per thread and chunk: patch_pix * 4 <= 5 * 256
constexpr int PA_TILES = 2;  // 16-pixel MFMA tiles per wave
constexpr size_t PA_LDS_MAX = 160 * 1024;

// NCT: the column tiles (of 16 output channels) this workgroup computes, spread over its 4 waves
template <typename T, int NCT>
__global__ __launch_bounds__(256) void preact_conv3x3_kernel(PreactParams p) {
  constexpr bool F32 = sizeof(T) == 4;
  constexpr int NPL = F32 ? 3 : 1;
  constexpr uint32_t E = Act8<T>::ESZ;
  constexpr int NW = 16 * NCT;                      // weight rows (output channels) of the workgroup
  constexpr int WUNITS = 9 * NW;                    // unit = tap * NW + row
  constexpr uint32_t WBYTES = WUNITS * 64u;
  constexpr int WIT = (WUNITS * 4 + 255) / 256;     // weight vectors per thread, chunk and plane
  constexpr int NPW = 4 / NCT;                      // waves that share a column tile
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id_uniform();
  const int frow = lane & 15, fq = lane >> 4;
  const int ct = wave % NCT, pw = wave / NCT;       // the wave's column tile, its first pixel tile
  const int n0 = blockIdx.y * NW;                   // the workgroup's first output channel
  const int Cr = (p.C + 31) & ~31;
  float* coef = reinterpret_cast<float*>(smem);  // [2][Cr]: scale, shift (zeros past C)
  float* red = coef + 2 * Cr;                    // [4 waves][2][16]
  char* bufs = smem + (size_t)(2 * Cr + 128) * 4;
  const uint32_t patch_b = (uint32_t)p.patch_pix * 64u;
  const uint32_t buf_b = NPL * (patch_b + WBYTES);
  const int s = p.stride;

  // ---- BN coefficients of the input channels from the replica sums; block (0, 0) publishes the moments
  bn_coef_from_acc(p, coef, Cr, p.N * p.H * p.W, blockIdx.x == 0 && blockIdx.y == 0);
  __syncthreads();

  const __amdgpu_buffer_rsrc_t xr = make_rsrc(p.x, p.x_bytes);
  __amdgpu_buffer_rsrc_t wr[NPL];
  wr[0] = make_rsrc(p.w, p.w_bytes);
  if constexpr (F32) {
    wr[1] = make_rsrc(p.w_mid, p.w_bytes);
    wr[2] = make_rsrc(p.w_lo, p.w_bytes);
  }
  const int v = tid & 3;  // the thread's 16-byte column of every unit it stages (256 % 4 == 0)

  // the weight vectors this thread stages: unit = tap * NW + row (every row n0 + row < Nout: the launcher's grid)
  uint32_t woff[WIT], wlds[WIT];
#pragma unroll
  for (int it = 0; it < WIT; ++it) {
    const int unit = (it * 256 + tid) >> 2;
    const int tap = unit / NW, row = unit - tap * NW;
    const bool ok = unit < WUNITS;
    woff[it] = ok ? (uint32_t)((n0 + row) * p.Kpad + tap * p.C) * 2u : HCB_OOB;
    wlds[it] = ok ? patch_off(unit, v) : HCB_OOB;
  }
  const uint32_t a0 = patch_off(ct * 16 + frow, fq);  // this lane's weight fragment of tap 0; tap t: + t * NW * 64

  float kout[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) kout[e] = p.stats_shift != nullptr ? p.stats_shift[n0 + ct * 16 + fq * 4 + e] : 0.f;
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};

  const int nchunks = Cr >> 5;
  for (int strip = blockIdx.x; strip < p.nstrips; strip += gridDim.x) {
    const int n = strip / p.strips_per_img;
    const int r0 = (strip - n * p.strips_per_img) * p.TR;  // first output row
    const int rows = min(p.TR, p.P - r0);
    const int npix = rows * p.Q;
    const int ntiles = (npix + 15) >> 4;
    const int h0 = r0 * s - p.pt;  // image row / column of patch pixel (0, 0)
    const int w0 = -p.pl;

    // the patch vectors this thread stages: byte offset of the pixel (or out of range) and LDS place
    uint32_t goff[PA_MAXIT], plds[PA_MAXIT];
#pragma unroll
    for (int it = 0; it < PA_MAXIT; ++it) {
      const int pp = (it * 256 + tid) >> 2;
      const int r = pp / p.PW, c = pp - r * p.PW;
      const int h = h0 + r, w = w0 + c;
      const bool in = pp < p.patch_pix;
      const bool ok = in && (unsigned)h < (unsigned)p.H && (unsigned)w < (unsigned)p.W;
      goff[it] = ok ? (uint32_t)(((size_t)(n * p.H + h) * p.W + w) * p.ldx) * E : HCB_OOB;
      plds[it] = in ? patch_off(pp, v) : HCB_OOB;
    }
    // the pixel fragments this lane reads: tile = pw + NPW * ti, output pixel frow of it (clamped into the strip)
    uint32_t baddr[PA_TILES][9];
#pragma unroll
    for (int ti = 0; ti < PA_TILES; ++ti) {
      const int o = min((pw + NPW * ti) * 16 + frow, npix - 1);
      const int orow = o / p.Q, ocol = o - orow * p.Q;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap)
        baddr[ti][tap] = patch_off((orow * s + tap / 3) * p.PW + ocol * s + tap % 3, fq);
    }

    Act8<T> xv[PA_MAXIT];
    u32x4 wv[WIT][NPL];
    auto gload = [&](int c0) {
      const int cc = c0 + v * 8;
      const bool cok = cc < p.C;
#pragma unroll
      for (int it = 0; it < PA_MAXIT; ++it)
        xv[it].load(xr, (cok && goff[it] != HCB_OOB) ? goff[it] + (uint32_t)cc * E : HCB_OOB);
#pragma unroll
      for (int it = 0; it < WIT; ++it)
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
      for (int it = 0; it < PA_MAXIT; ++it)
        if (plds[it] != HCB_OOB) bnrelu_store<T>(pb, patch_b, plds[it], xv[it], goff[it] != HCB_OOB, sc, sh);
#pragma unroll
      for (int it = 0; it < WIT; ++it) {
        if (wlds[it] == HCB_OOB) continue;
#pragma unroll
        for (int t = 0; t < NPL; ++t) *reinterpret_cast<u32x4*>(wb + t * WBYTES + wlds[it]) = wv[it][t];
      }
    };

    f32x4 acc[PA_TILES];
#pragma unroll
    for (int ti = 0; ti < PA_TILES; ++ti) acc[ti] = f32x4{0.f, 0.f, 0.f, 0.f};

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
          for (int t = 0; t < NPL; ++t) a[t] = *reinterpret_cast<const u32x4*>(wb + t * WBYTES + a0 + tap * (NW * 64));
#pragma unroll
          for (int ti = 0; ti < PA_TILES; ++ti) {
            if (pw + NPW * ti >= ntiles) continue;  // (wave-uniform)
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

    // ---- the strip's outputs: lane = output pixel frow of its tiles, channels n0 + ct * 16 + fq * 4 .. + 3
    const size_t m0 = ((size_t)n * p.P + r0) * p.Q;
#pragma unroll
    for (int ti = 0; ti < PA_TILES; ++ti) {
      const int o = (pw + NPW * ti) * 16 + frow;
      if (o >= npix) continue;
      if (p.stats != nullptr) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = acc[ti][e] - kout[e];
          s1[e] += d;
          s2[e] += d * d;
        }
      }
      T* dst = reinterpret_cast<T*>(p.y) + (m0 + o) * p.ldy + n0 + ct * 16 + fq * 4;
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
  stats_reduce<NCT>(s1, s2, red, p.stats, p.stats_R, p.stats_C, n0, wave, frow, fq);
}

struct PaPlan {
  int nct, gy, TR, P, Q, pt, pl, PW, pix;
  size_t lds;
};

// column tiles per workgroup, strip rows and patch size for this problem; false when it does not fit
bool pa_plan(int H, int W, int C, int Nout, int s, bool f32, PaPlan* pl) {
  if (!(C == 16 || C == 32 || C == 64) || !(Nout == 16 || Nout == 32 || Nout == 64) || !(s == 1 || s == 2)) return false;
  if (H < 1 || W < 1) return false;
  const int nct_all = Nout / 16;
  pl->nct = f32 && nct_all > 2 ? 2 : nct_all;
  pl->gy = nct_all / pl->nct;
  same3(H, s, &pl->P, &pl->pt);
  same3(W, s, &pl->Q, &pl->pl);
  const int maxpix = 16 * PA_TILES * (4 / pl->nct);
  const int Cr = (C + 31) & ~31;
  const int nbuf = Cr > 32 ? 2 : 1;
  pl->PW = (pl->Q - 1) * s + 3;
  int TR = maxpix / pl->Q;
  if (TR > pl->P) TR = pl->P;
  for (; TR >= 1; --TR) {
    const int pix = ((TR - 1) * s + 3) * pl->PW;
    const size_t lds = (size_t)(2 * Cr + 128) * 4 +
                       (size_t)nbuf * (f32 ? 3 : 1) * ((size_t)pix * 64 + (size_t)9 * 16 * pl->nct * 64);
    if (pix * 4 <= PA_MAXIT * 256 && lds <= PA_LDS_MAX) {
      pl->TR = TR;
      pl->pix = pix;
      pl->lds = lds;
      return true;
    }
  }
  return false;
}

template <typename T>
void pa_launch_t(const PreactParams& p, int nct, dim3 grid, size_t lds, hipStream_t st) {
  const char* name = "preact_conv3x3";
  if (nct == 1)
    launch_big_lds(preact_conv3x3_kernel<T, 1>, grid, lds, st, p, name);
  else if (nct == 2)
    launch_big_lds(preact_conv3x3_kernel<T, 2>, grid, lds, st, p, name);
  else if constexpr (sizeof(T) == 2)  // (fp32 never has more than two column tiles per workgroup: pa_plan)
    launch_big_lds(preact_conv3x3_kernel<T, 4>, grid, lds, st, p, name);
}

}  // namespace

bool preact_conv3x3_fits(int N, int H, int W, int C, int Nout, int stride, bool f32) {
  PaPlan pl;
  return N >= 1 && pa_plan(H, W, C, Nout, stride, f32, &pl);
}

void launch_preact_conv3x3(const PreactParams& p0, hipStream_t st, bool f32) {
  PreactParams p = p0;
  PaPlan pl;
  if (!pa_plan(p.H, p.W, p.C, p.Nout, p.stride, f32, &pl)) {  // (the binding refuses it by name first)
    fprintf(stderr, "hcb preact_conv3x3: %d x %d x %d -> %d, stride %d does not fit\n", p.H, p.W, p.C, p.Nout, p.stride);
    abort();
  }
  p.P = pl.P; p.Q = pl.Q; p.pt = pl.pt; p.pl = pl.pl; p.TR = pl.TR; p.PW = pl.PW; p.patch_pix = pl.pix;
  p.strips_per_img = (p.P + p.TR - 1) / p.TR;
  p.nstrips = p.N * p.strips_per_img;
  dim3 grid((unsigned)p.nstrips, (unsigned)pl.gy);
  // deterministic mode: at most R blocks per column group, so each replica slot receives a single add
  if (p.stats != nullptr && deterministic() && (int)grid.x > p.stats_R) grid.x = p.stats_R;
  if (f32)
    pa_launch_t<float>(p, pl.nct, grid, pl.lds, st);
  else
    pa_launch_t<uint16_t>(p, pl.nct, grid, pl.lds, st);
}

}  // namespace hcb
