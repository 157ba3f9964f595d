// Plane (fp32, bf16x6) 3x3 / stride 1 / pad 1 forward and data-gradient GEMM with the input patch
// RESIDENT IN LDS (the rows of gemm_cfg.h HCB_P3PATCH_CFGS; instantiated in conv_p3.hip).
//
// conv_igemm_p3_kernel fetches an im2col A tile per filter tap, so every input pixel crosses L2 ->
// LDS nine times. Cutting that traffic to 0.57x buys 2-3 % of an isolated launch and 1.0 % of the
// fp32 training step on the 28x28 and 14x14 layers (profiles/p3_patch.txt). Here, as in
// the 16-bit conv3x3_patch.hip, a block's BM consecutive output pixels map to ONE contiguous row range
// of a zero-padded linear index of the input, loaded once per 32-channel slab (three planes); the
// nine shifted A operands are read straight out of it and only the three weight planes stream per
// k-step.
//
//   * padded index with shared padding (gemm_cfg.h p3_patch_rows): Lp(n, p, q) = (n * (H + 1) + p) *
//     (W + 1) + q; tap (r, s) reads Lp + r * (W + 1) + s. Row hh' = 0 of an image is its top padding
//     and the bottom padding of the image before it, column ww' = 0 of a row is its left padding and
//     the right padding of the row before it; both are loaded with an out-of-range buffer offset and
//     arrive as zeros without memory traffic;
//   * k order slab-major, tap-minor: step k = (slab k / 9, tap k % 9). The weight planes stream through
//     the NST-slot LDS-DMA ring with early release and ilv_schedule, exactly as conv_igemm_p3_kernel's
//     register-double-buffered (PIPE) loop; the MFMA step is p3_mma;
//   * the patch is double buffered: slab s + 1's patch is issued in the group of tap 0 of slab s (the
//     barrier of that step has retired every wave's last read of the buffer, tap 8 of slab s - 1),
//     ahead of the step's weight refill. The counted wait of tap 1 .. NST - 2 therefore leaves the
//     patch pieces outstanding, every other wait covers them: each vmcnt is exact;
//   * LDS rows are 64 bytes (32 channels), 16-byte chunks XOR-swizzled with p3_swz<32> on the source
//     side of the lane-linear DMA image and on the fragment reads. A tap's fragment rows start at an
//     arbitrary patch row, so A reads can meet 2-way bank conflicts (as in conv3x3_patch.hip);
//   * every thread issues the same number of patch pieces: a wave whose 16 rows lie past the patch
//     lands zeros in a 1 KB zone nobody reads.
// No split-K, no inference epilogue: such a problem runs the row's FB cfg (launch_p3_patch: false).
#pragma once
#include "conv_p3_fwd.h"
#include "gemm_cfg.h"

namespace hcb {

// padded linear index of output pixel m (P == H, Q == W)
__device__ __forceinline__ int p3p_lp(const ConvParams& p, int m) {
  const int n = (int)fdiv((uint32_t)m, p.fd_hw), r = m - n * p.H * p.W;
  const int pp = (int)fdiv((uint32_t)r, p.fd_w), qq = r - pp * p.W;
  return (n * (p.H + 1) + pp) * (p.W + 1) + qq;
}

template <int BN, int NST>
constexpr int p3p_ring_bytes() {
  return NST * NPL * BN * 64;
}
// load passes (NT / 4 rows each) that cover the largest patch the LDS can hold beside the ring
template <int BN, int NST, int NT>
constexpr int p3p_pmax() {
  const int rows = (int)((P3_PATCH_LDS_MAX - p3p_ring_bytes<BN, NST>() - 1024 - BN * 16) / (2 * NPL * 64));
  return (rows + NT / 4 - 1) / (NT / 4);
}

template <int WM, int WN, int TM, int TN, int NST, bool BNB>
__global__ __launch_bounds__(WM* WN * 64, WM* WN / 4) void conv_p3_patch_kernel(ConvParams p) {
  constexpr int BM = WM * TM, BN = WN * TN;
  constexpr int MI = TM / 16, NI = TN / 16;
  constexpr int NT = WM * WN * 64, RB = 64, RP = NT / 4;  // threads; bytes per LDS row; rows per load pass
  constexpr int BV = BN / RP;
  constexpr int LW = NPL * BV;                  // weight pieces per thread per slot
  constexpr int PMAX = p3p_pmax<BN, NST, NT>();
  constexpr int PL = NPL * PMAX;                // patch pieces per thread per slab
  constexpr int BIMG = BN * RB, BSTAGE = NPL * BIMG;
  static_assert(BV >= 1 && BV * RP == BN, "weight tile rows must be a multiple of the load pass");
  static_assert(NST >= 3 && NST <= 4 && (NST - 1) * LW + PL <= 63, "vmcnt range");
  static_assert(igemm_epilogue_lds(BM, BN, WM) <= (size_t)p3p_ring_bytes<BN, NST>() + 2 * NPL * 16 * RB,
                "the epilogue staging must lie below the BN parameters");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = wave_id_uniform();
  const int wm = wid / WN, wn = wid % WN;
  const int tiles_n = (p.Nout + BN - 1) / BN;
  const int tile = xcd_remap(blockIdx.x, gridDim.x);
  const int tm = tile / tiles_n, tn = tile % tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;
  const int chunk = (tid & 3) ^ p3_swz<32>(tid >> 2);  // source chunk of the lane-linear DMA image
  const int W1 = p.W + 1;

  const int prows_max = p.patch_rows;   // multiple of 16 (launcher)
  const int pimg = prows_max * RB;      // one plane of a patch buffer
  char* ring = smem;
  char* patch = smem + NST * BSTAGE;
  char* sink = patch + 2 * NPL * pimg;  // 1 KB: pieces of waves past the patch
  const size_t param_off = (size_t)(NST * BSTAGE + 2 * NPL * pimg + 1024);

  const char* xb = reinterpret_cast<const char*>(p.x);
  const __amdgpu_buffer_rsrc_t xr0 = make_rsrc(xb, p.x_bytes);
  const __amdgpu_buffer_rsrc_t xr1 = make_rsrc(xb + p.x_plane, p.x_bytes);
  const __amdgpu_buffer_rsrc_t xr2 = make_rsrc(xb + 2 * (size_t)p.x_plane, p.x_bytes);
  const __amdgpu_buffer_rsrc_t wr0 = make_rsrc(p.w, p.w_bytes);
  const __amdgpu_buffer_rsrc_t wr1 = make_rsrc(p.w_lo, p.w_bytes);
  const __amdgpu_buffer_rsrc_t wr2 = make_rsrc(p.w_lo2, p.w_bytes);

  // the block's input patch: padded rows [lbase, lbase + prows), prows <= patch_rows (the launcher's
  // bound; clamped all the same, so that no read or DMA piece leaves the buffer)
  const int mlast = min(m0 + BM, p.M) - 1;
  const int lbase = p3p_lp(p, m0);
  const int reach = 2 * W1 + 3;
  const int prows = min(p3p_lp(p, mlast) + reach - lbase, prows_max);
  uint32_t poff[PMAX];  // byte offset of this thread's patch chunk, channel slab 0
  {
    const int HW1 = (p.H + 1) * W1;
#pragma unroll
    for (int v = 0; v < PMAX; ++v) {
      const int j = v * RP + (tid >> 2);
      uint32_t o = HCB_OOB;
      if (j < prows) {
        const int L = lbase + j;
        const int n = (int)fdiv((uint32_t)L, p.fd_hw2), rem = L - n * HW1;
        const int hh = (int)fdiv((uint32_t)rem, p.fd_w2), ww = rem - hh * W1;
        if (n < p.N && hh >= 1 && ww >= 1)
          o = (uint32_t)((((n * p.H + hh - 1) * p.W + ww - 1) * p.ldx + chunk * 8) * 2);
      }
      poff[v] = o;
    }
  }
  // this lane's fragment rows in the patch (rows past M read a valid row; the epilogue discards them)
  int prow[MI];
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int m = m0 + wm * TM + i * 16 + (lane & 15);
    prow[i] = min(p3p_lp(p, m <= mlast ? m : mlast) - lbase, prows_max - reach);
  }
  uint32_t b_off[BV];
#pragma unroll
  for (int v = 0; v < BV; ++v) {
    const int j = n0 + (tid >> 2) + RP * v;
    b_off[v] = (j < p.Nout) ? (uint32_t)(j * p.Kpad + chunk * 8) * 2u : HCB_OOB;
  }

  const int nslab = p.C / 32, nk = nslab * 9;

  f32x4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  EpiPrefetch<WM, WN, TM, TN, BNB, true> pre;
  pre.load_shift(p, n0, wn, lane);
  if constexpr (BNB) stage_bnb_params<BN, NT>(p, n0, smem + param_off);  // published by the first barrier

  // the patch of slab sl into buffer sl & 1: PL pieces per thread, whatever the patch's size
  auto load_patch = [&](int sl) {
    char* pb = patch + (sl & 1) * NPL * pimg;
    const uint32_t cb = (uint32_t)sl * 64u;
#pragma unroll
    for (int v = 0; v < PMAX; ++v) {
      const int row0 = v * RP + wid * 16;  // wave-uniform
      const bool in = row0 < prows_max;
      const uint32_t o = (in && poff[v] != HCB_OOB) ? poff[v] + cb : HCB_OOB;
      char* d = pb + row0 * RB;
      glds16(xr0, in ? d : sink, o);
      glds16(xr1, in ? d + pimg : sink, o);
      glds16(xr2, in ? d + 2 * pimg : sink, o);
    }
  };
  // the weight planes of step k (slab sl, tap t) into ring slot `stage`; past the last step every
  // offset is out of range (zeros into a slot nobody reads again), so the vmcnt arithmetic is uniform
  auto issue_w = [&](int stage, int sl, int t) {
    const bool live = sl < nslab;
    const uint32_t kb = (uint32_t)(t * p.C + sl * 32) * 2u;
    char* sb = ring + stage * BSTAGE + wid * 16 * RB;
#pragma unroll
    for (int v = 0; v < BV; ++v) {
      const uint32_t o = (b_off[v] == HCB_OOB || !live) ? HCB_OOB : b_off[v] + kb;
      glds16(wr0, sb + RP * v * RB, o);
      glds16(wr1, sb + BIMG + RP * v * RB, o);
      glds16(wr2, sb + 2 * BIMG + RP * v * RB, o);
    }
  };
  // the fragments of step (sl, t): A from the patch at the tap's row offset, B from the ring slot
  const int frow = lane & 15, fq = lane >> 4;
  auto read = [&](int stage, int sl, int t, P3Frags<TM, TN, 1>& f) {
    const int r = t / 3, tapoff = r * W1 + (t - 3 * r);
    const u32x4* A = reinterpret_cast<const u32x4*>(patch + (sl & 1) * NPL * pimg);
    const u32x4* B = reinterpret_cast<const u32x4*>(ring + stage * BSTAGE);
    const int aimg = prows_max * 4;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int row = prow[i] + tapoff, o = row * 4 + (fq ^ p3_swz<32>(row));
#pragma unroll
      for (int t3 = 0; t3 < NPL; ++t3) f.a[0][t3][i] = A[t3 * aimg + o];
    }
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int row = wn * TN + j * 16 + frow, o = row * 4 + (fq ^ p3_swz<32>(row));
#pragma unroll
      for (int t3 = 0; t3 < NPL; ++t3) f.b[0][t3][j] = B[t3 * (BIMG / 16) + o];
    }
  };

  load_patch(0);
#pragma unroll
  for (int s = 0; s < NST; ++s) issue_w(s, s / 9, s % 9);  // NST <= 4 < 9: slab 0
  P3Frags<TM, TN, 1> fr[2];
  wait_vmcnt<(NST - 1) * LW>();  // patch 0 and slot 0 have landed for this thread
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  read(0, 0, 0, fr[0]);

  constexpr int NMF = MI * NI * 6, NRD = (MI + NI) * NPL;
  int sl = 0, t = 0, st = 0;  // step k = sl * 9 + t, its ring slot st = k % NST
  // the step NST ahead (refilled into the slot this step releases)
  int slr = NST / 9, tr = NST % 9;
  auto body = [&](P3Frags<TM, TN, 1>& cur, P3Frags<TM, TN, 1>& nxt) {
    const bool has_next = sl + 1 < nslab;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's reads of step k are done
    // step k + 1's weights have landed for this thread once only what was issued after them is
    // outstanding: NST - 2 slots, and at taps 1 .. NST - 2 the next slab's patch (issued at tap 0)
    if (has_next && t >= 1 && t <= NST - 2)
      wait_vmcnt<(NST - 2) * LW + PL>();
    else
      wait_vmcnt<(NST - 2) * LW>();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (has_next && t == 0) load_patch(sl + 1);
    issue_w(st, slr, tr);
    // step k + 1
    int sn = sl, tn1 = t + 1, stn = st + 1;
    if (tn1 == 9) {
      tn1 = 0;
      ++sn;
    }
    if (stn == NST) stn = 0;
    read(stn, sn, tn1, nxt);
    p3_mma<TM, TN, 1>(cur, acc);
    ilv_schedule<NMF, LW, NRD>();
    sl = sn;
    t = tn1;
    st = stn;
    if (++tr == 9) {
      tr = 0;
      ++slr;
    }
  };
  for (int k = 0; k < nk; k += 2) {
    body(fr[0], fr[1]);
    if (k + 1 < nk) body(fr[1], fr[0]);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the dummy pieces have landed before LDS reuse
  __syncthreads();  // every wave is done reading before the epilogue reuses LDS
  igemm_epilogue<WM, WN, TM, TN, BNB, true, false>(p, acc, smem, tm, m0, n0, wm, wn, lane, tid, pre, false,
                                                   BNB ? smem + param_off : nullptr);
}

// the problems the patch kernels serve
inline bool p3_patch_eligible(const ConvParams& p) {
  return p.R == 3 && p.S == 3 && p.stride_h == 1 && p.stride_w == 1 && p.pad_h == 1 && p.pad_w == 1 &&
         p.dil_h == 1 && p.dil_w == 1 && p.idil_h == 1 && p.idil_w == 1 && p.P == p.H && p.Q == p.W &&
         p.C % 32 == 0 && p.Kpad >= 9 * p.C && !p.remap && p.splits == 1 && !p.inf && !p.y_p3 &&
         p.w_lo != nullptr && p.w_lo2 != nullptr;
}

// false (nothing launched): the problem or the LDS budget does not fit
template <int WM, int WN, int TM, int TN, int NST>
static bool launch_p3_patch(ConvParams p, hipStream_t st) {
  constexpr int BM = WM * TM, BN = WN * TN, NT = WM * WN * 64;
  if (!p3_patch_eligible(p)) return false;
  const bool bnb = p.bnb_acc != nullptr;
  const int rows = p3_patch_rows(p.H, p.W, BM);
  const long lds = p3_patch_lds(p.H, p.W, BM, BN, NST, bnb);
  if (lds > P3_PATCH_LDS_MAX || rows > p3p_pmax<BN, NST, NT>() * (NT / 4)) return false;
  p.patch_rows = rows;
  p.fd_hw = make_fastdiv((uint32_t)(p.H * p.W));
  p.fd_w = make_fastdiv((uint32_t)p.W);
  p.fd_hw2 = make_fastdiv((uint32_t)((p.H + 1) * (p.W + 1)));
  p.fd_w2 = make_fastdiv((uint32_t)(p.W + 1));
  static const hipError_t once[2] = {set_lds_max(conv_p3_patch_kernel<WM, WN, TM, TN, NST, false>),
                                     set_lds_max(conv_p3_patch_kernel<WM, WN, TM, TN, NST, true>)};
  (void)once;
  const int tiles = ((p.M + BM - 1) / BM) * ((p.Nout + BN - 1) / BN);
  if (bnb)
    hipLaunchKernelGGL((conv_p3_patch_kernel<WM, WN, TM, TN, NST, true>), dim3(tiles), dim3(NT), (size_t)lds, st, p);
  else
    hipLaunchKernelGGL((conv_p3_patch_kernel<WM, WN, TM, TN, NST, false>), dim3(tiles), dim3(NT), (size_t)lds, st, p);
  return true;
}

// the rows of gemm_cfg.h HCB_P3PATCH_CFGS: -1 launched, else the cfg that serves the problem (FB)
#define HCB_CASE_P3PATCH(C, WM, WN, TM, TN, KW, NST, OCC, FB) \
  case C: return launch_p3_patch<WM, WN, TM, TN, NST>(p, st) ? -1 : FB;
static int launch_p3_patch_cfg(const ConvParams& p, int cfg, hipStream_t st) {
  switch (cfg) {
    HCB_P3PATCH_CFGS(HCB_CASE)
    default: return cfg;
  }
}
#undef HCB_CASE_P3PATCH

}  // namespace hcb
