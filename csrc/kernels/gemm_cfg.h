// The conv GEMM configurations: one table per kernel family, one row per cfg. Whatever has to know
// what a cfg means is derived from its row: the launch switches (conv_igemm.hip, conv3x3_patch.hip,
// conv_wgrad.hip, conv_p3.hip), the block tiles that size statistics slabs and split-K workspaces,
// the cfgs the bindings accept, and hcb.gemm_cfg_table, which tests/test_gemm_cfg_tables.py pins
// against the Python planner's tables. No torch or HIP headers: bindings.cpp reads the same rows.
//
// A row is X(cfg, KIND, WM, WN, TM, TN, ...) in cfg order. KIND selects the launcher: a launch switch
// is the family's rows through HCB_CASE, with HCB_CASE_<KIND> defined beside it. WM x WN waves of
// TM x TN wave tiles make the block tile; the other columns are the family's template arguments (0
// where a kind has none); FB is the cfg that runs when the row's kernel does not serve a problem
// (-1: it always does). A changed row changes what the numbers in tuned/*.json mean: bump
// autotune.CACHE_VERSION with it.
#pragma once

namespace hcb {

enum GemmKind {
  K_REG = 0,      // register-staged double-buffered LDS
  K_GLDS = 1,     // LDS-DMA ring of NST 64-deep stages
  K_PATCH = 2,    // 3x3 / stride 1 with the input patch resident in LDS (conv3x3_patch.hip)
  K_KQ = 3,       // weight grad with an intra-workgroup k-split over KS wave groups
  K_TILE = 4,     // plane GEMM, one workgroup per tile
  K_PERSIST = 5,  // plane GEMM, persistent workgroups (conv_p3_persist.h)
  K_BRES = 7,     // ... with the workgroup's weight slice resident in LDS (6 was its stream-K form)
  K_RETIRED = 8,  // a stream-K number kept for old plans: runs FB
  K_P3PATCH = 9,  // plane GEMM, 3x3 / stride 1 with the input patch resident in LDS (conv_p3_patch.h)
};

// ---------------------------------------------------------------- 16-bit forward / data gradient
// X(cfg, KIND, WM, WN, TM, TN, NST, PMAX, FB). 0-3 register-staged; 4-7 the same tiles on the
// LDS-DMA ring; 8-11 deeper rings for latency-bound few-tile layers; 12-16 eight-wave workgroups
// (two waves per SIMD when a layer has only ~1 tile per CU); 17-21 the patch kernels, PMAX load
// passes of patch at most, FB the LDS-DMA kernel of the same row tile (so per-tile statistics slabs
// keep their size).
// (round 5: the rejected variants -- two k-steps per stage, cfg 22-26; occupancy-sized two-slot
// rings, 27-30; the register-pipelined loop, 31-37; the plane kernel on one 16-bit plane, 100-117 --
// were measured without a step gain and removed: profiles/r5_prune_variants.txt)
#define HCB_CONV_CFGS(X)                  \
  X(0, REG, 2, 2, 64, 64, 0, 0, -1)       \
  X(1, REG, 4, 1, 32, 64, 0, 0, -1)       \
  X(2, REG, 2, 2, 32, 32, 0, 0, -1)       \
  X(3, REG, 1, 4, 64, 32, 0, 0, -1)       \
  X(4, GLDS, 2, 2, 64, 64, 3, 0, -1)      \
  X(5, GLDS, 4, 1, 32, 64, 3, 0, -1)      \
  X(6, GLDS, 2, 2, 32, 32, 4, 0, -1)      \
  X(7, GLDS, 1, 4, 64, 32, 3, 0, -1)      \
  X(8, GLDS, 2, 2, 64, 64, 4, 0, -1)      \
  X(9, GLDS, 2, 2, 64, 64, 5, 0, -1)      \
  X(10, GLDS, 4, 1, 32, 64, 6, 0, -1)     \
  X(11, GLDS, 1, 4, 64, 32, 6, 0, -1)     \
  X(12, GLDS, 2, 4, 64, 32, 3, 0, -1)     \
  X(13, GLDS, 4, 2, 32, 64, 3, 0, -1)     \
  X(14, GLDS, 4, 2, 64, 64, 3, 0, -1)     \
  X(15, GLDS, 2, 4, 64, 64, 3, 0, -1)     \
  X(16, GLDS, 2, 4, 32, 32, 4, 0, -1)     \
  X(17, PATCH, 2, 4, 64, 32, 3, 8, 13)    \
  X(18, PATCH, 4, 2, 64, 64, 3, 8, 14)    \
  X(19, PATCH, 4, 2, 64, 32, 3, 8, 14)    \
  X(20, PATCH, 2, 2, 64, 32, 3, 16, 5)    \
  X(21, PATCH, 2, 4, 64, 32, 4, 8, 13)

// ---------------------------------------------------------------- 16-bit weight gradient
// X(cfg, KIND, WM, WN, TM, TN, NST, KS): block tile = (Nout tile, K tile). 13 / 14: 64x32 / 32x64
// wave tiles, twice the MFMAs per loaded row of the 64x64 tile.
#define HCB_WGRAD_CFGS(X)             \
  X(0, REG, 2, 2, 64, 64, 0, 0)       \
  X(1, REG, 1, 4, 64, 32, 0, 0)       \
  X(2, REG, 2, 2, 32, 32, 0, 0)       \
  X(3, GLDS, 2, 2, 64, 64, 4, 0)      \
  X(4, GLDS, 2, 4, 64, 32, 3, 0)      \
  X(5, GLDS, 4, 2, 64, 64, 3, 0)      \
  X(6, GLDS, 2, 4, 64, 64, 3, 0)      \
  X(7, GLDS, 2, 4, 32, 32, 4, 0)      \
  X(8, GLDS, 2, 2, 32, 32, 4, 0)      \
  X(9, GLDS, 1, 4, 64, 32, 4, 0)      \
  X(10, KQ, 1, 1, 64, 64, 0, 4)       \
  X(11, KQ, 2, 1, 64, 64, 0, 2)       \
  X(12, KQ, 1, 2, 64, 64, 0, 2)       \
  X(13, REG, 2, 2, 64, 32, 0, 0)      \
  X(14, REG, 2, 2, 32, 64, 0, 0)

// ---------------------------------------------------------------- plane (fp32) forward / data gradient
// X(cfg, KIND, WM, WN, TM, TN, KW, NST, OCC, FB): NST ring slots of KW-deep k-slices, built for OCC
// workgroups per CU. 18-22 persistent twins of per-tile cfgs (FB: the twin), 31-36 weights resident.
// 23-30 are the retired stream-K numbers: the form was measured 11-30 % slower per layer than the
// whole-tile persistent kernels (29 / 30, 64x64 wave tiles: 5x slower) and removed
// (profiles/r4v_streamk_probe.txt, profiles/r6_quantization_streamk.txt). The rows stay, with their
// tiles, so that tuned/*.json and autotune caches that name them keep their meaning: each runs FB, the
// cfg it used to fall back to.
#define HCB_P3_CFGS(X)                          \
  X(0, TILE, 2, 2, 64, 32, 64, 2, 1, -1)        \
  X(1, TILE, 2, 2, 32, 64, 64, 2, 1, -1)        \
  X(2, TILE, 4, 2, 32, 32, 64, 2, 1, -1)        \
  X(3, TILE, 2, 4, 32, 32, 64, 2, 1, -1)        \
  X(4, TILE, 2, 2, 32, 32, 64, 2, 1, -1)        \
  X(5, TILE, 4, 1, 32, 64, 64, 2, 1, -1)        \
  X(6, TILE, 1, 4, 64, 32, 64, 2, 1, -1)        \
  X(7, TILE, 2, 4, 64, 32, 32, 3, 1, -1)        \
  X(8, TILE, 4, 2, 32, 64, 32, 3, 1, -1)        \
  X(9, TILE, 2, 2, 64, 64, 32, 3, 1, -1)        \
  X(10, TILE, 4, 2, 64, 64, 32, 2, 1, -1)       \
  X(11, TILE, 2, 4, 64, 64, 32, 2, 1, -1)       \
  X(12, TILE, 2, 2, 32, 64, 32, 4, 1, -1)       \
  X(13, TILE, 2, 2, 64, 32, 32, 4, 1, -1)       \
  X(14, TILE, 2, 2, 64, 32, 32, 2, 2, -1)       \
  X(15, TILE, 2, 2, 32, 64, 32, 2, 2, -1)       \
  X(16, TILE, 2, 2, 32, 32, 32, 3, 2, -1)       \
  X(17, TILE, 2, 2, 32, 32, 32, 2, 3, -1)       \
  X(18, PERSIST, 2, 2, 32, 64, 32, 2, 2, 15)    \
  X(19, PERSIST, 2, 2, 64, 32, 32, 2, 2, 14)    \
  X(20, PERSIST, 2, 2, 32, 32, 32, 3, 2, 16)    \
  X(21, PERSIST, 2, 2, 32, 32, 32, 2, 3, 17)    \
  X(22, PERSIST, 2, 4, 64, 32, 32, 3, 1, 7)     \
  X(23, RETIRED, 2, 2, 32, 64, 32, 2, 2, 18)    \
  X(24, RETIRED, 2, 2, 64, 32, 32, 2, 2, 19)    \
  X(25, RETIRED, 2, 2, 32, 32, 32, 3, 2, 20)    \
  X(26, RETIRED, 2, 2, 32, 32, 32, 2, 3, 21)    \
  X(27, RETIRED, 2, 4, 64, 32, 32, 3, 1, 22)    \
  X(28, RETIRED, 4, 2, 32, 64, 32, 3, 1, 8)     \
  X(29, RETIRED, 4, 2, 64, 64, 32, 2, 1, 10)    \
  X(30, RETIRED, 2, 4, 64, 64, 32, 2, 1, 11)    \
  X(31, BRES, 1, 4, 64, 64, 32, 3, 1, 18)       \
  X(32, BRES, 2, 4, 64, 64, 32, 2, 1, 18)       \
  X(33, BRES, 2, 2, 32, 32, 32, 3, 1, 20)       \
  X(34, BRES, 2, 2, 64, 32, 32, 2, 1, 19)       \
  X(35, BRES, 4, 2, 32, 32, 32, 2, 1, 19)       \
  X(36, BRES, 4, 2, 32, 64, 32, 2, 1, 22)

// ---------------------------------------------------------------- plane (fp32) 3x3 patch kernels
// X(cfg, KIND, WM, WN, TM, TN, KW, NST, OCC, FB): a table of its own, numbered from P3_PATCH_CFG0, so
// that every number of HCB_P3_CFGS (and of tuned/*.json) keeps its meaning. A problem the kernel does
// not serve (not 3x3 / stride 1 / pad 1, C % 32, split-K, a patch that does not fit LDS) runs FB, the
// per-tile cfg of the same block tile.
constexpr int P3_PATCH_CFG0 = 64;
// (measured and not kept: the 2x4 waves of 64x32 form of 64, equal to it; a 128x64 tile of four waves
// for the 64-column stage-1 layers, 33 % slower than their persistent cfg: profiles/p3_patch.txt)
#define HCB_P3PATCH_CFGS(X) X(64, P3PATCH, 4, 2, 32, 64, 32, 3, 1, 8)

// ---------------------------------------------------------------- plane (fp32) weight gradient
// X(cfg, KIND, WM, WN, TM, TN, KW, NST, OCC): NST slots of KW pixel rows. 16-18: persistent twins of
// 12, 13, 15 (their ring is always 2 x 32).
#define HCB_WP3_CFGS(X)                   \
  X(0, TILE, 2, 2, 64, 32, 64, 2, 1)      \
  X(1, TILE, 2, 2, 32, 64, 64, 2, 1)      \
  X(2, TILE, 2, 2, 32, 32, 64, 3, 1)      \
  X(3, TILE, 4, 2, 32, 32, 64, 2, 1)      \
  X(4, TILE, 2, 4, 32, 32, 64, 2, 1)      \
  X(5, TILE, 2, 2, 32, 32, 64, 2, 1)      \
  X(6, TILE, 2, 4, 64, 32, 32, 3, 1)      \
  X(7, TILE, 4, 2, 32, 64, 32, 3, 1)      \
  X(8, TILE, 4, 2, 64, 64, 32, 2, 1)      \
  X(9, TILE, 2, 4, 64, 64, 32, 2, 1)      \
  X(10, TILE, 2, 2, 64, 64, 32, 3, 1)     \
  X(11, TILE, 2, 2, 64, 32, 32, 3, 1)     \
  X(12, TILE, 2, 2, 64, 32, 32, 2, 2)     \
  X(13, TILE, 2, 2, 32, 64, 32, 2, 2)     \
  X(14, TILE, 2, 2, 32, 32, 32, 3, 2)     \
  X(15, TILE, 2, 2, 32, 32, 32, 2, 3)     \
  X(16, PERSIST, 2, 2, 64, 32, 32, 2, 2)  \
  X(17, PERSIST, 2, 2, 32, 64, 32, 2, 2)  \
  X(18, PERSIST, 2, 2, 32, 32, 32, 2, 3)

#define HCB_CASE(C, KIND, ...) HCB_CASE_##KIND(C, __VA_ARGS__)

// ---------------------------------------------------------------- the rows as data
struct GemmCfg {
  int cfg, kind, wm, wn, tm, tn, kw, nst, occ, extra, fb;  // extra: PMAX (patch) / KS (k-split)
};

#define HCB_ROW_CONV(C, KIND, WM, WN, TM, TN, NST, PMAX, FB) {C, K_##KIND, WM, WN, TM, TN, 64, NST, 1, PMAX, FB},
#define HCB_ROW_WGRAD(C, KIND, WM, WN, TM, TN, NST, KS) {C, K_##KIND, WM, WN, TM, TN, 64, NST, 1, KS, -1},
#define HCB_ROW_P3(C, KIND, WM, WN, TM, TN, KW, NST, OCC, FB) {C, K_##KIND, WM, WN, TM, TN, KW, NST, OCC, 0, FB},
#define HCB_ROW_WP3(C, KIND, WM, WN, TM, TN, KW, NST, OCC) {C, K_##KIND, WM, WN, TM, TN, KW, NST, OCC, 0, -1},
inline constexpr GemmCfg CONV_CFGS[] = {HCB_CONV_CFGS(HCB_ROW_CONV)};
inline constexpr GemmCfg WGRAD_CFGS[] = {HCB_WGRAD_CFGS(HCB_ROW_WGRAD)};
inline constexpr GemmCfg P3_CFGS[] = {HCB_P3_CFGS(HCB_ROW_P3)};
inline constexpr GemmCfg WP3_CFGS[] = {HCB_WP3_CFGS(HCB_ROW_WP3)};
inline constexpr GemmCfg P3PATCH_CFGS[] = {HCB_P3PATCH_CFGS(HCB_ROW_P3)};
#undef HCB_ROW_CONV
#undef HCB_ROW_WGRAD
#undef HCB_ROW_P3
#undef HCB_ROW_WP3

template <int N>
constexpr bool gemm_cfgs_in_order(const GemmCfg (&t)[N]) {
  for (int i = 0; i < N; ++i)
    if (t[i].cfg != i || t[i].fb >= N) return false;
  return true;
}
static_assert(gemm_cfgs_in_order(CONV_CFGS) && gemm_cfgs_in_order(WGRAD_CFGS) && gemm_cfgs_in_order(P3_CFGS) &&
                  gemm_cfgs_in_order(WP3_CFGS),
              "row i of a table is cfg i, and falls back inside the table");

constexpr int N_CONV_CFG = sizeof(CONV_CFGS) / sizeof(GemmCfg);
constexpr int N_WGRAD_CFG = sizeof(WGRAD_CFGS) / sizeof(GemmCfg);
constexpr int N_P3_CFG = sizeof(P3_CFGS) / sizeof(GemmCfg);
constexpr int N_WP3_CFG = sizeof(WP3_CFGS) / sizeof(GemmCfg);
constexpr int N_P3PATCH_CFG = sizeof(P3PATCH_CFGS) / sizeof(GemmCfg);

// row i of the patch table is cfg P3_PATCH_CFG0 + i and falls back to a per-tile plane cfg of its block tile
constexpr bool p3_patch_rows_ok() {
  for (int i = 0; i < N_P3PATCH_CFG; ++i) {
    const GemmCfg& r = P3PATCH_CFGS[i];
    if (r.cfg != P3_PATCH_CFG0 + i || r.fb < 0 || r.fb >= N_P3_CFG || r.kw != 32) return false;
    const GemmCfg& f = P3_CFGS[r.fb];
    if (f.kind != K_TILE || f.wm * f.tm != r.wm * r.tm || f.wn * f.tn != r.wn * r.tn) return false;
  }
  return true;
}
static_assert(p3_patch_rows_ok(), "a patch row falls back to the per-tile cfg of the same block tile");
constexpr bool p3_cfg_patch(int cfg) { return cfg >= P3_PATCH_CFG0 && cfg < P3_PATCH_CFG0 + N_P3PATCH_CFG; }
// a cfg the plane forward / data-gradient launcher accepts
constexpr bool p3_cfg_valid(int cfg) { return (cfg >= 0 && cfg < N_P3_CFG) || p3_cfg_patch(cfg); }

// a cfg's launcher kind (-1 outside the table) and block tile (d outside the table)
template <int N>
constexpr int gemm_kind(const GemmCfg (&t)[N], int cfg) {
  return cfg >= 0 && cfg < N ? t[cfg].kind : -1;
}
template <int N>
constexpr int gemm_tile(const GemmCfg (&t)[N], int cfg, bool n, int d) {
  return cfg < 0 || cfg >= N ? d : n ? t[cfg].wn * t[cfg].tn : t[cfg].wm * t[cfg].tm;
}
constexpr int conv_tile_m(int cfg) { return gemm_tile(CONV_CFGS, cfg, false, 128); }
constexpr int conv_tile_n(int cfg) { return gemm_tile(CONV_CFGS, cfg, true, 128); }
constexpr int wgrad_tile_m(int cfg) { return gemm_tile(WGRAD_CFGS, cfg, false, 64); }
constexpr int wgrad_tile_n(int cfg) { return gemm_tile(WGRAD_CFGS, cfg, true, 64); }
constexpr int p3_tile_m(int cfg) {
  return p3_cfg_patch(cfg) ? gemm_tile(P3PATCH_CFGS, cfg - P3_PATCH_CFG0, false, 128) : gemm_tile(P3_CFGS, cfg, false, 128);
}
constexpr int p3_tile_n(int cfg) {
  return p3_cfg_patch(cfg) ? gemm_tile(P3PATCH_CFGS, cfg - P3_PATCH_CFG0, true, 64) : gemm_tile(P3_CFGS, cfg, true, 64);
}
constexpr int p3_slot_k(int cfg) { return cfg >= 0 && cfg < N_P3_CFG ? P3_CFGS[cfg].kw : 32; }
constexpr int wgrad_p3_tile_m(int cfg) { return gemm_tile(WP3_CFGS, cfg, false, 64); }
constexpr int wgrad_p3_tile_n(int cfg) { return gemm_tile(WP3_CFGS, cfg, true, 64); }

// the cfgs with an inference-epilogue (INF) instantiation: every 16-bit cfg but the patch kernels,
// the per-tile plane kernels
constexpr bool conv_cfg_has_inf(int cfg) { return cfg >= 0 && cfg < N_CONV_CFG && CONV_CFGS[cfg].kind != K_PATCH; }
constexpr bool p3_cfg_has_inf(int cfg) { return gemm_kind(P3_CFGS, cfg) == K_TILE; }
// in-launch split-K runs on the LDS-DMA kernels: not on a register-staged row
constexpr bool conv_cfg_splitk(int cfg) { return cfg >= 0 && gemm_kind(CONV_CFGS, cfg) != K_REG; }
constexpr bool wp3_cfg_persistent(int cfg) { return gemm_kind(WP3_CFGS, cfg) == K_PERSIST; }

// ---------------------------------------------------------------- the resident 3x3 patch (conv_p3_patch.h)
// The patch is addressed by a padded linear index with ONE shared zero row between images and ONE
// shared zero column between image rows: Lp(n, p, q) = (n * (H + 1) + p) * (W + 1) + q, and tap (r, s)
// of output pixel (n, p, q) reads row Lp + r * (W + 1) + s. Upper bound of the rows a block of BM
// consecutive output pixels spans: BM - 1 steps, +1 per image-row wrap, +(W + 1) per image wrap, plus
// the window's reach 2 * (W + 1) + 3; rounded up to the 16 rows one wave's LDS-DMA instruction fills.
constexpr int p3_patch_rows(int H, int W, int BM) {
  const int d = BM - 1, span = d + (d + W - 1) / W + (W + 1) * ((d + H * W - 1) / (H * W)) + 2 * (W + 1) + 3;
  return (span + 15) / 16 * 16;
}
// LDS bytes of a launch: NST weight slots of three BN x 64-byte planes, two patch buffers of three
// planes of 64-byte rows, a 1 KB landing zone for the DMA pieces past the patch, the fused BN-backward
// parameters (16 bytes per column)
constexpr long p3_patch_lds(int H, int W, int BM, int BN, int NST, bool bnb) {
  return (long)NST * 3 * BN * 64 + 2l * 3 * p3_patch_rows(H, W, BM) * 64 + 1024 + (bnb ? BN * 16 : 0);
}
// of patch cfg `cfg` on H x W images; 0: not a patch cfg
constexpr long p3_patch_cfg_lds(int cfg, int H, int W, bool bnb) {
  if (!p3_cfg_patch(cfg)) return 0;
  const GemmCfg& r = P3PATCH_CFGS[cfg - P3_PATCH_CFG0];
  return p3_patch_lds(H, W, r.wm * r.tm, r.wn * r.tn, r.nst, bnb);
}
constexpr long P3_PATCH_LDS_MAX = 160 * 1024;

}  // namespace hcb
