// torch.library registrations (namespace `hcb`; `hcb16` for the IEEE-fp16 build of the same
// sources, -DHCB_F16 -Dhcb=hcb16) for the hand-written gfx950 kernels.
//
// Every op is a thin, allocation-free launcher: Python pre-allocates outputs with the
// caching allocator (so the whole training step can be captured in a HIP graph) and
// passes geometry as an int list; the launcher validates shapes / byte ranges on the
// host BEFORE anything reaches the GPU (an out-of-range gather must never be launched)
// and enqueues on the current HIP stream.
#include <algorithm>
#include <cmath>
#include <vector>

#include <torch/library.h>
#include <ATen/core/Tensor.h>
#include <ATen/ops/empty.h>
#include <c10/hip/HIPStream.h>
#include <c10/util/Exception.h>

#include "kernels/kernels.h"

using at::Tensor;

#ifdef HCB_F16
constexpr at::ScalarType kAct = at::kHalf;  // 16-bit activation / GEMM operand type of this build
#define HCB_ACT_NAME "float16"
#else
constexpr at::ScalarType kAct = at::kBFloat16;
#define HCB_ACT_NAME "bfloat16"
#endif
// library name through one macro level, so -Dhcb=hcb16 also renames the torch.library namespace
#define HCB_TORCH_LIBRARY(ns, m) TORCH_LIBRARY(ns, m)
#define HCB_TORCH_LIBRARY_IMPL(ns, k, m) TORCH_LIBRARY_IMPL(ns, k, m)

namespace {

hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

// raw pointers (the Python side owns and keeps the tensors alive; no static Tensor dtor at exit)
float* g_splitk_ws = nullptr;
int64_t g_splitk_ws_bytes = 0;
unsigned* g_splitk_cnt = nullptr;
int64_t g_splitk_cnt_n = 0;

void check_cuda(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), "hcb: ", name, " must be a GPU tensor");
}
void check_act(const Tensor& t, const char* name) {
  check_cuda(t, name);
  TORCH_CHECK(t.scalar_type() == kAct, "hcb: ", name, " must be " HCB_ACT_NAME " (the activation dtype of this build)");
}
// an activation of this build's 16-bit type, or (bf16 library only) fp32 -- the reference
// precision path (--compute_dtype fp32); returns true for fp32
bool check_act_or_f32(const Tensor& t, const char* name) {
  check_cuda(t, name);
#ifndef HCB_F16
  if (t.scalar_type() == at::kFloat) return true;
#endif
  TORCH_CHECK(t.scalar_type() == kAct, "hcb: ", name, " must be " HCB_ACT_NAME " or float32");
  return false;
}
bool same_act(const Tensor& a, const Tensor& b, const char* name) {
  const bool f = check_act_or_f32(b, name);
  TORCH_CHECK(a.scalar_type() == b.scalar_type(), "hcb: ", name, " dtype differs from the other activations");
  return f;
}
void check_f32(const Tensor& t, const char* name) {
  check_cuda(t, name);
  TORCH_CHECK(t.scalar_type() == at::kFloat, "hcb: ", name, " must be float32");
}
// bytes addressable from t.data_ptr() to the end of its storage
int64_t avail_bytes(const Tensor& t) {
  return (int64_t)t.storage().nbytes() - t.storage_offset() * (int64_t)t.element_size();
}
void check_range(const Tensor& t, int64_t need_bytes, const char* name) {
  TORCH_CHECK(need_bytes <= avail_bytes(t), "hcb: ", name, " needs ", need_bytes,
              " bytes but only ", avail_bytes(t), " are addressable");
}
void check_align16(const void* p, const char* name) {
  TORCH_CHECK(((uintptr_t)p & 15) == 0, "hcb: ", name, " must be 16-byte aligned");
}

// fp32 path (conv_p3.hip): a plane tensor is bf16 [3, ...] (plane t = select(0, t))
int64_t check_planes(const Tensor& t, const char* name) {
  check_cuda(t, name);
  TORCH_CHECK(t.scalar_type() == at::kBFloat16 && t.dim() >= 2 && t.size(0) == 3,
              "hcb: ", name, " must be bf16 planes [3, ...]");
  TORCH_CHECK(t.stride(-1) == 1, "hcb: ", name, " channels must be contiguous");
  check_align16(t.data_ptr(), name);
  TORCH_CHECK((t.stride(0) * 2) % 16 == 0, "hcb: ", name, " plane stride must keep 16-byte alignment");
  return t.stride(0);  // elements between planes
}

// Bytes of an NHWC conv input that the kernels may address. ldx < C is a ROW WINDOW: pixel w's C
// "channels" are the ldx channels of pixels w, w+1, ... (the space-to-depth stem's 4x4 filter read as
// 4x1 over 64-channel windows of 16-channel pixels: one contiguous 128-byte row per filter row,
// StemS2D.fold_spec); the buffer then ends with the tensor and the windows of the last pixels, which
// no output reads, run out of range (zeros).
static int64_t x_span_bytes(int64_t N, int64_t H, int64_t W, int64_t C, int64_t ldx, int64_t e) {
  return ldx >= C ? ((N * H * W - 1) * ldx + C) * e : N * H * W * ldx * e;
}

// The two geometry lists, decoded HERE and nowhere else: entry i of the list is field i of the table,
// the order of ops/functional.py's ConvGeom / WgradGeom records (conv_geom_fields exports the names
// and tests/test_conv_geom_cpu.py holds the two orders equal).
template <class P>
struct GeomField {
  const char* name;
  int P::*field;
};
using CP = hcb::ConvParams;
using WP = hcb::WgradParams;
const GeomField<CP> kConvGeom[] = {
    {"N", &CP::N}, {"H", &CP::H}, {"W", &CP::W}, {"C", &CP::C}, {"ldx", &CP::ldx},
    {"P", &CP::P}, {"Q", &CP::Q}, {"R", &CP::R}, {"S", &CP::S},
    {"sh", &CP::stride_h}, {"sw", &CP::stride_w}, {"ph", &CP::pad_h}, {"pw", &CP::pad_w},
    {"dh", &CP::dil_h}, {"dw", &CP::dil_w}, {"idh", &CP::idil_h}, {"idw", &CP::idil_w},
    {"Nout", &CP::Nout}, {"K", &CP::K}, {"Kpad", &CP::Kpad}, {"ldy", &CP::ldy},
    {"remap", &CP::remap}, {"OH", &CP::OH}, {"OW", &CP::OW}, {"osh", &CP::osh}, {"osw", &CP::osw},
    {"beta", &CP::beta}, {"out_f32", &CP::out_f32},
    {"relu", &CP::relu}, {"stats_R", &CP::stats_R}, {"splits", &CP::splits}, {"oh0", &CP::oh0}, {"ow0", &CP::ow0}};
const GeomField<WP> kWgradGeom[] = {
    {"N", &WP::N}, {"H", &WP::H}, {"W", &WP::W}, {"C", &WP::C}, {"ldx", &WP::ldx},
    {"P", &WP::P}, {"Q", &WP::Q}, {"R", &WP::R}, {"S", &WP::S},
    {"sh", &WP::stride_h}, {"sw", &WP::stride_w}, {"ph", &WP::pad_h}, {"pw", &WP::pad_w},
    {"dh", &WP::dil_h}, {"dw", &WP::dil_w}, {"Nout", &WP::Nout}, {"ldy", &WP::ldy}};

template <class P, size_t n>
P decode_geom(const GeomField<P> (&fields)[n], at::IntArrayRef g, const char* op) {
  TORCH_CHECK(g.size() == n, "hcb.", op, ": geom must have ", n, " entries");
  P p{};
  for (size_t i = 0; i < n; ++i) p.*fields[i].field = (int)g[i];
  p.M = p.N * p.P * p.Q;
  return p;
}

std::vector<std::string> conv_geom_fields(std::string kind) {
  std::vector<std::string> out;
  if (kind == "conv") {
    for (const auto& f : kConvGeom) out.push_back(f.name);
  } else if (kind == "wgrad") {
    for (const auto& f : kWgradGeom) out.push_back(f.name);
  } else {
    TORCH_CHECK(false, "hcb.conv_geom_fields: kind is conv or wgrad");
  }
  return out;
}

// output rows of a GEMM (after remap) and the bytes that `rows` rows of Nout columns, read and written
// as whole 8-column vectors, span at row stride ld
int64_t out_rows(const hcb::ConvParams& p) { return p.remap ? (int64_t)p.N * p.OH * p.OW : (int64_t)p.M; }
int64_t pad8(int64_t n) { return (n + 7) / 8 * 8; }
int64_t out_span_bytes(int64_t rows, int64_t ld, int64_t Nout, int64_t esz) {
  return ((rows - 1) * ld + pad8(Nout)) * esz;
}

// the geometry, operand and byte-range checks every forward / data-gradient / inference GEMM shares
// (x: the 16-bit input, or plane 0 of a plane input); statistics and split-K are attached per family
hcb::ConvParams conv_params(const Tensor& x, const Tensor& w, const Tensor& y, const c10::optional<Tensor>& yres,
                            const c10::optional<Tensor>& bias, at::IntArrayRef g) {
  hcb::ConvParams p = decode_geom(kConvGeom, g, "conv_igemm");
  check_act(x, "x");
  check_act(w, "w");
  check_cuda(y, "y");
  TORCH_CHECK(p.C % 8 == 0 && p.ldx % 8 == 0 && (p.ldx >= p.C || p.C % p.ldx == 0),
              "hcb.conv_igemm: C, ldx must be multiples of 8 (ldx < C: a row window, C a multiple of ldx)");
  TORCH_CHECK(p.Kpad % 64 == 0 && p.Kpad >= p.K && p.K == p.R * p.S * p.C,
              "hcb.conv_igemm: Kpad must be a multiple of 64 >= K = R*S*C");
  TORCH_CHECK(p.ldy % 8 == 0 && p.ldy >= pad8(p.Nout), "hcb.conv_igemm: bad ldy");
  TORCH_CHECK(p.idil_h >= 1 && p.idil_w >= 1 && p.dil_h >= 1 && p.dil_w >= 1, "hcb.conv_igemm: bad dilation");
  TORCH_CHECK(p.M > 0 && p.Nout > 0, "hcb.conv_igemm: empty problem");
  int64_t xb = x_span_bytes(p.N, p.H, p.W, p.C, p.ldx, 2);
  int64_t wb = (int64_t)p.Nout * p.Kpad * 2;
  TORCH_CHECK(xb < (1ll << 31) && wb < (1ll << 31), "hcb.conv_igemm: operand exceeds 2 GiB buffer range");
  check_range(x, xb, "x");
  check_range(w, wb, "w");
  TORCH_CHECK(p.remap >= 0 && p.remap <= 2, "hcb.conv_igemm: remap is 0, 1 or 2");
  if (p.remap) {
    TORCH_CHECK(p.oh0 >= 0 && p.ow0 >= 0 && (p.P - 1) * p.osh + p.oh0 < p.OH && (p.Q - 1) * p.osw + p.ow0 < p.OW,
                "hcb.conv_igemm: remap out of range");
    // remap 2 zeroes each GEMM pixel's whole stride cell: the cells must cover the output
    TORCH_CHECK(p.remap != 2 || (!p.beta && p.oh0 == 0 && p.ow0 == 0 && p.P * p.osh >= p.OH && p.Q * p.osw >= p.OW),
                "hcb.conv_igemm: remap 2 needs cells covering the output and no beta");
  } else {
    TORCH_CHECK(p.oh0 == 0 && p.ow0 == 0, "hcb.conv_igemm: a remap origin needs remap");
  }
  const int64_t span = out_span_bytes(out_rows(p), p.ldy, p.Nout, p.out_f32 ? 4 : 2);
  TORCH_CHECK(y.scalar_type() == (p.out_f32 ? at::kFloat : kAct), "hcb.conv_igemm: y dtype");
  check_range(y, span, "y");
  check_align16(x.data_ptr(), "x");
  check_align16(w.data_ptr(), "w");
  check_align16(y.data_ptr(), "y");
  p.x = x.data_ptr();
  p.w = w.data_ptr();
  p.y = y.data_ptr();
  if (p.beta) {
    TORCH_CHECK(yres.has_value(), "hcb.conv_igemm: beta needs yres");
    check_range(*yres, span, "yres");
    check_align16(yres->data_ptr(), "yres");
    p.yres = yres->data_ptr();
  }
  if (bias.has_value()) {
    check_f32(*bias, "bias");
    TORCH_CHECK(bias->numel() >= p.Nout, "hcb.conv_igemm: bias too small");
    p.bias = bias->data_ptr<float>();
  }
  p.x_bytes = (uint32_t)xb;
  p.w_bytes = (uint32_t)wb;
  return p;
}

// the statistics buffer of a GEMM epilogue: stats_R replicas, or one slab per row tile of tile_m rows
void attach_stats(hcb::ConvParams& p, const c10::optional<Tensor>& stats, int tile_m, const char* op) {
  if (!stats.has_value()) return;
  check_f32(*stats, "stats");
  const int64_t rows = p.stats_R > 0 ? p.stats_R : (p.M + tile_m - 1) / tile_m;
  TORCH_CHECK(stats->numel() >= rows * 2 * p.Nout, "hcb.", op, ": stats buffer too small");
  p.stats = stats->data_ptr<float>();
}

// the split-K workspace of a GEMM of bm x bn tiles with p.splits > 1
void attach_splitk(hcb::ConvParams& p, int bm, int bn, const char* op) {
  TORCH_CHECK(p.splits >= 1 && p.splits <= p.Kpad / 64, "hcb.", op, ": 1 <= splits <= k-steps");
  if (p.splits == 1) return;
  const int64_t tiles = (int64_t)((p.M + bm - 1) / bm) * ((p.Nout + bn - 1) / bn);
  TORCH_CHECK(g_splitk_ws != nullptr && g_splitk_cnt != nullptr, "hcb.", op, ": split-K workspace not set");
  TORCH_CHECK(tiles * p.splits * bm * bn * 4 <= g_splitk_ws_bytes, "hcb.", op, ": split-K workspace too small");
  TORCH_CHECK(tiles <= g_splitk_cnt_n, "hcb.", op, ": split-K counter array too small");
  p.ws = g_splitk_ws;
  p.cnt = g_splitk_cnt;
}

// a 16-bit GEMM (conv_igemm.hip): conv_params plus the statistics slab and split-K against the conv tiles
hcb::ConvParams igemm_params(const Tensor& x, const Tensor& w, const Tensor& y, const c10::optional<Tensor>& yres,
                             const c10::optional<Tensor>& bias, const c10::optional<Tensor>& stats,
                             at::IntArrayRef g, int64_t cfg) {
  hcb::ConvParams p = conv_params(x, w, y, yres, bias, g);
  attach_stats(p, stats, hcb::conv_tile_m((int)cfg), "conv_igemm");
  TORCH_CHECK(p.splits <= 1 || hcb::conv_cfg_splitk((int)cfg),
              "hcb.conv_igemm: split-K needs an LDS-DMA config (cfg >= 4)");
  attach_splitk(p, hcb::conv_tile_m((int)cfg), hcb::conv_tile_n((int)cfg), "conv_igemm");
  return p;
}

// split-K scratch shared by every conv launch of the process (one compute stream): fp32 slabs
// and zero-initialised per-tile tickets that the kernels leave zeroed
void set_splitk_workspace(const Tensor& ws, const Tensor& cnt) {
  check_f32(ws, "ws");
  check_cuda(cnt, "cnt");
  TORCH_CHECK(cnt.scalar_type() == at::kInt && cnt.is_contiguous() && ws.is_contiguous(), "hcb: bad split-K workspace");
  g_splitk_ws = ws.data_ptr<float>();
  g_splitk_ws_bytes = ws.numel() * 4;
  g_splitk_cnt = reinterpret_cast<unsigned*>(cnt.data_ptr<int>());
  g_splitk_cnt_n = cnt.numel();
}

const float* opt_f32(const c10::optional<Tensor>& t, int64_t n, const char* what) {
  if (!t.has_value()) return nullptr;
  check_f32(*t, what);
  TORCH_CHECK(t->numel() >= n, "hcb: ", what, " too small");
  return t->data_ptr<float>();
}

void conv_igemm(const Tensor& x, const Tensor& w, const Tensor& y, const c10::optional<Tensor>& yres,
                const c10::optional<Tensor>& bias, const c10::optional<Tensor>& stats,
                at::IntArrayRef g, int64_t cfg, const c10::optional<Tensor>& stats_shift) {
  hcb::ConvParams p = igemm_params(x, w, y, yres, bias, stats, g, cfg);
  TORCH_CHECK(!stats_shift.has_value() || p.stats != nullptr, "hcb.conv_igemm: stats_shift without stats");
  p.stats_shift = opt_f32(stats_shift, p.Nout, "stats_shift");
  hcb::launch_conv_igemm(p, (int)cfg, cur_stream());
}

// data-grad conv whose output is the dy of a BN layer: the epilogue gates it with the
// layer's ReLU mask (mode 1: y > 0, 2: recomputed from z, 0: none), stores g and adds
// sum(g), sum(g*xhat) per channel into acc [R][2][Nout] (see ConvParams::bnb_*)
// the fused BN-backward fields of a data-grad GEMM; f32: the fp32 path (z fp32, y the [3, ...] bf16
// planes of the activation -- the epilogue reads the hi plane -- output g fp32)
void set_bnb(hcb::ConvParams& p, const Tensor& z, const c10::optional<Tensor>& yact, int64_t ld, const Tensor& mean,
             const Tensor& invstd, const Tensor& gamma, const Tensor& beta, const Tensor& acc, int64_t R, int64_t mode,
             bool f32) {
  TORCH_CHECK(!p.relu && p.bias == nullptr, "hcb.conv_igemm_bnb: no bias / relu");
  TORCH_CHECK(p.out_f32 == (f32 ? 1 : 0), "hcb.conv_igemm_bnb: 16-bit output (fp32 on the fp32 path)");
  TORCH_CHECK(mode >= 0 && mode <= 2 && R >= 1, "hcb.conv_igemm_bnb: bad mode / R");
  TORCH_CHECK(ld % 8 == 0 && ld >= pad8(p.Nout), "hcb.conv_igemm_bnb: bad ld");
  if (f32)
    check_f32(z, "z");
  else
    check_act(z, "z");
  check_range(z, out_span_bytes(out_rows(p), ld, p.Nout, f32 ? 4 : 2), "z");
  check_align16(z.data_ptr(), "z");
  p.bnb_y = nullptr;
  if (mode == 1) {
    TORCH_CHECK(yact.has_value(), "hcb.conv_igemm_bnb: mode 1 needs y");
    if (f32)
      check_planes(*yact, "y");
    else
      check_act(*yact, "y");
    check_range(*yact, out_span_bytes(out_rows(p), ld, p.Nout, 2), "y");
    check_align16(yact->data_ptr(), "y");
    p.bnb_y = yact->data_ptr();
  }
  for (const Tensor* t : {&mean, &invstd, &gamma, &beta}) {
    check_f32(*t, "bn param");
    TORCH_CHECK(t->numel() >= p.Nout, "hcb.conv_igemm_bnb: per-channel tensor too small");
  }
  check_f32(acc, "acc");
  TORCH_CHECK(acc.numel() >= R * 2 * p.Nout, "hcb.conv_igemm_bnb: acc too small");
  p.bnb_z = z.data_ptr();
  p.bnb_ld = (int)ld;
  p.bnb_mean = mean.data_ptr<float>();
  p.bnb_invstd = invstd.data_ptr<float>();
  p.bnb_gamma = gamma.data_ptr<float>();
  p.bnb_beta = beta.data_ptr<float>();
  p.bnb_acc = acc.data_ptr<float>();
  p.bnb_mode = (int)mode;
  p.bnb_R = (int)R;
}


// data-grad conv whose output is the dy of a BN layer: the epilogue gates it with the
// layer's ReLU mask (mode 1: y > 0, 2: recomputed from z, 0: none), stores g and adds
// sum(g), sum(g*xhat) per channel into acc [R][2][Nout] (see ConvParams::bnb_*)
void conv_igemm_bnb(const Tensor& x, const Tensor& w, const Tensor& y, const c10::optional<Tensor>& yres,
                    at::IntArrayRef g, int64_t cfg, const Tensor& z, const c10::optional<Tensor>& yact,
                    int64_t ld, const Tensor& mean, const Tensor& invstd, const Tensor& gamma, const Tensor& beta,
                    const Tensor& acc, int64_t R, int64_t mode) {
  hcb::ConvParams p = igemm_params(x, w, y, yres, c10::nullopt, c10::nullopt, g, cfg);
  set_bnb(p, z, yact, ld, mean, invstd, gamma, beta, acc, R, mode, false);
  hcb::launch_conv_igemm(p, (int)cfg, cur_stream());
}

// the inference-epilogue fields of a forward GEMM (ConvParams::inf): the four live BN vectors and eps;
// the residual (p.beta, validated by conv_params against y's format, rows and ldy) stays in p.yres
void set_inf(hcb::ConvParams& p, const Tensor& y, const Tensor& gamma, const Tensor& beta, const Tensor& mean,
             const Tensor& var, double eps) {
  TORCH_CHECK(p.bias == nullptr && p.stats == nullptr && p.remap == 0 && p.idil_h == 1 && p.idil_w == 1,
              "hcb.conv_inf: a forward conv without bias / statistics / remap / lhs dilation");
  TORCH_CHECK(eps > 0.0, "hcb.conv_inf: eps > 0");
  for (const Tensor* t : {&gamma, &beta, &mean, &var}) {
    check_f32(*t, "bn param");
    TORCH_CHECK(t->dim() == 1 && t->numel() == p.Nout && t->is_contiguous() && t->device() == y.device(),
                "hcb.conv_inf: gamma / beta / moving mean / moving variance must be fp32 [cout] on the output's device");
  }
  p.bnb_gamma = gamma.data_ptr<float>();
  p.bnb_beta = beta.data_ptr<float>();
  p.bnb_mean = mean.data_ptr<float>();
  p.bnb_invstd = var.data_ptr<float>();  // the moving variance (see ConvParams::inf)
  p.inf = 1;
  p.inf_eps = (float)eps;
}

// forward conv + inference BN (+ residual, ReLU) in the GEMM epilogue: y = act(scale * conv(x, w) +
// shift [+ res]), 16-bit y; geom as conv_igemm (beta = 1: res is read, in y's format and ldy)
void conv_igemm_inf(const Tensor& x, const Tensor& w, const Tensor& y, const c10::optional<Tensor>& res,
                    at::IntArrayRef g, int64_t cfg, const Tensor& gamma, const Tensor& beta, const Tensor& mean,
                    const Tensor& var, double eps) {
  TORCH_CHECK(hcb::conv_cfg_has_inf((int)cfg), "hcb.conv_igemm_inf: cfg 0..16 (a patch cfg runs its LDS-DMA twin)");
  hcb::ConvParams p = igemm_params(x, w, y, res, c10::nullopt, c10::nullopt, g, cfg);
  TORCH_CHECK(x.scalar_type() != at::kFloat && !p.out_f32,
              "hcb.conv_igemm_inf: 16-bit operands and output (fp32 runs on the plane GEMMs: hcb.conv_p3_inf)");
  TORCH_CHECK(!p.beta || res->scalar_type() == y.scalar_type(), "hcb.conv_igemm_inf: res dtype differs from y");
  set_inf(p, y, gamma, beta, mean, var, eps);
  hcb::launch_conv_igemm(p, (int)cfg, cur_stream());
}

// the rows of a family's table (gemm_cfg.h), flat, 12 per cfg: cfg, kind, WM, WN, TM, TN, slot depth,
// ring slots, occupancy, PMAX / KS, fallback cfg (-1 none), has an inference-epilogue instantiation
// host-only: the LDS bytes a plane 3x3 patch cfg needs on H x W images (gemm_cfg.h p3_patch_lds;
// its launcher runs the row's fallback above P3_PATCH_LDS_MAX) and the patch rows of one buffer
std::vector<int64_t> p3_patch_fit(int64_t cfg, int64_t H, int64_t W, bool bnb) {
  TORCH_CHECK(hcb::p3_cfg_patch((int)cfg) && H >= 1 && W >= 1 && H < 32768 && W < 32768, "hcb.p3_patch_fit: a patch cfg, H, W >= 1");
  const int bm = hcb::p3_tile_m((int)cfg);
  return {(int64_t)hcb::p3_patch_cfg_lds((int)cfg, (int)H, (int)W, bnb), (int64_t)hcb::p3_patch_rows((int)H, (int)W, bm),
          (int64_t)hcb::P3_PATCH_LDS_MAX};
}

std::vector<int64_t> gemm_cfg_table(std::string family) {
  const hcb::GemmCfg* rows = nullptr;
  int n = 0;
  bool (*inf)(int) = [](int) { return false; };
  if (family == "conv") {
    rows = hcb::CONV_CFGS, n = hcb::N_CONV_CFG, inf = hcb::conv_cfg_has_inf;
  } else if (family == "wgrad") {
    rows = hcb::WGRAD_CFGS, n = hcb::N_WGRAD_CFG;
  } else if (family == "p3") {
    rows = hcb::P3_CFGS, n = hcb::N_P3_CFG, inf = hcb::p3_cfg_has_inf;
  } else if (family == "wgrad_p3") {
    rows = hcb::WP3_CFGS, n = hcb::N_WP3_CFG;
  } else if (family == "p3_patch") {
    rows = hcb::P3PATCH_CFGS, n = hcb::N_P3PATCH_CFG;
  } else {
    TORCH_CHECK(false, "hcb.gemm_cfg_table: family is conv, wgrad, p3, wgrad_p3 or p3_patch");
  }
  std::vector<int64_t> out;
  for (int i = 0; i < n; ++i) {
    const hcb::GemmCfg& r = rows[i];
    for (int v : {r.cfg, r.kind, r.wm, r.wn, r.tm, r.tn, r.kw, r.nst, r.occ, r.extra, r.fb, (int)inf(i)}) out.push_back(v);
  }
  return out;
}

// The weight-gradient GEMM of both precisions: the 17-entry geometry, its checks, the k-step split and
// the fast divisors. dy / x: the 16-bit operands, or plane 0 of plane operands; op: "conv_wgrad" /
// "conv_wgrad_p3". Returns the split count that leaves no empty split.
int wgrad_params(hcb::WgradParams& p, const Tensor& dy, const Tensor& x, const Tensor& dw, at::IntArrayRef g,
                 int64_t splits, const char* op) {
  p = decode_geom(kWgradGeom, g, op);
  check_f32(dw, "dw");
  p.K = p.R * p.S * p.C;
  TORCH_CHECK(p.C % 8 == 0 && p.ldx % 8 == 0, "hcb.", op, ": C, ldx multiples of 8");
  TORCH_CHECK(p.ldy % 8 == 0 && p.ldy >= p.Nout, "hcb.", op, ": bad ldy");
  TORCH_CHECK(splits >= 1, "hcb.", op, ": splits >= 1");
  const int64_t xb = x_span_bytes(p.N, p.H, p.W, p.C, p.ldx, 2);
  const int64_t yb = out_span_bytes(p.M, p.ldy, p.Nout, 2);
  TORCH_CHECK(xb < (1ll << 31) && yb < (1ll << 31), "hcb.", op, ": operand exceeds 2 GiB");
  check_range(dw, (int64_t)p.Nout * p.K * 4, "dw");
  const int nkt = (p.M + 63) / 64;
  const int per = (nkt + (int)splits - 1) / (int)splits;
  p.ksteps_per_split = per;
  p.fd_pq = hcb::make_fastdiv((uint32_t)(p.P * p.Q));
  p.fd_q = hcb::make_fastdiv((uint32_t)p.Q);
  p.fd_c = hcb::make_fastdiv((uint32_t)p.C);
  p.fd_s = hcb::make_fastdiv((uint32_t)p.S);
  p.dy = dy.data_ptr();
  p.x = x.data_ptr();
  p.dw = dw.data_ptr<float>();
  p.dy_bytes = (uint32_t)yb;
  p.x_bytes = (uint32_t)xb;
  return (nkt + per - 1) / per;
}

void conv_wgrad(const Tensor& dy, const Tensor& x, const Tensor& dw, at::IntArrayRef g, int64_t cfg,
                int64_t splits) {
  const bool f32 = same_act(dy, x, "x");
  TORCH_CHECK(!f32, "hcb.conv_wgrad: 16-bit operands only (fp32 runs on the plane GEMMs: hcb.conv_wgrad_p3)");
  hcb::WgradParams p;
  const int eff_splits = wgrad_params(p, dy, x, dw, g, splits, "conv_wgrad");
  check_range(x, p.x_bytes, "x");
  check_range(dy, p.dy_bytes, "dy");
  check_align16(x.data_ptr(), "x");
  check_align16(dy.data_ptr(), "dy");
  hcb::launch_conv_wgrad(p, (int)cfg, eff_splits, cur_stream());
}

// the BN apply kernels' activation code: 0 none, 1 ReLU, 2 ReLU with the upper clip act_max (ReLU6)
int relu_code(int64_t relu, const c10::optional<double>& act_max) {
  TORCH_CHECK(!act_max.has_value() || (relu != 0 && *act_max > 0.0), "hcb.bn_apply: act_max clips a ReLU at a positive value");
  return relu == 0 ? 0 : (act_max.has_value() ? 2 : 1);
}

void bn_apply(const Tensor& x, int64_t ldx, const Tensor& y, int64_t ldy, const c10::optional<Tensor>& res,
              int64_t ldr, int64_t M, int64_t C, const Tensor& mean, const Tensor& invstd,
              const Tensor& gamma, const Tensor& beta, int64_t relu, c10::optional<double> act_max) {
  check_act(x, "x");
  check_act(y, "y");
  TORCH_CHECK(C % 8 == 0 && C <= 2048 && ldx % 8 == 0 && ldy % 8 == 0, "hcb.bn_apply: C/ld");
  check_range(x, ((M - 1) * ldx + C) * 2, "x");
  check_range(y, ((M - 1) * ldy + C) * 2, "y");
  const void* rp = nullptr;
  if (res.has_value()) {
    check_act(*res, "res");
    TORCH_CHECK(ldr % 8 == 0, "hcb.bn_apply: ldr");
    check_range(*res, ((M - 1) * ldr + C) * 2, "res");
    rp = res->data_ptr();
  }
  hcb::launch_bn_apply(x.data_ptr(), (int)ldx, y.data_ptr(), (int)ldy, rp, (int)ldr, (int)M, (int)C,
                       mean.data_ptr<float>(), invstd.data_ptr<float>(), gamma.data_ptr<float>(),
                       beta.data_ptr<float>(), relu_code(relu, act_max), cur_stream(), (float)act_max.value_or(0.0));
}

// geom = [N,H,W,C,P,Q,ldy,kh,kw,sh,sw,ph,pw]; z contiguous [N,H,W,C]
void bn_relu_maxpool_acc(const Tensor& z, const Tensor& y, const Tensor& amax, at::IntArrayRef g, const Tensor& acc,
                         int64_t R, double eps, double momentum, const Tensor& gamma, const Tensor& beta,
                         const Tensor& saved_mean, const Tensor& saved_invstd, const Tensor& run_mean,
                         const Tensor& run_var, const c10::optional<Tensor>& shift) {
  TORCH_CHECK(g.size() == 13, "hcb.bn_relu_maxpool_acc: geom");
  const bool f32 = check_act_or_f32(z, "z");
  // fp32 z with a bf16 y: y is the [3, ...] bf16 planes of the fp32 output (conv_p3 operands)
  const bool yp3 = f32 && y.scalar_type() == at::kBFloat16;
  const int64_t yps = yp3 ? check_planes(y, "y") : 0;
  if (!yp3) same_act(z, y, "y");
  const int64_t e = f32 ? 4 : 2;
  check_cuda(amax, "amax");
  const int64_t N = g[0], H = g[1], W = g[2], C = g[3], P = g[4], Q = g[5], ldy = g[6];
  TORCH_CHECK(z.is_contiguous() && z.numel() == N * H * W * C, "hcb.bn_relu_maxpool_acc: z contiguous [N,H,W,C]");
  TORCH_CHECK(C % 8 == 0 && C <= 2048 && ldy % 8 == 0 && ldy >= C, "hcb.bn_relu_maxpool_acc: C / ldy");
  TORCH_CHECK(g[7] * g[8] <= 255, "hcb.bn_relu_maxpool_acc: window too large for the uint8 argmax");
  check_range(y, yp3 ? (2 * yps + (N * P * Q - 1) * ldy + C) * 2 : ((N * P * Q - 1) * ldy + C) * e, "y");
  TORCH_CHECK(amax.scalar_type() == at::kByte && amax.is_contiguous() && amax.numel() >= N * P * Q * C,
              "hcb.bn_relu_maxpool_acc: amax uint8 [N,P,Q,C]");
  TORCH_CHECK(N * P * Q < (1ll << 31) && N * H * W < (1ll << 31), "hcb.bn_relu_maxpool_acc: 32-bit index range");
  for (const Tensor* t : {&acc, &gamma, &beta, &saved_mean, &saved_invstd, &run_mean, &run_var}) check_f32(*t, "bn");
  TORCH_CHECK(acc.numel() >= R * 2 * C && gamma.numel() >= C && beta.numel() >= C && saved_mean.numel() >= C &&
                  saved_invstd.numel() >= C && run_mean.numel() >= C && run_var.numel() >= C,
              "hcb.bn_relu_maxpool_acc: per-channel tensors too small");
  hcb::launch_bn_relu_maxpool_acc(z.data_ptr(), N, H, W, C, y.data_ptr(), P, Q, ldy, amax.data_ptr(), g[7], g[8], g[9],
                                  g[10], g[11], g[12], acc.data_ptr<float>(), R, (float)eps, (float)momentum,
                                  gamma.data_ptr<float>(), beta.data_ptr<float>(), saved_mean.data_ptr<float>(),
                                  saved_invstd.data_ptr<float>(), run_mean.data_ptr<float>(),
                                  run_var.data_ptr<float>(), opt_f32(shift, C, "shift"), cur_stream(), f32, yps);
}

// geom = [N,H,W,C,ldx,P,Q,ldy,kh,kw,sh,sw,ph,pw,is_max,incl_pad]
void pool_fwd(const Tensor& x, const Tensor& y, const c10::optional<Tensor>& idx, at::IntArrayRef g) {
  TORCH_CHECK(g.size() == 16, "hcb.pool_fwd: geom");
  check_act(x, "x");
  check_act(y, "y");
  TORCH_CHECK(g[3] % 8 == 0 && g[4] % 8 == 0 && g[7] % 8 == 0, "hcb.pool_fwd: C/ld % 8");
  TORCH_CHECK(g[0] * g[5] * g[6] * (g[3] / 8) < (1ll << 31), "hcb.pool_fwd: 32-bit index range");
  check_range(x, ((g[0] * g[1] * g[2] - 1) * g[4] + g[3]) * 2, "x");
  check_range(y, ((g[0] * g[5] * g[6] - 1) * g[7] + g[3]) * 2, "y");
  void* ip = nullptr;
  if (idx.has_value()) {
    TORCH_CHECK(idx->scalar_type() == at::kByte && idx->is_contiguous() && idx->numel() >= g[0] * g[5] * g[6] * g[3],
                "hcb.pool_fwd: idx must be contiguous uint8 [N,P,Q,C]");
    ip = idx->data_ptr();
  }
  hcb::launch_pool_fwd(x.data_ptr(), y.data_ptr(), g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[8],
                       g[9], g[10], g[11], g[12], g[13], g[14], g[15], ip, cur_stream());
}

// fp32 path: the pool on bf16 planes; x / y [3][N][H|P][W|Q][ld] (channel-slice views allowed)
void pool_fwd_p3(const Tensor& x, const Tensor& y, const c10::optional<Tensor>& idx, at::IntArrayRef g) {
  TORCH_CHECK(g.size() == 16, "hcb.pool_fwd_p3: geom");
  const int64_t xps = check_planes(x, "x"), yps = check_planes(y, "y");
  TORCH_CHECK(g[3] % 8 == 0 && g[4] % 8 == 0 && g[7] % 8 == 0, "hcb.pool_fwd_p3: C/ld % 8");
  TORCH_CHECK(g[0] * g[5] * g[6] * (g[3] / 8) < (1ll << 31), "hcb.pool_fwd_p3: 32-bit index range");
  check_range(x, (2 * xps + (g[0] * g[1] * g[2] - 1) * g[4] + g[3]) * 2, "x");
  check_range(y, (2 * yps + (g[0] * g[5] * g[6] - 1) * g[7] + g[3]) * 2, "y");
  void* ip = nullptr;
  if (idx.has_value()) {
    TORCH_CHECK(g[14] && idx->scalar_type() == at::kByte && idx->is_contiguous() &&
                    idx->numel() >= g[0] * g[5] * g[6] * g[3],
                "hcb.pool_fwd_p3: idx (max pool only) must be contiguous uint8 [N,P,Q,C]");
    ip = idx->data_ptr();
  }
  hcb::launch_pool_fwd_p3((const uint16_t*)x.data_ptr(), xps, (uint16_t*)y.data_ptr(), yps, g[0], g[1], g[2], g[3],
                          g[4], g[5], g[6], g[7], g[8], g[9], g[10], g[11], g[12], g[13], g[14], g[15], ip,
                          cur_stream());
}

void pool_bwd(const Tensor& dy, const Tensor& x, const Tensor& y, const c10::optional<Tensor>& idx,
              const Tensor& dx, at::IntArrayRef g, bool accumulate) {
  TORCH_CHECK(g.size() == 16, "hcb.pool_bwd: geom");
  const bool f32 = check_act_or_f32(dy, "dy");
  same_act(dy, x, "x");
  same_act(dy, y, "y");
  same_act(dy, dx, "dx");
  const int64_t e = f32 ? 4 : 2;
  check_range(x, ((g[0] * g[1] * g[2] - 1) * g[4] + g[3]) * e, "x");
  check_range(dx, ((g[0] * g[1] * g[2] - 1) * g[4] + g[3]) * e, "dx");
  check_range(y, ((g[0] * g[5] * g[6] - 1) * g[7] + g[3]) * e, "y");
  check_range(dy, ((g[0] * g[5] * g[6] - 1) * g[7] + g[3]) * e, "dy");
  if (f32)  // the fp32 kernel set: the argmax-gather max-pool backward, the 3x3/1 average pool
    TORCH_CHECK((g[14] && idx.has_value() && g[8] == g[9] && g[10] == g[11] && (g[8] + g[10] - 1) / g[10] <= 3 &&
                 g[0] * g[1] <= 65535 && g[0] * g[1] * g[2] * g[4] < (1ll << 31) &&
                 g[0] * g[5] * g[6] * std::max(g[7], g[3]) < (1ll << 31)) ||
                    (!g[14] && g[8] == 3 && g[9] == 3 && g[10] == 1 && g[11] == 1 &&
                     g[0] * g[5] * g[6] * g[7] * 4 < 0x7fffffffLL),
                "hcb.pool_bwd: fp32 supports the square max pool with its argmax and the 3x3/1 average pool");
  TORCH_CHECK(g[3] % 8 == 0 && g[4] % 8 == 0 && g[7] % 8 == 0, "hcb.pool_bwd: C/ld % 8");
  TORCH_CHECK(g[0] * g[1] * g[2] * (g[3] / 8) < (1ll << 31), "hcb.pool_bwd: 32-bit index range");
  if (idx.has_value())
    TORCH_CHECK(idx->scalar_type() == at::kByte && idx->is_contiguous() && idx->numel() >= g[0] * g[5] * g[6] * g[3],
                "hcb.pool_bwd: idx must be contiguous uint8 [N,P,Q,C]");
  hcb::launch_pool_bwd(dy.data_ptr(), x.data_ptr(), y.data_ptr(), dx.data_ptr(), g[0], g[1], g[2], g[3],
                       g[4], g[5], g[6], g[7], g[8], g[9], g[10], g[11], g[12], g[13], g[14], g[15],
                       accumulate ? 1 : 0, idx.has_value() ? idx->data_ptr() : nullptr, cur_stream(), f32);
}

void gap_fwd(const Tensor& x, const Tensor& y, int64_t N, int64_t HW, int64_t C) {
  const bool f32 = check_act_or_f32(x, "x");
  same_act(x, y, "y");
  const int64_t e = f32 ? 4 : 2;
  TORCH_CHECK(C % 8 == 0, "hcb.gap_fwd: C % 8");
  check_range(x, N * HW * C * e, "x");
  check_range(y, N * C * e, "y");
  hcb::launch_gap_fwd(x.data_ptr(), y.data_ptr(), (int)N, (int)HW, (int)C, cur_stream(), f32);
}

void gap_bwd(const Tensor& dy, const Tensor& dx, int64_t N, int64_t HW, int64_t C) {
  const bool f32 = check_act_or_f32(dy, "dy");
  same_act(dy, dx, "dx");
  const int64_t e = f32 ? 4 : 2;
  check_range(dy, N * C * e, "dy");
  check_range(dx, N * HW * C * e, "dx");
  hcb::launch_gap_bwd(dy.data_ptr(), dx.data_ptr(), (int)N, (int)HW, (int)C, cur_stream(), f32);
}

void softmax_xent(const Tensor& logits, int64_t ld, const Tensor& labels, int64_t ncls,
                  const Tensor& row_loss, const Tensor& dlogits, int64_t lddl, double scale,
                  const c10::optional<Tensor>& scale_dev, const c10::optional<Tensor>& dl32,
                  double label_smoothing) {
  check_f32(logits, "logits");
  TORCH_CHECK(label_smoothing >= 0.0 && label_smoothing <= 1.0, "hcb.softmax_xent: label_smoothing in [0, 1]");
  check_cuda(labels, "labels");
  TORCH_CHECK(labels.scalar_type() == at::kLong, "hcb.softmax_xent: labels int64");
  const bool f32 = check_act_or_f32(dlogits, "dlogits");
  int64_t B = labels.numel();
  check_range(logits, B * ld * 4, "logits");
  check_range(dlogits, B * lddl * (f32 ? 4 : 2), "dlogits");
  TORCH_CHECK(row_loss.numel() >= B, "hcb.softmax_xent: row_loss");
  float* d32 = nullptr;
  if (dl32.has_value()) {  // 16-bit dlogits: also the unrounded fp32 values (the bias gradient's source)
    TORCH_CHECK(!f32, "hcb.softmax_xent: dl32 only with 16-bit dlogits");
    check_f32(*dl32, "dl32");
    check_range(*dl32, B * lddl * 4, "dl32");
    d32 = dl32->data_ptr<float>();
  }
  hcb::launch_softmax_xent(logits.data_ptr<float>(), (int)ld, labels.data_ptr<int64_t>(), (int)B, (int)ncls,
                           row_loss.data_ptr<float>(), dlogits.data_ptr(), (int)lddl, (float)scale,
                           scale_dev.has_value() ? scale_dev->data_ptr<float>() : nullptr, cur_stream(), f32, d32,
                           (float)label_smoothing);
}

// counters[0:3] += {examples, top-1 hits, top-5 hits} of the batch (csrc/kernels/metrics.hip)
void eval_metrics(const Tensor& logits, int64_t ld, const Tensor& labels, int64_t ncls, const Tensor& counters) {
  check_f32(logits, "logits");
  check_cuda(labels, "labels");
  check_cuda(counters, "counters");
  TORCH_CHECK(labels.scalar_type() == at::kLong, "hcb.eval_metrics: labels int64");
  TORCH_CHECK(counters.scalar_type() == at::kLong, "hcb.eval_metrics: counters int64");
  TORCH_CHECK(logits.is_contiguous() && labels.is_contiguous() && counters.is_contiguous(),
              "hcb.eval_metrics: contiguous tensors only");
  TORCH_CHECK(counters.numel() >= 3, "hcb.eval_metrics: counters[3]");
  TORCH_CHECK(ncls >= 1 && ld >= ncls, "hcb.eval_metrics: ld >= ncls >= 1");
  TORCH_CHECK(logits.device() == labels.device() && logits.device() == counters.device(),
              "hcb.eval_metrics: logits, labels and counters on one device");
  const int64_t B = labels.numel();
  TORCH_CHECK(B * ld < (int64_t)1 << 31, "hcb.eval_metrics: B * ld < 2^31");
  TORCH_CHECK(logits.numel() >= B * ld, "hcb.eval_metrics: logits hold ", logits.numel(), " elements, B * ld = ",
              B * ld);
  hcb::launch_eval_metrics(logits.data_ptr<float>(), (int)ld, labels.data_ptr<int64_t>(), (int)B, (int)ncls,
                           counters.data_ptr<int64_t>(), cur_stream());
}

void nonfinite(const Tensor& g, const Tensor& flag) {
  check_f32(g, "g");
  check_f32(flag, "flag");
  TORCH_CHECK(g.is_contiguous() && flag.numel() >= 1, "hcb.nonfinite: args");
  check_align16(g.data_ptr(), "g");
  hcb::launch_nonfinite(g.data_ptr<float>(), g.numel(), flag.data_ptr<float>(), cur_stream());
}

void loss_total(const Tensor& row_loss, int64_t B, const c10::optional<Tensor>& l2, double half_wd,
                const Tensor& loss) {
  check_f32(row_loss, "row_loss");
  check_f32(loss, "loss");
  TORCH_CHECK(B >= 1 && row_loss.numel() >= B && loss.numel() >= 1, "hcb.loss_total: args");
  const float* l2p = nullptr;
  if (l2.has_value()) {
    check_f32(*l2, "l2");
    TORCH_CHECK(l2->numel() >= 1 && l2->is_contiguous(), "hcb.loss_total: l2");
    l2p = l2->data_ptr<float>();
  }
  hcb::launch_loss_total(row_loss.data_ptr<float>(), (int)B, l2p, l2p ? (int)l2->numel() : 0, (float)half_wd,
                         loss.data_ptr<float>(), cur_stream());
}

void loss_scale_update(const Tensor& hyper, double world, bool dynamic) {
  check_f32(hyper, "hyper");
  TORCH_CHECK(hyper.numel() >= 8 && hyper.is_contiguous(), "hcb.loss_scale_update: hyper[8]");
  hcb::launch_loss_scale_update(hyper.data_ptr<float>(), (float)world, dynamic ? 1 : 0, cur_stream());
}

// zero up to ZERO_BUFS contiguous fp32 tensors (16-byte aligned) in one launch
void zero_bufs(at::TensorList ts) {
  TORCH_CHECK(ts.size() >= 1 && ts.size() <= (size_t)hcb::ZERO_BUFS, "hcb.zero_bufs: 1..", hcb::ZERO_BUFS, " tensors");
  float* ptrs[hcb::ZERO_BUFS];
  int64_t ns[hcb::ZERO_BUFS];
  for (size_t i = 0; i < ts.size(); ++i) {
    check_f32(ts[i], "zero_bufs");
    TORCH_CHECK(ts[i].is_contiguous(), "hcb.zero_bufs: contiguous tensors only");
    check_align16(ts[i].data_ptr(), "zero_bufs");
    ptrs[i] = ts[i].data_ptr<float>();
    ns[i] = ts[i].numel();
  }
  hcb::launch_zero_bufs(ptrs, ns, (int)ts.size(), cur_stream());
}

void colsum(const Tensor& g, int64_t ld, int64_t M, int64_t N, const Tensor& out) {
  check_cuda(g, "g");
  check_f32(out, "out");
  bool f32 = g.scalar_type() == at::kFloat;
  TORCH_CHECK(f32 || g.scalar_type() == kAct, "hcb.colsum: dtype");
  // the kernel reads whole 8-column vectors: rows padded to 8 columns, 16-byte aligned
  TORCH_CHECK(ld % 8 == 0 && ld >= ((N + 7) / 8) * 8, "hcb.colsum: ld must be a multiple of 8 covering N");
  check_range(g, ((M - 1) * ld + ((N + 7) / 8) * 8) * (f32 ? 4 : 2), "g");
  check_align16(g.data_ptr(), "g");
  TORCH_CHECK(out.numel() >= N, "hcb.colsum: out too small");
  hcb::launch_colsum2(g.data_ptr(), (int)ld, (int)M, (int)N, f32 ? 1 : 0, out.data_ptr<float>(), cur_stream());
}

void sgd_momentum(const Tensor& w, const Tensor& mom, const Tensor& g, int64_t n_decay, const Tensor& hyper,
                  const c10::optional<Tensor>& l2, bool nesterov) {
  check_f32(w, "w");
  check_f32(mom, "mom");
  check_f32(g, "g");
  check_f32(hyper, "hyper");
  TORCH_CHECK(w.is_contiguous() && mom.is_contiguous() && g.is_contiguous(), "hcb.sgd_momentum: contiguous");
  TORCH_CHECK(w.numel() == mom.numel() && w.numel() == g.numel(), "hcb.sgd_momentum: sizes");
  check_align16(w.data_ptr(), "w");
  check_align16(mom.data_ptr(), "mom");
  check_align16(g.data_ptr(), "g");
  int slots = 0;
  if (l2.has_value()) {  // 1 slot: atomic sum (caller zeroes); more: per-block partials (loss_total sums)
    check_f32(*l2, "l2");
    slots = (int)l2->numel();
    TORCH_CHECK(l2->is_contiguous() && (slots == 1 || slots >= hcb::sgd_grid(w.numel())),
                "hcb.sgd_momentum: l2 must hold 1 or >= ", hcb::sgd_grid(w.numel()), " floats");
  }
  hcb::launch_sgd_momentum(w.data_ptr<float>(), mom.data_ptr<float>(), g.data_ptr<float>(), w.numel(),
                           n_decay, hyper.data_ptr<float>(), l2.has_value() ? l2->data_ptr<float>() : nullptr,
                           slots, nesterov ? 1 : 0, (int)hyper.numel(), cur_stream());
}

// the checks the two-slot optimizers share with sgd_momentum; returns the l2 slot count
int check_opt2(const char* op, const Tensor& w, const Tensor& s1, const Tensor& s2, const Tensor& g,
               const Tensor& hyper, const Tensor& ohyper, const c10::optional<Tensor>& l2) {
  check_f32(w, "w");
  check_f32(s1, "slot");
  check_f32(s2, "slot2");
  check_f32(g, "g");
  check_f32(hyper, "hyper");
  check_f32(ohyper, "ohyper");
  TORCH_CHECK(w.is_contiguous() && s1.is_contiguous() && s2.is_contiguous() && g.is_contiguous(), "hcb.", op,
              ": contiguous");
  TORCH_CHECK(w.numel() == s1.numel() && w.numel() == s2.numel() && w.numel() == g.numel(), "hcb.", op, ": sizes");
  check_align16(w.data_ptr(), "w");
  check_align16(s1.data_ptr(), "slot");
  check_align16(s2.data_ptr(), "slot2");
  check_align16(g.data_ptr(), "g");
  TORCH_CHECK(hyper.numel() >= 4 && hyper.is_contiguous(), "hcb.", op, ": hyper[>=4]");
  TORCH_CHECK(ohyper.numel() >= 3 && ohyper.is_contiguous(), "hcb.", op, ": ohyper[>=3]");
  int slots = 0;
  if (l2.has_value()) {
    check_f32(*l2, "l2");
    slots = (int)l2->numel();
    TORCH_CHECK(l2->is_contiguous() && (slots == 1 || slots >= hcb::sgd_grid(w.numel())), "hcb.", op,
                ": l2 must hold 1 or >= ", hcb::sgd_grid(w.numel()), " floats");
  }
  return slots;
}

void rmsprop(const Tensor& w, const Tensor& mom, const Tensor& ms, const Tensor& g, int64_t n_decay,
             const Tensor& hyper, const Tensor& ohyper, const c10::optional<Tensor>& l2) {
  const int slots = check_opt2("rmsprop", w, mom, ms, g, hyper, ohyper, l2);
  hcb::launch_rmsprop(w.data_ptr<float>(), mom.data_ptr<float>(), ms.data_ptr<float>(), g.data_ptr<float>(),
                      w.numel(), n_decay, hyper.data_ptr<float>(), ohyper.data_ptr<float>(),
                      l2.has_value() ? l2->data_ptr<float>() : nullptr, slots, (int)hyper.numel(), cur_stream());
}

void adam(const Tensor& w, const Tensor& m, const Tensor& v, const Tensor& g, int64_t n_decay, const Tensor& hyper,
          const Tensor& ohyper, const Tensor& state, const c10::optional<Tensor>& l2) {
  const int slots = check_opt2("adam", w, m, v, g, hyper, ohyper, l2);
  check_f32(state, "state");
  TORCH_CHECK(state.numel() >= 2 && state.is_contiguous(), "hcb.adam: state[2]");
  hcb::launch_adam(w.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(), g.data_ptr<float>(), w.numel(),
                   n_decay, hyper.data_ptr<float>(), ohyper.data_ptr<float>(), state.data_ptr<float>(),
                   l2.has_value() ? l2->data_ptr<float>() : nullptr, slots, (int)hyper.numel(), cur_stream());
}

void adam_advance(const Tensor& state, const Tensor& ohyper, const Tensor& hyper) {
  check_f32(state, "state");
  check_f32(ohyper, "ohyper");
  check_f32(hyper, "hyper");
  TORCH_CHECK(state.numel() >= 2 && state.is_contiguous(), "hcb.adam_advance: state[2]");
  TORCH_CHECK(ohyper.numel() >= 3 && ohyper.is_contiguous(), "hcb.adam_advance: ohyper[>=3]");
  TORCH_CHECK(hyper.numel() >= 4 && hyper.is_contiguous(), "hcb.adam_advance: hyper[>=4]");
  hcb::launch_adam_advance(state.data_ptr<float>(), ohyper.data_ptr<float>(), hyper.data_ptr<float>(),
                           (int)hyper.numel(), cur_stream());
}

void weight_pack(const Tensor& master, const Tensor& pack, const Tensor& table, int64_t max_work, int64_t lo) {
  check_f32(master, "master");
  int64_t pstride = 0;
  if (lo == 3) {  // all three planes: pack is [3][n] bf16 (plane t at t * stride(0))
    pstride = check_planes(pack, "pack");
    TORCH_CHECK(pack.dim() == 2, "hcb.weight_pack: planes [3][n]");
  } else {
    TORCH_CHECK(lo >= 0 && lo <= 2, "hcb.weight_pack: lo 0..3");
    check_act(pack, "pack");
  }
  check_cuda(table, "table");
  TORCH_CHECK(table.scalar_type() == at::kLong && table.dim() == 2 && table.size(1) == 9, "hcb.weight_pack: table [n][9] int64");
  TORCH_CHECK(table.is_contiguous(), "hcb.weight_pack: table contiguous");
  hcb::launch_weight_pack(master.data_ptr<float>(), (uint16_t*)pack.data_ptr(),
                          reinterpret_cast<const hcb::WPackEntry*>(table.data_ptr<int64_t>()),
                          (int)table.size(0), max_work, cur_stream(), (int)lo, pstride);
}

void add_bf16(const Tensor& a, const Tensor& b, const Tensor& y) {
  check_act(a, "a");
  check_act(b, "b");
  check_act(y, "y");
  TORCH_CHECK(a.numel() == b.numel() && a.numel() == y.numel() && a.numel() % 8 == 0, "hcb.add_bf16: sizes");
  TORCH_CHECK(a.is_contiguous() && b.is_contiguous() && y.is_contiguous(), "hcb.add_bf16: contiguous");
  hcb::launch_add_bf16(a.data_ptr(), b.data_ptr(), y.data_ptr(), a.numel(), cur_stream());
}

// ---- finalize-free BN (statistics in R replicas of [2][C], fp32 atomics)
void bn_apply_acc(const Tensor& x, int64_t ldx, const Tensor& y, int64_t ldy, const c10::optional<Tensor>& res,
                  int64_t ldr, int64_t M, int64_t C, const Tensor& acc, int64_t R, double eps, double momentum,
                  const Tensor& gamma, const Tensor& beta, int64_t relu, const Tensor& saved_mean,
                  const Tensor& saved_invstd, const c10::optional<Tensor>& rm, const c10::optional<Tensor>& rv,
                  const c10::optional<Tensor>& shift, const c10::optional<Tensor>& res_acc, const c10::optional<Tensor>& res_gamma,
                  const c10::optional<Tensor>& res_beta, const c10::optional<Tensor>& res_saved_mean,
                  const c10::optional<Tensor>& res_saved_invstd, const c10::optional<Tensor>& res_rm,
                  const c10::optional<Tensor>& res_rv, const c10::optional<Tensor>& res_shift,
                  c10::optional<double> act_max) {
  const bool f32 = check_act_or_f32(x, "x");
  // fp32 z with a bf16 y: y is written as [3, ...] bf16 planes; a bf16 residual is planes too
  const bool yp3 = f32 && y.scalar_type() == at::kBFloat16;
  const int64_t yps = yp3 ? check_planes(y, "y") : 0;
  if (!yp3) same_act(x, y, "y");
  int64_t rps = 0;
  const int64_t e = f32 ? 4 : 2;
  check_f32(acc, "acc");
  TORCH_CHECK(C % 8 == 0 && C <= 2048 && ldx % 8 == 0 && ldy % 8 == 0 && R >= 1, "hcb.bn_apply_acc: C/ld/R");
  TORCH_CHECK(acc.numel() >= R * 2 * C && saved_mean.numel() >= C && saved_invstd.numel() >= C, "hcb.bn_apply_acc: sizes");
  check_range(x, ((M - 1) * ldx + C) * e, "x");
  check_range(y, yp3 ? (2 * yps + (M - 1) * ldy + C) * 2 : ((M - 1) * ldy + C) * e, "y");
  const void* rp = nullptr;
  if (res.has_value()) {
    TORCH_CHECK(ldr % 8 == 0, "hcb.bn_apply_acc: ldr");
    if (yp3 && res->scalar_type() == at::kBFloat16) {
      TORCH_CHECK(!res_acc.has_value(), "hcb.bn_apply_acc: a residual BN reads the fp32 z_sc, not planes");
      rps = check_planes(*res, "res");
      check_range(*res, (2 * rps + (M - 1) * ldr + C) * 2, "res");
    } else {
      same_act(x, *res, "res");
      check_range(*res, ((M - 1) * ldr + C) * e, "res");
      TORCH_CHECK(!yp3 || res_acc.has_value(), "hcb.bn_apply_acc: a plain fp32-path residual must be planes");
    }
    rp = res->data_ptr();
  }
  // residual BN (projection shortcut): the residual is that BN's raw input z_sc
  hcb::ResBN rb{};
  if (res_acc.has_value()) {
    TORCH_CHECK(rp != nullptr && res_gamma && res_beta && res_saved_mean && res_saved_invstd,
                "hcb.bn_apply_acc: a residual BN needs res plus its acc / gamma / beta / saved stats");
    rb.acc = opt_f32(res_acc, R * 2 * C, "res_acc");
    rb.gamma = opt_f32(res_gamma, C, "res_gamma");
    rb.beta = opt_f32(res_beta, C, "res_beta");
    rb.saved_mean = const_cast<float*>(opt_f32(res_saved_mean, C, "res_saved_mean"));
    rb.saved_invstd = const_cast<float*>(opt_f32(res_saved_invstd, C, "res_saved_invstd"));
    rb.run_mean = const_cast<float*>(opt_f32(res_rm, C, "res_running_mean"));
    rb.run_var = const_cast<float*>(opt_f32(res_rv, C, "res_running_var"));
    TORCH_CHECK((rb.run_mean == nullptr) == (rb.run_var == nullptr), "hcb.bn_apply_acc: residual running stats");
    rb.shift = opt_f32(res_shift, C, "res_shift");
  }
  hcb::launch_bn_apply_acc(x.data_ptr(), (int)ldx, y.data_ptr(), (int)ldy, rp, (int)ldr, (int)M, (int)C,
                           acc.data_ptr<float>(), (int)R, (float)eps, (float)momentum, gamma.data_ptr<float>(),
                           beta.data_ptr<float>(), relu_code(relu, act_max), saved_mean.data_ptr<float>(),
                           saved_invstd.data_ptr<float>(), rm.has_value() ? rm->data_ptr<float>() : nullptr,
                           rv.has_value() ? rv->data_ptr<float>() : nullptr, opt_f32(shift, C, "shift"),
                           res_acc.has_value() ? &rb : nullptr, cur_stream(), f32, yps, rps,
                           (float)act_max.value_or(0.0));
}

// pooled-gradient source (pool_amax / pool_geom = [H, W, P, Q, k, s, pt, pl]): dy is the max-pool
// gradient [N][P][Q] (row stride lddy) and amax its window-local argmax [N][P][Q][C]; returns the
// number of dy rows to range-check
int64_t pool_src(hcb::PoolSrc& ps, const Tensor& dy, int64_t lddy, int64_t M, int64_t C,
                 const c10::optional<Tensor>& amax, at::OptionalIntArrayRef geom) {
  TORCH_CHECK(amax.has_value() == geom.has_value(), "hcb.bn_bwd: pool_amax and pool_geom go together");
  if (!amax.has_value()) return M;
  TORCH_CHECK(geom->size() == 8, "hcb.bn_bwd: pool_geom = [H, W, P, Q, k, s, pt, pl]");
  const auto g = *geom;
  ps.H = (int)g[0]; ps.W = (int)g[1]; ps.P = (int)g[2]; ps.Q = (int)g[3];
  ps.k = (int)g[4]; ps.s = (int)g[5]; ps.pt = (int)g[6]; ps.pl = (int)g[7];
  ps.C = (int)C;
  ps.ldp = (int)lddy;
  TORCH_CHECK(ps.H > 0 && ps.W > 0 && M % ((int64_t)ps.H * ps.W) == 0, "hcb.bn_bwd: M vs H x W");
  TORCH_CHECK(ps.s >= 1 && ps.k >= 1 && ps.k <= 2 * ps.s && ps.pt >= 0 && ps.pl >= 0 && ps.pt < ps.k && ps.pl < ps.k,
              "hcb.bn_bwd: pool windows must overlap at most 2 x 2 per pixel");
  const int64_t N = M / ((int64_t)ps.H * ps.W), rows = N * ps.P * ps.Q;
  TORCH_CHECK(amax->scalar_type() == at::kByte && amax->is_cuda() && amax->is_contiguous() &&
                  amax->numel() >= rows * C, "hcb.bn_bwd: pool_amax must be uint8 [N][P][Q][C]");
  TORCH_CHECK(lddy % 8 == 0, "hcb.bn_bwd: pooled dy row stride");
  ps.dyp = dy.data_ptr();
  ps.amax = amax->data_ptr<uint8_t>();
  return rows;
}

void bn_bwd_reduce_acc(const Tensor& dy, int64_t lddy, const c10::optional<Tensor>& y, int64_t ldyv,
                       const Tensor& x, int64_t ldx, int64_t M, int64_t C, const Tensor& mean, const Tensor& invstd,
                       const Tensor& gamma, const Tensor& beta, int64_t relu, const Tensor& acc, int64_t R,
                       const c10::optional<Tensor>& gout, int64_t ldg, const c10::optional<Tensor>& pool_amax,
                       at::OptionalIntArrayRef pool_geom) {
  const bool f32 = check_act_or_f32(dy, "dy");
  same_act(dy, x, "x");
  const int64_t e = f32 ? 4 : 2;
  check_f32(acc, "acc");
  TORCH_CHECK(C % 8 == 0 && C <= 2048 && R >= 1 && acc.numel() >= R * 2 * C, "hcb.bn_bwd_reduce_acc: C/R");
  hcb::PoolSrc ps{};
  const int64_t dyrows = pool_src(ps, dy, lddy, M, C, pool_amax, pool_geom);
  TORCH_CHECK(!pool_amax.has_value() || (!gout.has_value() && relu != 1), "hcb.bn_bwd_reduce_acc: pooled dy: no gout / y");
  check_range(dy, ((dyrows - 1) * lddy + C) * e, "dy");
  check_range(x, ((M - 1) * ldx + C) * e, "x");
  const void* yp = nullptr;
  bool yh = false;  // fp32 path: y given as its bf16 planes, the mask read from the hi plane
  if (relu == 1) {
    TORCH_CHECK(y.has_value(), "hcb.bn_bwd_reduce_acc: relu=1 needs y");
    yh = f32 && y->scalar_type() == at::kBFloat16;
    if (yh) {
      check_planes(*y, "y");
      check_range(*y, ((M - 1) * ldyv + C) * 2, "y");
    } else {
      same_act(dy, *y, "y");
      check_range(*y, ((M - 1) * ldyv + C) * e, "y");
    }
    yp = y->data_ptr();
  }
  void* gp = nullptr;
  if (gout.has_value()) {
    same_act(dy, *gout, "gout");
    check_range(*gout, ((M - 1) * ldg + C) * e, "gout");
    gp = gout->data_ptr();
  }
  hcb::launch_bn_bwd_reduce_acc(dy.data_ptr(), (int)lddy, yp, (int)ldyv, x.data_ptr(), (int)ldx, (int)M, (int)C,
                                mean.data_ptr<float>(), invstd.data_ptr<float>(), gamma.data_ptr<float>(),
                                beta.data_ptr<float>(), (int)relu, acc.data_ptr<float>(), (int)R, gp, (int)ldg,
                                cur_stream(), f32, yh, pool_amax.has_value() ? &ps : nullptr);
}

void bn_bwd_apply_acc(const Tensor& dy, int64_t lddy, const c10::optional<Tensor>& y, int64_t ldyv,
                      const Tensor& x, int64_t ldx, const Tensor& dx, int64_t lddx, int64_t M, int64_t C,
                      const Tensor& mean, const Tensor& invstd, const Tensor& gamma, const Tensor& beta,
                      const Tensor& acc, int64_t R, const Tensor& dgamma, const Tensor& dbeta, int64_t relu,
                      const c10::optional<Tensor>& shift_out, const c10::optional<Tensor>& pool_amax,
                      at::OptionalIntArrayRef pool_geom, const c10::optional<Tensor>& add, int64_t ldadd) {
  const bool f32 = check_act_or_f32(dy, "dy");
  same_act(dy, x, "x");
  // fp32 dy with a bf16 dx: dx is written as [3, ...] bf16 planes (the data / weight-gradient
  // GEMM operand format)
  const bool dp3 = f32 && dx.scalar_type() == at::kBFloat16;
  const int64_t dxps = dp3 ? check_planes(dx, "dx") : 0;
  if (!dp3) same_act(dy, dx, "dx");
  const int64_t e = f32 ? 4 : 2;
  if (add.has_value()) {  // dx = BN'(dy) + add: plain dx (no planes), no pooled dy
    same_act(dy, *add, "add");
    TORCH_CHECK(!dp3 && !pool_amax.has_value() && ldadd % 8 == 0, "hcb.bn_bwd_apply_acc: add needs a plain dx");
    check_range(*add, ((M - 1) * ldadd + C) * e, "add");
  }
  check_f32(acc, "acc");
  TORCH_CHECK(C % 8 == 0 && C <= 2048 && R >= 1 && acc.numel() >= R * 2 * C, "hcb.bn_bwd_apply_acc: C/R");
  hcb::PoolSrc ps{};
  const int64_t dyrows = pool_src(ps, dy, lddy, M, C, pool_amax, pool_geom);
  TORCH_CHECK(!pool_amax.has_value() || (relu != 1 && dp3 == f32), "hcb.bn_bwd_apply_acc: pooled dy: no y; fp32 writes planes");
  check_range(dy, ((dyrows - 1) * lddy + C) * e, "dy");
  check_range(x, ((M - 1) * ldx + C) * e, "x");
  check_range(dx, dp3 ? (2 * dxps + (M - 1) * lddx + C) * 2 : ((M - 1) * lddx + C) * e, "dx");
  const void* yp = nullptr;
  bool yh = false;
  if (relu == 1) {
    TORCH_CHECK(y.has_value(), "hcb.bn_bwd_apply_acc: relu=1 needs y");
    yh = f32 && y->scalar_type() == at::kBFloat16;
    if (yh) {
      check_planes(*y, "y");
      check_range(*y, ((M - 1) * ldyv + C) * 2, "y");
    } else {
      same_act(dy, *y, "y");
      check_range(*y, ((M - 1) * ldyv + C) * e, "y");
    }
    yp = y->data_ptr();
  }
  hcb::launch_bn_bwd_apply_acc(dy.data_ptr(), (int)lddy, yp, (int)ldyv, x.data_ptr(), (int)ldx, dx.data_ptr(),
                               (int)lddx, (int)M, (int)C, mean.data_ptr<float>(), invstd.data_ptr<float>(),
                               gamma.data_ptr<float>(), beta.data_ptr<float>(), acc.data_ptr<float>(), (int)R,
                               dgamma.data_ptr<float>(), dbeta.data_ptr<float>(), (int)relu,
                               const_cast<float*>(opt_f32(shift_out, C, "shift_out")), cur_stream(), f32, yh, dxps,
                               pool_amax.has_value() ? &ps : nullptr, add.has_value() ? add->data_ptr() : nullptr,
                               (int)ldadd);
}

void bn_stats_acc(const Tensor& x, int64_t ldx, int64_t M, int64_t C, const Tensor& acc, int64_t R,
                  const c10::optional<Tensor>& shift) {
  const bool f32 = check_act_or_f32(x, "x");
  check_f32(acc, "acc");
  TORCH_CHECK(C % 8 == 0 && C <= 2048 && ldx % 8 == 0 && ldx >= C && R >= 1 && M >= 1, "hcb.bn_stats_acc: C/ld/R");
  TORCH_CHECK(acc.numel() >= R * 2 * C, "hcb.bn_stats_acc: acc too small");
  check_range(x, ((M - 1) * ldx + C) * (f32 ? 4 : 2), "x");
  hcb::launch_bn_stats_acc(x.data_ptr(), (int)ldx, (int)M, (int)C, opt_f32(shift, C, "shift"), acc.data_ptr<float>(),
                           (int)R, cur_stream(), f32);
}

// ---- depthwise 3x3 conv (dwconv.hip). geom = [N, H, W, C, ldx, P, Q, ldz, sh, sw, pt, pl]: x / dx
// [N,H,W,C] with row stride ldx, z / dz [N,P,Q,C] with row stride ldz, w fp32 [C,3,3]
hcb::DwParams dw_params(at::IntArrayRef g, const Tensor& x, const Tensor& z, const Tensor& w, bool* f32,
                        const char* op) {
  TORCH_CHECK(g.size() == 12, "hcb.", op, ": geom = [N, H, W, C, ldx, P, Q, ldz, sh, sw, pt, pl]");
  *f32 = check_act_or_f32(x, "x");
  same_act(x, z, "z");
  check_f32(w, "w");
  const int64_t N = g[0], H = g[1], W = g[2], C = g[3], ldx = g[4], P = g[5], Q = g[6], ldz = g[7];
  const int64_t sh = g[8], sw = g[9], pt = g[10], pl = g[11];
  const int64_t e = *f32 ? 4 : 2;
  TORCH_CHECK(N >= 1 && H >= 1 && W >= 1 && P >= 1 && Q >= 1, "hcb.", op, ": empty tensor");
  TORCH_CHECK(C >= 8 && C % 8 == 0, "hcb.", op, ": C must be a multiple of 8, got ", C);
  TORCH_CHECK(ldx % 8 == 0 && ldz % 8 == 0 && ldx >= C && ldz >= C, "hcb.", op, ": row strides (multiples of 8, >= C)");
  TORCH_CHECK(sh == sw && (sh == 1 || sh == 2), "hcb.", op, ": stride 1 or 2");
  TORCH_CHECK(pt >= 0 && pt <= 1 && pl >= 0 && pl <= 1, "hcb.", op, ": top / left pads in {0, 1}");
  TORCH_CHECK((P - 1) * sh - pt < H && (Q - 1) * sw - pl < W, "hcb.", op, ": output larger than the padded input allows");
  const int64_t xb = ((N * H * W - 1) * ldx + C) * e, zb = ((N * P * Q - 1) * ldz + C) * e;
  TORCH_CHECK(xb < (1ll << 31) && zb < (1ll << 31), "hcb.", op, ": tensors must stay below 2 GiB (32-bit offsets)");
  check_range(x, xb, "x");
  check_range(z, zb, "z");
  TORCH_CHECK(w.is_contiguous() && w.numel() == 9 * C, "hcb.", op, ": w must be contiguous fp32 [C, 3, 3]");
  check_align16(x.data_ptr(), "x");
  check_align16(z.data_ptr(), "z");
  check_align16(w.data_ptr(), "w");
  hcb::DwParams p{};
  p.x = x.data_ptr();
  p.z = z.data_ptr();
  p.w = w.data_ptr<float>();
  p.N = (int)N; p.H = (int)H; p.W = (int)W; p.C = (int)C; p.ldx = (int)ldx;
  p.P = (int)P; p.Q = (int)Q; p.ldz = (int)ldz; p.S = (int)sh; p.pt = (int)pt; p.pl = (int)pl;
  return p;
}

void dwconv_fwd(const Tensor& x, const Tensor& w, const Tensor& z, at::IntArrayRef g,
                const c10::optional<Tensor>& stats, int64_t R, const c10::optional<Tensor>& shift) {
  bool f32;
  hcb::DwParams p = dw_params(g, x, z, w, &f32, "dwconv_fwd");
  if (stats.has_value()) {
    TORCH_CHECK(R >= 1, "hcb.dwconv_fwd: stats_R");
    p.stats = const_cast<float*>(opt_f32(stats, R * 2 * p.C, "stats"));
    p.R = (int)R;
    p.shift = opt_f32(shift, p.C, "stats_shift");
  }
  hcb::launch_dwconv_fwd(p, cur_stream(), f32);
}

void dwconv_dgrad(const Tensor& dz, const Tensor& w, const Tensor& dx, at::IntArrayRef g, bool accumulate) {
  bool f32;
  hcb::DwParams p = dw_params(g, dx, dz, w, &f32, "dwconv_dgrad");
  p.accumulate = accumulate ? 1 : 0;
  hcb::launch_dwconv_dgrad(p, cur_stream(), f32);
}

int64_t dwconv_wgrad_blocks(at::IntArrayRef g) {
  TORCH_CHECK(g.size() == 12 && g[3] >= 8 && g[3] % 8 == 0 && g[0] * g[5] * g[6] >= 1 &&
                  g[0] * g[5] * g[6] < (1ll << 31), "hcb.dwconv_wgrad_blocks: geom");
  return hcb::dwconv_wgrad_blocks((int)g[0], (int)g[5], (int)g[6], (int)g[3]);
}

void dwconv_wgrad(const Tensor& dz, const Tensor& x, const Tensor& ws, const Tensor& dw, at::IntArrayRef g) {
  bool f32;
  check_f32(dw, "dw");
  hcb::DwParams p = dw_params(g, x, dz, dw, &f32, "dwconv_wgrad");  // (dw checked as the [C, 3, 3] weight is)
  p.w = nullptr;
  check_f32(ws, "ws");
  const int64_t nblk = hcb::dwconv_wgrad_blocks(p.N, p.P, p.Q, p.C);
  TORCH_CHECK(ws.is_contiguous() && ws.numel() >= nblk * 9 * p.C, "hcb.dwconv_wgrad: the workspace holds ", ws.numel(),
              " floats, this problem needs ", nblk * 9 * p.C, " (dwconv_wgrad_blocks * 9 * C)");
  check_align16(ws.data_ptr(), "ws");
  hcb::launch_dwconv_wgrad(p, ws.data_ptr<float>(), (int)nblk, dw.data_ptr<float>(), cur_stream(), f32);
}

void relu_bwd(const Tensor& dy, const Tensor& y, const Tensor& dz) {
  const bool f32 = check_act_or_f32(dy, "dy");
  same_act(dy, y, "y");
  same_act(dy, dz, "dz");
  TORCH_CHECK(dy.numel() == y.numel() && dy.numel() == dz.numel() && dy.numel() % 8 == 0, "hcb.relu_bwd: sizes");
  TORCH_CHECK(dy.is_contiguous() && y.is_contiguous() && dz.is_contiguous(), "hcb.relu_bwd: contiguous");
  hcb::launch_relu_bwd(dy.data_ptr(), y.data_ptr(), dz.data_ptr(), dy.numel(), cur_stream(), f32);
}

void dropout_fwd(const Tensor& x, const Tensor& y, const Tensor& mask, double keep, int64_t seed, const Tensor& step) {
  const bool f32 = check_act_or_f32(x, "x");
  same_act(x, y, "y");
  check_cuda(mask, "mask");
  check_cuda(step, "step");
  TORCH_CHECK(x.is_contiguous() && y.is_contiguous() && mask.is_contiguous(), "hcb.dropout_fwd: contiguous");
  TORCH_CHECK(x.numel() == y.numel() && x.numel() % 8 == 0 && mask.scalar_type() == at::kByte &&
                  mask.numel() * 8 >= x.numel(),
              "hcb.dropout_fwd: sizes (mask: one bit per element)");
  TORCH_CHECK(step.scalar_type() == at::kLong && step.numel() >= 1, "hcb.dropout_fwd: step int64");
  TORCH_CHECK(keep > 0.0 && keep <= 1.0, "hcb.dropout_fwd: 0 < keep <= 1");
  hcb::launch_dropout_fwd(x.data_ptr(), y.data_ptr(), mask.data_ptr<uint8_t>(), x.numel(), (float)keep, (uint64_t)seed,
                          step.data_ptr<int64_t>(), cur_stream(), f32);
}

void dropout_bwd(const Tensor& dy, const Tensor& mask, const Tensor& dx, double keep) {
  const bool f32 = check_act_or_f32(dy, "dy");
  same_act(dy, dx, "dx");
  check_cuda(mask, "mask");
  TORCH_CHECK(dy.is_contiguous() && dx.is_contiguous() && mask.is_contiguous(), "hcb.dropout_bwd: contiguous");
  TORCH_CHECK(dy.numel() == dx.numel() && dy.numel() % 8 == 0 && mask.scalar_type() == at::kByte &&
                  mask.numel() * 8 >= dy.numel(),
              "hcb.dropout_bwd: sizes");
  TORCH_CHECK(keep > 0.0 && keep <= 1.0, "hcb.dropout_bwd: 0 < keep <= 1");
  hcb::launch_dropout_bwd(dy.data_ptr(), mask.data_ptr<uint8_t>(), dx.data_ptr(), dy.numel(), (float)keep, cur_stream(),
                          f32);
}

void synth_images(const Tensor& out, int64_t C, int64_t Cpad, double mean, double std, int64_t seed) {
  const bool f32 = check_act_or_f32(out, "out");
  TORCH_CHECK(out.numel() % Cpad == 0, "hcb.synth_images: numel % Cpad");
  hcb::launch_synth_images(out.data_ptr(), out.numel() / Cpad, (int)C, (int)Cpad, (float)mean, (float)std,
                           (uint64_t)seed, cur_stream(), f32);
}

void synth_labels(const Tensor& out, int64_t ncls, int64_t seed) {
  check_cuda(out, "out");
  TORCH_CHECK(out.scalar_type() == at::kLong, "hcb.synth_labels: int64");
  hcb::launch_synth_labels(out.data_ptr<int64_t>(), (int)out.numel(), (int)ncls, (uint64_t)seed, cur_stream());
}

// desc_host: the CPU copy of desc, used to check every crop lies inside src before launching
void preprocess_images(const Tensor& src, const Tensor& desc, const Tensor& desc_host, const Tensor& out,
                       at::ArrayRef<double> scale, at::ArrayRef<double> bias) {
  check_cuda(src, "src");
  check_cuda(desc, "desc");
  const bool f32 = check_act_or_f32(out, "out");  // the fp32 path's input is fp32
  TORCH_CHECK(src.scalar_type() == at::kByte && src.is_contiguous(), "hcb.preprocess_images: src uint8 contiguous");
  TORCH_CHECK(desc.scalar_type() == at::kLong && desc.dim() == 2 && desc.size(1) == 4 && desc.is_contiguous(),
              "hcb.preprocess_images: desc int64 [B][4]");
  TORCH_CHECK(!desc_host.is_cuda() && desc_host.scalar_type() == at::kLong && desc_host.is_contiguous() &&
                  desc_host.sizes() == desc.sizes(),
              "hcb.preprocess_images: desc_host must be the CPU copy of desc");
  TORCH_CHECK(out.dim() == 4 && out.is_contiguous() && out.size(1) == out.size(2) && out.size(3) % 8 == 0 &&
                  out.size(3) >= 8,
              "hcb.preprocess_images: out [B][S][S][Cpad] contiguous, Cpad % 8 == 0");
  TORCH_CHECK(scale.size() == 3 && bias.size() == 3, "hcb.preprocess_images: 3 scales / biases");
  const int64_t B = desc.size(0);
  TORCH_CHECK(B <= out.size(0), "hcb.preprocess_images: more crops than output images");
  const int64_t* d = desc_host.data_ptr<int64_t>();
  for (int64_t i = 0; i < B; ++i) {
    TORCH_CHECK(d[4 * i] >= 0 && d[4 * i + 1] > 0 && d[4 * i + 2] > 0 &&
                    d[4 * i] + d[4 * i + 1] * d[4 * i + 2] * 3 <= src.numel(),
                "hcb.preprocess_images: crop ", i, " outside the staging buffer");
  }
  TORCH_CHECK(out.size(1) * out.size(1) < (1ll << 31), "hcb.preprocess_images: image too large");
  const float sc[3] = {(float)scale[0], (float)scale[1], (float)scale[2]};
  const float bi[3] = {(float)bias[0], (float)bias[1], (float)bias[2]};
  if (B == 0) return;
  hcb::launch_preprocess_images(src.data_ptr<uint8_t>(), desc.data_ptr<int64_t>(), (int)B, out.data_ptr(),
                                (int)out.size(1), (int)out.size(3), sc, bi, f32, cur_stream());
}

// preprocess_images with a colour stage and a resize method per image (kernels/distort.hip). params
// [B][8] float32 = brightness delta, saturation factor, hue delta, contrast factor, ordering (-1 | 0 | 1),
// method (0..3), 0, 0; desc_host / params_host: the CPU copies, checked here before anything is launched.
// work: at least B * ceil(S*S / 256) * 4 float32 of scratch, no need to clear it
void preprocess_distort(const Tensor& src, const Tensor& desc, const Tensor& desc_host, const Tensor& params,
                        const Tensor& params_host, const Tensor& out, const Tensor& work, at::ArrayRef<double> scale,
                        at::ArrayRef<double> bias) {
  check_cuda(src, "src");
  check_cuda(desc, "desc");
  check_cuda(params, "params");
  check_cuda(work, "work");
  const bool f32 = check_act_or_f32(out, "out");
  TORCH_CHECK(src.scalar_type() == at::kByte && src.is_contiguous(), "hcb.preprocess_distort: src uint8 contiguous");
  TORCH_CHECK(desc.scalar_type() == at::kLong && desc.dim() == 2 && desc.size(1) == 4 && desc.is_contiguous(),
              "hcb.preprocess_distort: desc int64 [B][4]");
  TORCH_CHECK(!desc_host.is_cuda() && desc_host.scalar_type() == at::kLong && desc_host.is_contiguous() &&
                  desc_host.sizes() == desc.sizes(),
              "hcb.preprocess_distort: desc_host must be the CPU copy of desc");
  const int64_t B = desc.size(0);
  TORCH_CHECK(params.scalar_type() == at::kFloat && params.dim() == 2 && params.size(0) == B && params.size(1) == 8 &&
                  params.is_contiguous(),
              "hcb.preprocess_distort: params float32 [B][8]");
  TORCH_CHECK(!params_host.is_cuda() && params_host.scalar_type() == at::kFloat && params_host.is_contiguous() &&
                  params_host.sizes() == params.sizes(),
              "hcb.preprocess_distort: params_host must be the CPU copy of params");
  TORCH_CHECK(out.dim() == 4 && out.is_contiguous() && out.size(1) == out.size(2) && out.size(3) % 8 == 0 &&
                  out.size(3) >= 8,
              "hcb.preprocess_distort: out [B][S][S][Cpad] contiguous, Cpad % 8 == 0");
  TORCH_CHECK(scale.size() == 3 && bias.size() == 3, "hcb.preprocess_distort: 3 scales / biases");
  TORCH_CHECK(B <= out.size(0), "hcb.preprocess_distort: more crops than output images");
  const int64_t S = out.size(1);
  TORCH_CHECK(S * S < (1ll << 31), "hcb.preprocess_distort: image too large");
  const int64_t* d = desc_host.data_ptr<int64_t>();
  const float* q = params_host.data_ptr<float>();
  bool any_colour = false;
  for (int64_t i = 0; i < B; ++i) {
    TORCH_CHECK(d[4 * i] >= 0 && d[4 * i + 1] > 0 && d[4 * i + 2] > 0 &&
                    d[4 * i] + d[4 * i + 1] * d[4 * i + 2] * 3 <= src.numel(),
                "hcb.preprocess_distort: crop ", i, " outside the staging buffer");
    // the nearest / bicubic / area index arithmetic forms (dst + 1) * in in 32 bits
    TORCH_CHECK(d[4 * i + 1] * S < (1ll << 31) && d[4 * i + 2] * S < (1ll << 31),
                "hcb.preprocess_distort: crop ", i, " too large");
    const float* r = q + 8 * i;
    for (int k = 0; k < 8; ++k)
      TORCH_CHECK(std::isfinite(r[k]), "hcb.preprocess_distort: parameter ", k, " of image ", i, " is not finite");
    TORCH_CHECK(r[5] == 0.f || r[5] == 1.f || r[5] == 2.f || r[5] == 3.f, "hcb.preprocess_distort: resize method of image ",
                i, " must be 0 (nearest), 1 (bilinear), 2 (bicubic) or 3 (area)");
    TORCH_CHECK(r[4] == -1.f || r[4] == 0.f || r[4] == 1.f, "hcb.preprocess_distort: colour ordering of image ", i,
                " must be -1 (none), 0 or 1");
    TORCH_CHECK(r[1] >= 0.f && r[3] >= 0.f, "hcb.preprocess_distort: saturation and contrast factors of image ", i,
                " must be >= 0");
    TORCH_CHECK(r[6] == 0.f && r[7] == 0.f, "hcb.preprocess_distort: the spare parameter slots of image ", i,
                " must be 0");
    any_colour |= r[4] >= 0.f;
  }
  TORCH_CHECK(work.scalar_type() == at::kFloat && work.is_contiguous() &&
                  work.numel() >= hcb::preprocess_distort_work_floats((int)B, (int)S),
              "hcb.preprocess_distort: work too small: float32, at least B * ceil(S*S / 256) * 4 = ",
              hcb::preprocess_distort_work_floats((int)B, (int)S), " elements");
  const float sc[3] = {(float)scale[0], (float)scale[1], (float)scale[2]};
  const float bi[3] = {(float)bias[0], (float)bias[1], (float)bias[2]};
  if (B == 0) return;
  hcb::launch_preprocess_distort(src.data_ptr<uint8_t>(), desc.data_ptr<int64_t>(), params.data_ptr<float>(),
                                 any_colour, (int)B, out.data_ptr(), work.data_ptr<float>(), (int)S, (int)out.size(3), sc,
                                 bi, f32, cur_stream());
}

// CIFAR-10 batch from the device-resident split (kernels/cifar.hip). desc [B][4] int32 = (index | -1, oy,
// ox, flip); desc_host: its CPU copy, every row range-checked here before anything is launched
void cifar_batch(const Tensor& data, const Tensor& labels_all, const Tensor& desc, const Tensor& desc_host,
                 const Tensor& out, const Tensor& labels_out) {
  check_cuda(data, "data");
  check_cuda(labels_all, "labels_all");
  check_cuda(desc, "desc");
  check_cuda(labels_out, "labels_out");
  const bool f32 = check_act_or_f32(out, "out");
  TORCH_CHECK(data.scalar_type() == at::kByte && data.is_contiguous() && data.dim() == 4 && data.size(1) == 3 &&
                  data.size(2) == 32 && data.size(3) == 32,
              "hcb.cifar_batch: data uint8 [N][3][32][32] contiguous");
  const int64_t N = data.size(0);
  TORCH_CHECK(N * 3072 < (1ll << 40), "hcb.cifar_batch: dataset too large");
  TORCH_CHECK(labels_all.scalar_type() == at::kLong && labels_all.is_contiguous() && labels_all.dim() == 1 &&
                  labels_all.size(0) == N,
              "hcb.cifar_batch: labels_all int64 [N] contiguous");
  TORCH_CHECK(desc.scalar_type() == at::kInt && desc.dim() == 2 && desc.size(1) == 4 && desc.is_contiguous(),
              "hcb.cifar_batch: desc int32 [B][4]");
  TORCH_CHECK(!desc_host.is_cuda() && desc_host.scalar_type() == at::kInt && desc_host.is_contiguous() &&
                  desc_host.sizes() == desc.sizes(),
              "hcb.cifar_batch: desc_host must be the CPU copy of desc");
  const int64_t B = desc.size(0);
  TORCH_CHECK(out.dim() == 4 && out.is_contiguous() && out.size(0) == B && out.size(1) == 32 && out.size(2) == 32 &&
                  out.size(3) % 8 == 0 && out.size(3) >= 8,
              "hcb.cifar_batch: out [B][32][32][Cpad] contiguous, Cpad % 8 == 0");
  TORCH_CHECK(labels_out.scalar_type() == at::kLong && labels_out.is_contiguous() && labels_out.dim() == 1 &&
                  labels_out.size(0) == B,
              "hcb.cifar_batch: labels_out int64 [B] contiguous");
  TORCH_CHECK(data.device() == out.device() && labels_all.device() == out.device() && desc.device() == out.device() &&
                  labels_out.device() == out.device(),
              "hcb.cifar_batch: data, labels_all, desc, out and labels_out on one device");
  TORCH_CHECK(B < 65536, "hcb.cifar_batch: batch too large");
  check_align16(out.data_ptr(), "out");
  const int* d = desc_host.data_ptr<int>();
  for (int64_t i = 0; i < B; ++i) {
    TORCH_CHECK(d[4 * i] >= -1 && d[4 * i] < N, "hcb.cifar_batch: index of row ", i, " outside [-1, N)");
    TORCH_CHECK(d[4 * i + 1] >= 0 && d[4 * i + 1] <= 8 && d[4 * i + 2] >= 0 && d[4 * i + 2] <= 8,
                "hcb.cifar_batch: crop offset of row ", i, " outside [0, 8]");
    TORCH_CHECK(d[4 * i + 3] == 0 || d[4 * i + 3] == 1, "hcb.cifar_batch: flip of row ", i, " must be 0 or 1");
  }
  if (B == 0) return;
  hcb::launch_cifar_batch(data.data_ptr<uint8_t>(), labels_all.data_ptr<int64_t>(), desc.data_ptr<int>(), (int)B,
                          out.data_ptr(), labels_out.data_ptr<int64_t>(), (int)out.size(3), f32, cur_stream());
}

// GPU JPEG decode, stage 1 (kernels/jpeg.hip): dequantise + 8x8 inverse DCT of every block of every image
// component in one launch. coef: the records jpeg_entropy_decode wrote (csrc/data/jpeg.h); segs [nseg][8] =
// (group0, nblocks, coefficient byte offset, record byte offset, quantisation table, plane byte offset, 0,
// 0); segs_host: its CPU copy, every row range-checked here before anything is launched
void jpeg_idct(const Tensor& coef, const Tensor& segs, const Tensor& segs_host, const Tensor& planes) {
  check_cuda(coef, "coef");
  check_cuda(segs, "segs");
  check_cuda(planes, "planes");
  TORCH_CHECK(coef.scalar_type() == at::kByte && coef.is_contiguous(), "hcb.jpeg_idct: coef uint8 contiguous");
  TORCH_CHECK(planes.scalar_type() == at::kByte && planes.is_contiguous(), "hcb.jpeg_idct: planes uint8 contiguous");
  TORCH_CHECK(segs.scalar_type() == at::kLong && segs.dim() == 2 && segs.size(1) == 8 && segs.is_contiguous(),
              "hcb.jpeg_idct: segs int64 [nseg][8]");
  TORCH_CHECK(!segs_host.is_cuda() && segs_host.scalar_type() == at::kLong && segs_host.is_contiguous() &&
                  segs_host.sizes() == segs.sizes(),
              "hcb.jpeg_idct: segs_host must be the CPU copy of segs");
  TORCH_CHECK(coef.device() == segs.device() && planes.device() == segs.device(),
              "hcb.jpeg_idct: coef, segs and planes on one device");
  check_align16(coef.data_ptr(), "coef");
  check_align16(planes.data_ptr(), "planes");
  const int64_t nseg = segs.size(0), G = hcb::jpeg_idct_group_blocks();
  TORCH_CHECK(nseg < (1ll << 24), "hcb.jpeg_idct: too many segments");
  const int64_t* s = segs_host.data_ptr<int64_t>();
  int64_t group = 0;
  for (int64_t i = 0; i < nseg; ++i) {
    const int64_t* r = s + 8 * i;
    TORCH_CHECK(r[1] > 0 && r[1] < (1ll << 31), "hcb.jpeg_idct: block count of segment ", i, " out of range");
    TORCH_CHECK(r[0] == group, "hcb.jpeg_idct: group prefix of segment ", i, " is ", r[0], ", expected ", group);
    TORCH_CHECK(r[2] >= 0 && r[2] % 16 == 0 && r[2] + r[1] * 128 <= coef.numel(),
                "hcb.jpeg_idct: coefficients of segment ", i, " outside coef (or not 16-byte aligned)");
    TORCH_CHECK(r[4] >= 0 && r[4] <= 3, "hcb.jpeg_idct: quantisation table index of segment ", i, " outside [0, 3]");
    TORCH_CHECK(r[3] >= 0 && r[3] % 16 == 0 && r[3] + 128 + 4 * 128 <= coef.numel(),
                "hcb.jpeg_idct: record of segment ", i, " outside coef (or not 16-byte aligned)");
    TORCH_CHECK(r[5] >= 0 && r[5] % 8 == 0 && r[5] + r[1] * 64 <= planes.numel(),
                "hcb.jpeg_idct: plane of segment ", i, " outside planes (or not 8-byte aligned)");
    TORCH_CHECK(r[6] == 0 && r[7] == 0, "hcb.jpeg_idct: the spare slots of segment ", i, " must be 0");
    group += (r[1] + G - 1) / G;
  }
  TORCH_CHECK(group < (1ll << 31), "hcb.jpeg_idct: too many blocks");
  if (nseg == 0) return;
  hcb::launch_jpeg_idct(segs.data_ptr<int64_t>(), (int)nseg, group, coef.data_ptr<uint8_t>(), planes.data_ptr<uint8_t>(),
                        cur_stream());
}

// GPU JPEG decode, stage 2 (kernels/jpeg.hip): chroma upsampling, YCbCr -> RGB, r x r box mean and crop, one
// thread per pixel of the packed crops in stage. imgs [B][24] = (ncomp | 0 = row skipped, r, hs, vs, H, W, y0,
// x0, 3 x (plane byte offset, bx0, by0, bw, bh), 0); desc [B][4] = (offset, h, w, flip) as preprocess_images
// reads it afterwards; imgs_host / desc_host: the CPU copies, every window range-checked here before launch
void jpeg_crop_rgb(const Tensor& planes, const Tensor& imgs, const Tensor& imgs_host, const Tensor& desc,
                   const Tensor& desc_host, const Tensor& stage) {
  check_cuda(planes, "planes");
  check_cuda(imgs, "imgs");
  check_cuda(desc, "desc");
  check_cuda(stage, "stage");
  TORCH_CHECK(planes.scalar_type() == at::kByte && planes.is_contiguous(), "hcb.jpeg_crop_rgb: planes uint8 contiguous");
  TORCH_CHECK(stage.scalar_type() == at::kByte && stage.is_contiguous(), "hcb.jpeg_crop_rgb: stage uint8 contiguous");
  TORCH_CHECK(imgs.scalar_type() == at::kLong && imgs.dim() == 2 && imgs.size(1) == 24 && imgs.is_contiguous(),
              "hcb.jpeg_crop_rgb: imgs int64 [B][24]");
  TORCH_CHECK(!imgs_host.is_cuda() && imgs_host.scalar_type() == at::kLong && imgs_host.is_contiguous() &&
                  imgs_host.sizes() == imgs.sizes(),
              "hcb.jpeg_crop_rgb: imgs_host must be the CPU copy of imgs");
  const int64_t B = imgs.size(0);
  TORCH_CHECK(desc.scalar_type() == at::kLong && desc.dim() == 2 && desc.size(0) == B && desc.size(1) == 4 &&
                  desc.is_contiguous(),
              "hcb.jpeg_crop_rgb: desc int64 [B][4]");
  TORCH_CHECK(!desc_host.is_cuda() && desc_host.scalar_type() == at::kLong && desc_host.is_contiguous() &&
                  desc_host.sizes() == desc.sizes(),
              "hcb.jpeg_crop_rgb: desc_host must be the CPU copy of desc");
  TORCH_CHECK(planes.device() == imgs.device() && desc.device() == imgs.device() && stage.device() == imgs.device(),
              "hcb.jpeg_crop_rgb: planes, imgs, desc and stage on one device");
  TORCH_CHECK(B < 65536, "hcb.jpeg_crop_rgb: batch too large");
  const int64_t* t = imgs_host.data_ptr<int64_t>();
  const int64_t* d = desc_host.data_ptr<int64_t>();
  int64_t max_pixels = 0;
  for (int64_t i = 0; i < B; ++i) {
    const int64_t* r = t + 24 * i;
    if (r[0] == 0) continue;
    const int64_t ncomp = r[0], red = r[1], hs = r[2], vs = r[3], H = r[4], W = r[5], y0 = r[6], x0 = r[7];
    const int64_t oh = d[4 * i + 1], ow = d[4 * i + 2];
    TORCH_CHECK(ncomp == 1 || ncomp == 3, "hcb.jpeg_crop_rgb: component count of image ", i, " must be 0, 1 or 3");
    TORCH_CHECK(red == 1 || red == 2 || red == 4 || red == 8, "hcb.jpeg_crop_rgb: reduction of image ", i,
                " must be 1, 2, 4 or 8");
    TORCH_CHECK((hs == 1 || hs == 2) && (vs == 1 || vs == 2) && (ncomp == 3 || (hs == 1 && vs == 1)),
                "hcb.jpeg_crop_rgb: sampling factors of image ", i, " must be 1 or 2 (1 for a grey image)");
    TORCH_CHECK(H > 0 && W > 0 && H <= 65535 && W <= 65535, "hcb.jpeg_crop_rgb: size of image ", i, " out of range");
    TORCH_CHECK(oh > 0 && ow > 0 && y0 >= 0 && x0 >= 0 && y0 + oh * red <= H && x0 + ow * red <= W,
                "hcb.jpeg_crop_rgb: crop window of image ", i, " outside the image");
    TORCH_CHECK(d[4 * i] >= 0 && d[4 * i] + oh * ow * 3 <= stage.numel(), "hcb.jpeg_crop_rgb: crop ", i,
                " outside the staging buffer");
    for (int64_t c = 0; c < ncomp; ++c) {
      const int64_t* f = r + 8 + 5 * c;
      const int64_t fh = c == 0 ? 1 : hs, fv = c == 0 ? 1 : vs;
      // samples of this plane the kernel reads: the crop, or its chroma taps clipped to the true plane
      int64_t xlo = x0, xhi = x0 + ow * red - 1, ylo = y0, yhi = y0 + oh * red - 1;
      if (fh == 2) {
        xlo = std::max<int64_t>((x0 >> 1) - 1, 0);
        xhi = std::min<int64_t>((xhi >> 1) + 1, (W + 1) / 2 - 1);
      }
      if (fv == 2) {
        ylo = std::max<int64_t>((y0 >> 1) - 1, 0);
        yhi = std::min<int64_t>((yhi >> 1) + 1, (H + 1) / 2 - 1);
      }
      TORCH_CHECK(f[1] >= 0 && f[2] >= 0 && f[3] > 0 && f[4] > 0 && f[3] <= 8192 && f[4] <= 8192 && f[1] <= 8192 &&
                      f[2] <= 8192 && f[1] * 8 <= xlo && xhi < (f[1] + f[3]) * 8 && f[2] * 8 <= ylo &&
                      yhi < (f[2] + f[4]) * 8,
                  "hcb.jpeg_crop_rgb: block window of image ", i, " component ", c, " does not cover its crop");
      TORCH_CHECK(f[0] >= 0 && f[0] + f[3] * f[4] * 64 <= planes.numel(), "hcb.jpeg_crop_rgb: plane of image ", i,
                  " component ", c, " outside planes");
    }
    TORCH_CHECK(oh * ow < (1ll << 31), "hcb.jpeg_crop_rgb: crop ", i, " too large");
    max_pixels = std::max(max_pixels, oh * ow);
  }
  if (max_pixels == 0) return;
  hcb::launch_jpeg_crop_rgb(imgs.data_ptr<int64_t>(), desc.data_ptr<int64_t>(), (int)B, max_pixels,
                            planes.data_ptr<uint8_t>(), stage.data_ptr<uint8_t>(), cur_stream());
}

// Plan-A shortcut (kernels/shortcut.hip): the geometry of x [N][H][W][C] (or its planes [3][N][H][W][C]) against
// y [N][P][Q][K] at stride s, in 16-byte vectors; refuses what the kernels do not do, by name
struct ShortcutGeom {
  int64_t NI;
  int H, W, P, Q, s, Cv, Kv, padv;
};
ShortcutGeom shortcut_geom(const Tensor& x, const Tensor& y, int64_t s, const char* op) {
  check_cuda(x, "x");
  check_cuda(y, "y");
  TORCH_CHECK(x.device() == y.device(), "hcb.", op, ": both tensors on one device");
  const auto dt = x.scalar_type();
  TORCH_CHECK(dt == y.scalar_type() && (dt == kAct || dt == at::kFloat || dt == at::kBFloat16),
              "hcb.", op, ": both tensors " HCB_ACT_NAME ", float32 or bfloat16 planes, of one dtype");
  TORCH_CHECK(x.dim() == y.dim() && (x.dim() == 4 || (x.dim() == 5 && dt == at::kBFloat16 && x.size(0) == 3)),
              "hcb.", op, ": [N][H][W][C] tensors, or bf16 planes [3][N][H][W][C]");
  TORCH_CHECK(x.is_contiguous() && y.is_contiguous(), "hcb.", op, ": contiguous tensors only");
  const int o = x.dim() - 4;
  TORCH_CHECK(y.size(0) == x.size(0) && y.size(o) == x.size(o), "hcb.", op, ": batch sizes differ");
  TORCH_CHECK(s == 1 || s == 2, "hcb.", op, ": stride 1 or 2");
  const int64_t H = x.size(o + 1), W = x.size(o + 2), C = x.size(o + 3);
  const int64_t P = y.size(o + 1), Q = y.size(o + 2), K = y.size(o + 3);
  TORCH_CHECK(H > 0 && W > 0 && H < (1 << 20) && W < (1 << 20), "hcb.", op, ": bad spatial size");
  TORCH_CHECK(P == (H + s - 1) / s && Q == (W + s - 1) / s, "hcb.", op, ": output is [ceil(H / s)][ceil(W / s)]");
  TORCH_CHECK(K >= C && (K - C) % 2 == 0, "hcb.", op, ": K - C must be even and >= 0 (a centred channel pad)");
  TORCH_CHECK(C % 8 == 0 && C > 0 && ((K - C) / 2) % 8 == 0, "hcb.", op,
              ": C % 8 == 0 and pad % 8 == 0 (pad = (K - C) / 2) only");
  const int64_t e = (int64_t)x.element_size();
  ShortcutGeom g;
  g.NI = x.numel() / (H * W * C);
  g.H = (int)H, g.W = (int)W, g.P = (int)P, g.Q = (int)Q, g.s = (int)s;
  g.Cv = (int)(C * e / 16), g.Kv = (int)(K * e / 16), g.padv = (int)((K - C) / 2 * e / 16);
  TORCH_CHECK((y.numel() * e / 16 + 255) / 256 < (1ll << 31) && (x.numel() * e / 16 + 255) / 256 < (1ll << 31),
              "hcb.", op, ": tensor too large");
  check_align16(x.data_ptr(), "x");
  check_align16(y.data_ptr(), "y");
  return g;
}

void shortcut_pad_fwd(const Tensor& x, const Tensor& y, int64_t s) {
  const ShortcutGeom g = shortcut_geom(x, y, s, "shortcut_pad_fwd");
  hcb::launch_shortcut_pad_fwd(x.data_ptr(), y.data_ptr(), g.NI, g.H, g.W, g.P, g.Q, g.s, g.Cv, g.Kv, g.padv, cur_stream());
}

// dx [N][H][W][C] = the adjoint applied to g [N][P][Q][K]: every element of dx is written
void shortcut_pad_bwd(const Tensor& g, const Tensor& dx, int64_t s) {
  TORCH_CHECK(g.dim() == 4, "hcb.shortcut_pad_bwd: the gradient is a plain [N][P][Q][K] activation");
  const ShortcutGeom q = shortcut_geom(dx, g, s, "shortcut_pad_bwd");
  hcb::launch_shortcut_pad_bwd(g.data_ptr(), dx.data_ptr(), q.NI, q.H, q.W, q.P, q.Q, q.s, q.Cv, q.Kv, q.padv, cur_stream());
}

// Local response normalisation (kernels/lrn.hip). A tensor is [N][H][W][C] of the build's 16-bit type
// (format 0) or fp32 (1), or bf16 planes [3][N][H][W][C] (2); returns the format and the logical shape
int lrn_format(const Tensor& t, const char* name, const char* op, std::vector<int64_t>* shape, int64_t* plane) {
  check_cuda(t, name);
  const auto dt = t.scalar_type();
  int f;
  if (t.dim() == 5) {
    TORCH_CHECK(dt == at::kBFloat16 && t.size(0) == 3, "hcb.", op, ": ", name,
                " has 5 dims but is not bf16 planes [3][N][H][W][C]");
    f = 2;
  } else {
    TORCH_CHECK(t.dim() == 4, "hcb.", op, ": ", name, " must be [N][H][W][C] (or bf16 planes [3][N][H][W][C])");
    TORCH_CHECK(dt == kAct || dt == at::kFloat, "hcb.", op, ": ", name, " must be " HCB_ACT_NAME " or float32");
    f = dt == kAct ? 0 : 1;
  }
  TORCH_CHECK(t.is_contiguous(), "hcb.", op, ": ", name, " must be contiguous (no strided views)");
  check_align16(t.data_ptr(), name);
  check_range(t, t.numel() * (int64_t)t.element_size(), name);
  *shape = t.sizes().vec();
  if (f == 2) shape->erase(shape->begin());
  *plane = f == 2 ? t.stride(0) : 0;
  return f;
}

hcb::LrnParams lrn_params(const std::vector<int64_t>& shape, int64_t r, double bias, double alpha, double beta,
                          const char* op) {
  const int64_t C = shape[3], M = shape[0] * shape[1] * shape[2];
  TORCH_CHECK(M >= 1, "hcb.", op, ": empty tensor");
  TORCH_CHECK(C >= 8 && C % 8 == 0, "hcb.", op, ": C must be a multiple of 8, got C = ", C);
  TORCH_CHECK(C <= 512, "hcb.", op, ": C must be <= 512 (the C / 8 lanes of a pixel share one wave), got C = ", C);
  TORCH_CHECK(r >= 1 && r <= 4, "hcb.", op, ": depth_radius r must be in 1..4 (a halo of one lane), got r = ", r);
  TORCH_CHECK(bias > 0 && std::isfinite(bias), "hcb.", op, ": bias must be > 0, got ", bias);
  TORCH_CHECK(alpha >= 0 && std::isfinite(alpha), "hcb.", op, ": alpha must be >= 0, got ", alpha);
  TORCH_CHECK(std::isfinite(beta), "hcb.", op, ": beta must be finite");
  TORCH_CHECK(M * C < (1ll << 40) && hcb::lrn_blocks(M, (int)C) < (1ll << 31), "hcb.", op, ": tensor too large");
  hcb::LrnParams p{};
  p.M = M;
  p.C = (int)C;
  p.r = (int)r;
  p.bias = (float)bias;
  p.alpha = (float)alpha;
  p.beta = (float)beta;
  p.pmode = beta == 0.75 ? 1 : (beta == 0.5 ? 2 : 0);
  return p;
}

void lrn_fwd(const Tensor& x, const Tensor& y, int64_t r, double bias, double alpha, double beta) {
  std::vector<int64_t> xs, ys;
  int64_t xpl, ypl;
  const int xf = lrn_format(x, "x", "lrn_fwd", &xs, &xpl), yf = lrn_format(y, "y", "lrn_fwd", &ys, &ypl);
  TORCH_CHECK(x.device() == y.device(), "hcb.lrn_fwd: both tensors on one device");
  TORCH_CHECK(xs == ys, "hcb.lrn_fwd: y must have x's shape");
  TORCH_CHECK((xf == 0) == (yf == 0), "hcb.lrn_fwd: a 16-bit x writes a 16-bit y; an fp32 or planes x writes fp32 or planes");
  hcb::LrnParams p = lrn_params(xs, r, bias, alpha, beta, "lrn_fwd");
  p.x = x.data_ptr();
  p.x_plane = xpl;
  p.out = y.data_ptr();
  p.out_plane = ypl;
  hcb::launch_lrn_fwd(p, xf, yf, cur_stream());
}

// dy / dx: plain activations (16-bit with a 16-bit x, fp32 with an fp32 or planes x); every element of dx is written
void lrn_bwd(const Tensor& dy, const Tensor& x, const Tensor& dx, int64_t r, double bias, double alpha, double beta) {
  std::vector<int64_t> xs, gs, ds;
  int64_t xpl, gpl, dpl;
  const int xf = lrn_format(x, "x", "lrn_bwd", &xs, &xpl);
  const int gf = lrn_format(dy, "dy", "lrn_bwd", &gs, &gpl), df = lrn_format(dx, "dx", "lrn_bwd", &ds, &dpl);
  TORCH_CHECK(x.device() == dy.device() && x.device() == dx.device(), "hcb.lrn_bwd: all tensors on one device");
  TORCH_CHECK(xs == gs && xs == ds, "hcb.lrn_bwd: dy and dx must have x's shape");
  TORCH_CHECK(gf == df && gf == (xf == 0 ? 0 : 1),
              "hcb.lrn_bwd: dy and dx are plain activations, 16-bit with a 16-bit x, float32 with an fp32 or planes x");
  hcb::LrnParams p = lrn_params(xs, r, bias, alpha, beta, "lrn_bwd");
  p.x = x.data_ptr();
  p.x_plane = xpl;
  p.dy = dy.data_ptr();
  p.out = dx.data_ptr();
  hcb::launch_lrn_bwd(p, xf, cur_stream());
}

static int pack_mode(const Tensor& t, const char* what) {
  switch (t.scalar_type()) {
    case at::kFloat: return 0;
    case at::kBFloat16: return 1;
    case at::kHalf: return 2;
    default: TORCH_CHECK(false, "hcb.", what, ": wire dtype must be float32, bfloat16 or float16");
  }
  return 0;
}

void bucket_pack(const Tensor& src, const Tensor& dst, double scale) {
  check_f32(src, "src");
  check_cuda(dst, "dst");
  TORCH_CHECK(dst.is_contiguous() && src.numel() == dst.numel(), "hcb.bucket_pack: sizes");
  hcb::launch_bucket_pack(src.data_ptr<float>(), dst.data_ptr(), src.numel(), (float)scale, pack_mode(dst, "bucket_pack"),
                          cur_stream());
}

void bucket_unpack(const Tensor& src, const Tensor& dst, double scale) {
  check_cuda(src, "src");
  check_f32(dst, "dst");
  TORCH_CHECK(src.is_contiguous() && src.numel() == dst.numel(), "hcb.bucket_unpack: sizes");
  hcb::launch_bucket_unpack(src.data_ptr(), dst.data_ptr<float>(), src.numel(), (float)scale,
                            pack_mode(src, "bucket_unpack"), cur_stream());
}

// ---- tensor fusion of the hvd API: scattered tensors <-> the flat fp32 fusion buffer, one launch.
// The table lives on the device, so its CONTENT cannot be checked here without a read-back: the
// host mirror it is uploaded from is validated where the layout is built and where rows are bound
// (parallel/fusion.py, FusionBuffer._validate: off + n within flat, off % 4 == 0, tag 0..2, slots
// disjoint, pointer aligned to the element size). Checked here: the table's shape / dtype / device
// and the flat buffer. A slice of rows (one bucket) is a valid table: prefixes are relative to row 0.
static int fusion_check(const Tensor& table, const Tensor& flat, const char* what) {
  check_cuda(table, "table");
  check_f32(flat, "flat");
  constexpr int64_t K = (int64_t)(sizeof(hcb::FusionEntry) / sizeof(int64_t));
  TORCH_CHECK(table.scalar_type() == at::kLong && table.dim() == 2 && table.size(1) == K && table.is_contiguous(),
              "hcb.", what, ": table must be a contiguous int64 [n][", K, "] tensor");
  TORCH_CHECK(flat.is_contiguous() && flat.device() == table.device(), "hcb.", what,
              ": flat must be contiguous and on the table's device");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(flat.data_ptr()) % 16 == 0, "hcb.", what, ": flat must be 16-byte aligned");
  TORCH_CHECK(table.size(0) < (1ll << 31), "hcb.", what, ": too many entries");
  return (int)table.size(0);
}
// every entry adds at most one partial chunk to numel / FUSION_CHUNK
static int64_t fusion_max_chunks(const Tensor& table, const Tensor& flat) {
  return flat.numel() / hcb::FUSION_CHUNK + table.size(0);
}

void fusion_pack(const Tensor& table, const Tensor& flat, double scale) {
  const int n = fusion_check(table, flat, "fusion_pack");
  hcb::launch_fusion_pack(reinterpret_cast<const hcb::FusionEntry*>(table.data_ptr<int64_t>()), n, flat.data_ptr<float>(),
                          fusion_max_chunks(table, flat), (float)scale, cur_stream());
}

void fusion_unpack(const Tensor& table, const Tensor& flat, double scale) {
  const int n = fusion_check(table, flat, "fusion_unpack");
  hcb::launch_fusion_unpack(reinterpret_cast<const hcb::FusionEntry*>(table.data_ptr<int64_t>()), n,
                            flat.data_ptr<float>(), fusion_max_chunks(table, flat), (float)scale, cur_stream());
}

int64_t fusion_chunk() { return hcb::fusion_chunk_elems(); }

// ---------------------------------------------------------------- space-to-depth stem
void stem_s2d(const Tensor& x, const Tensor& out, int64_t pad) {
  check_cuda(x, "x");
  check_cuda(out, "out");
  if (x.scalar_type() == at::kFloat) {  // fp32 image -> the folded tensor's three bf16 planes [3][N][Hs][Ws][16]
    const int64_t ops = check_planes(out, "out");
    TORCH_CHECK(x.dim() == 4 && out.dim() == 5 && x.is_contiguous() && out.select(0, 0).is_contiguous() &&
                    x.size(3) >= 4 && x.size(3) % 4 == 0 && out.size(4) == 16 && out.size(1) == x.size(0),
                "hcb.stem_s2d: fp32 x [N][H][W][>=4, multiple of 4] -> planes [3][N][Hs][Ws][16]");
    const int64_t H = x.size(1), W = x.size(2), Hs = out.size(2), Ws = out.size(3);
    TORCH_CHECK(2 * Hs - 1 - pad < H + 8 && 2 * Ws - 1 - pad < W + 8 && x.numel() < (1ll << 31),
                "hcb.stem_s2d: folded extent");
    hcb::launch_stem_s2d_f32(x.data_ptr<float>(), (int)x.size(0), (int)H, (int)W, (int)x.size(3),
                             reinterpret_cast<uint16_t*>(out.data_ptr()), ops, (int)Hs, (int)Ws, (int)pad,
                             cur_stream());
    return;
  }
  TORCH_CHECK(x.dim() == 4 && out.dim() == 4 && x.scalar_type() == kAct && out.scalar_type() == kAct,
              "hcb.stem_s2d: 16-bit NHWC tensors");
  TORCH_CHECK(x.is_contiguous() && out.is_contiguous() && x.size(3) >= 4 && x.size(3) % 4 == 0 && out.size(3) == 16 &&
                  out.size(0) == x.size(0),
              "hcb.stem_s2d: x [N][H][W][>=4, multiple of 4] -> out [N][Hs][Ws][16]");
  const int64_t H = x.size(1), W = x.size(2), Hs = out.size(1), Ws = out.size(2);
  TORCH_CHECK(2 * Hs - 1 - pad < H + 8 && 2 * Ws - 1 - pad < W + 8 && x.numel() < (1ll << 31),
              "hcb.stem_s2d: folded extent");
  hcb::launch_stem_s2d(reinterpret_cast<const uint16_t*>(x.data_ptr()), (int)x.size(0), (int)H, (int)W,
                       (int)x.size(3), reinterpret_cast<uint16_t*>(out.data_ptr()), (int)Hs, (int)Ws, (int)pad,
                       cur_stream());
}

void stem_wfold(const Tensor& w, const Tensor& wp) {
  check_f32(w, "w");
  check_cuda(wp, "wp");
  TORCH_CHECK(w.dim() == 4 && w.size(1) == 7 && w.size(2) == 7 && w.size(3) >= 3 && w.is_contiguous(),
              "hcb.stem_wfold: w [cout][7][7][>=3] fp32");
  // wp: the bf16 pack [cout][256], or (fp32 path) its hi / mid / lo planes [3][cout][256]
  const bool p3 = wp.dim() == 3 && wp.size(0) == 3 && wp.scalar_type() == at::kBFloat16;
  TORCH_CHECK((p3 || wp.scalar_type() == kAct) && wp.is_contiguous() && wp.numel() == (p3 ? 3 : 1) * w.size(0) * 256,
              "hcb.stem_wfold: wp bf16 [cout][256] or planes [3][cout][256]");
  hcb::launch_stem_wfold(w.data_ptr<float>(), (int)w.size(0), (int)w.size(3),
                         reinterpret_cast<uint16_t*>(wp.data_ptr()), cur_stream(), p3);
}

void stem_wgrad_unfold(const Tensor& dwp, const Tensor& dw) {
  check_f32(dwp, "dwp");
  check_f32(dw, "dw");
  TORCH_CHECK(dw.dim() == 4 && dw.size(1) == 7 && dw.size(2) == 7 && dw.size(3) >= 3 && dw.is_contiguous() &&
                  dwp.is_contiguous() && dwp.numel() == dw.size(0) * 256,
              "hcb.stem_wgrad_unfold: dwp [cout][256] -> dw [cout][7][7][>=3]");
  hcb::launch_stem_wgrad_unfold(dwp.data_ptr<float>(), (int)dw.size(0), (int)dw.size(3), dw.data_ptr<float>(),
                                cur_stream());
}

// ---- fp32 path on bf16 planes (conv_p3.hip)

// geom as conv_igemm; x: planes of the input, w: hi pack, w_lo: [2][n] mid / lo packs; y fp32
// (y_planes, the inference epilogue's plane output: y / yres are plane 0 of the output / residual
// planes, validated as 16-bit tensors with geom's out_f32 = 0)
hcb::ConvParams p3_params(const Tensor& x, const Tensor& w, const Tensor& w_lo, const Tensor& y,
                          const c10::optional<Tensor>& yres, const c10::optional<Tensor>& bias,
                          const c10::optional<Tensor>& stats, at::IntArrayRef g, int64_t cfg,
                          const c10::optional<Tensor>& stats_shift, bool y_planes = false) {
  const int64_t xps = check_planes(x, "x");
  TORCH_CHECK(hcb::p3_cfg_valid((int)cfg), "hcb.conv_p3: cfg 0..36, or a 3x3 patch cfg (64..)");
  // conv_params validates geometry and byte ranges on plane 0 (a bf16 tensor of this build's type)
  hcb::ConvParams p = conv_params(x.select(0, 0), w, y, yres, bias, g);
  const int bm = hcb::p3_tile_m((int)cfg), bn = hcb::p3_tile_n((int)cfg);
  TORCH_CHECK(y_planes ? !p.out_f32 : p.out_f32 && y.scalar_type() == at::kFloat,
              "hcb.conv_p3: fp32 output (geom out_f32 = 0 with a plane output)");
  check_range(x, 2 * xps * 2 + (int64_t)p.x_bytes, "x planes");
  TORCH_CHECK(2 * xps * 2 < (1ll << 32), "hcb.conv_p3: plane stride exceeds the 32-bit offset range");
  p.x_plane = (uint32_t)(xps * 2);
  TORCH_CHECK(w_lo.dim() == 2 && w_lo.size(0) == 2 && w_lo.stride(1) == 1 && w_lo.scalar_type() == w.scalar_type() &&
                  w_lo.size(1) >= (int64_t)p.Nout * p.Kpad,
              "hcb.conv_p3: w_lo must be [2][>= Nout*Kpad] of the pack's type");
  const Tensor m = w_lo.select(0, 0), l = w_lo.select(0, 1);
  check_align16(m.data_ptr(), "w_lo[0]");
  check_align16(l.data_ptr(), "w_lo[1]");
  p.w_lo = m.data_ptr();
  p.w_lo2 = l.data_ptr();
  attach_stats(p, stats, bm, "conv_p3");
  TORCH_CHECK(!stats_shift.has_value() || p.stats != nullptr, "hcb.conv_p3: stats_shift without stats");
  p.stats_shift = opt_f32(stats_shift, p.Nout, "stats_shift");
  attach_splitk(p, bm, bn, "conv_p3");
  return p;
}

void conv_p3(const Tensor& x, const Tensor& w, const Tensor& w_lo, const Tensor& y, const c10::optional<Tensor>& yres,
             const c10::optional<Tensor>& bias, const c10::optional<Tensor>& stats, at::IntArrayRef g, int64_t cfg,
             const c10::optional<Tensor>& stats_shift) {
  hcb::ConvParams p = p3_params(x, w, w_lo, y, yres, bias, stats, g, cfg, stats_shift);
  hcb::launch_conv_p3(p, (int)cfg, cur_stream());
}

// fp32 data gradient with the fused BN-backward epilogue (see conv_igemm_bnb): z fp32, yact the
// activation's planes (mode 1), output g fp32
void conv_p3_bnb(const Tensor& x, const Tensor& w, const Tensor& w_lo, const Tensor& y,
                 const c10::optional<Tensor>& yres, at::IntArrayRef g, int64_t cfg, const Tensor& z,
                 const c10::optional<Tensor>& yact, int64_t ld, const Tensor& mean, const Tensor& invstd,
                 const Tensor& gamma, const Tensor& beta, const Tensor& acc, int64_t R, int64_t mode) {
  hcb::ConvParams p = p3_params(x, w, w_lo, y, yres, c10::nullopt, c10::nullopt, g, cfg, c10::nullopt);
  set_bnb(p, z, yact, ld, mean, invstd, gamma, beta, acc, R, mode, true);
  hcb::launch_conv_p3(p, (int)cfg, cur_stream());
}

// fp32 forward conv + inference BN (+ residual, ReLU) in the plane GEMM's epilogue (see
// conv_igemm_inf): y fp32 (geom out_f32 = 1), or bf16 planes [3, ...] (out_f32 = 0) written with the
// output's plane stride; res in y's format. cfg 0..17: the per-tile kernels.
void conv_p3_inf(const Tensor& x, const Tensor& w, const Tensor& w_lo, const Tensor& y,
                 const c10::optional<Tensor>& res, at::IntArrayRef g, int64_t cfg, const Tensor& gamma,
                 const Tensor& beta, const Tensor& mean, const Tensor& var, double eps) {
  TORCH_CHECK(hcb::p3_cfg_has_inf((int)cfg), "hcb.conv_p3_inf: cfg 0..17 (a persistent cfg runs its per-tile twin)");
  const hcb::ConvParams q = decode_geom(kConvGeom, g, "conv_p3_inf");
  const bool yp3 = y.scalar_type() == at::kBFloat16;
  TORCH_CHECK(yp3 == (q.out_f32 == 0), "hcb.conv_p3_inf: geom out_f32 = 0 exactly for a plane output");
  hcb::ConvParams p;
  if (yp3) {
    const int64_t yps = check_planes(y, "y");
    c10::optional<Tensor> r0;
    int64_t rps = 0;
    if (q.beta) {
      TORCH_CHECK(res.has_value(), "hcb.conv_p3_inf: beta needs res");
      rps = check_planes(*res, "res");
      r0 = res->select(0, 0);
    }
    p = p3_params(x, w, w_lo, y.select(0, 0), r0, c10::nullopt, c10::nullopt, g, cfg, c10::nullopt, true);
    // conv_params checked plane 0's rows against the storage; the other two planes lie 2 * stride on
    const int64_t span = out_span_bytes(p.M, p.ldy, p.Nout, 2);
    check_range(y, 2 * yps * 2 + span, "y planes");
    TORCH_CHECK(yps >= span / 2, "hcb.conv_p3_inf: y planes overlap");
    if (p.beta) check_range(*res, 2 * rps * 2 + span, "res planes");
    p.y_p3 = 1;
    p.y_plane = yps;
    p.yres_plane = rps;
  } else {
    TORCH_CHECK(!q.beta || (res.has_value() && res->scalar_type() == at::kFloat), "hcb.conv_p3_inf: fp32 res");
    p = p3_params(x, w, w_lo, y, res, c10::nullopt, c10::nullopt, g, cfg, c10::nullopt);
  }
  set_inf(p, y, gamma, beta, mean, var, eps);
  hcb::launch_conv_p3(p, (int)cfg, cur_stream());
}

// geom as conv_wgrad; dy / x planes
void conv_wgrad_p3(const Tensor& dy, const Tensor& x, const Tensor& dw, at::IntArrayRef g, int64_t cfg,
                   int64_t splits) {
  const int64_t dps = check_planes(dy, "dy"), xps = check_planes(x, "x");
  TORCH_CHECK(cfg >= 0 && cfg < hcb::N_WP3_CFG, "hcb.conv_wgrad_p3: cfg 0..18");
  hcb::WgradParams p;
  const int eff_splits = wgrad_params(p, dy, x, dw, g, splits, "conv_wgrad_p3");
  TORCH_CHECK(2 * xps * 2 < (1ll << 32) && 2 * dps * 2 < (1ll << 32), "hcb.conv_wgrad_p3: plane stride range");
  check_range(x, 2 * xps * 2 + (int64_t)p.x_bytes, "x planes");
  check_range(dy, 2 * dps * 2 + (int64_t)p.dy_bytes, "dy planes");
  TORCH_CHECK(!hcb::wp3_cfg_persistent((int)cfg) || (int64_t)p.Nout * p.K * 4 < (1ll << 31),
              "hcb.conv_wgrad_p3: the persistent configs address dW through a 32-bit buffer offset");
  p.dy_plane = (uint32_t)(dps * 2);
  p.x_plane = (uint32_t)(xps * 2);
  hcb::launch_wgrad_p3(p, (int)cfg, eff_splits, cur_stream());
}

// fp32 x [rows][ldx] (first C channels) -> planes out [3][rows][ldo]
void split_planes(const Tensor& x, int64_t ldx, int64_t rows, int64_t C, const Tensor& out, int64_t ldo) {
  check_f32(x, "x");
  const int64_t ps = check_planes(out, "out");
  TORCH_CHECK(C % 8 == 0 && ldx % 8 == 0 && ldo % 8 == 0 && ldx >= C && ldo >= C, "hcb.split_planes: C / ld % 8");
  check_align16(x.data_ptr(), "x");
  check_range(x, ((rows - 1) * ldx + C) * 4, "x");
  check_range(out, (2 * ps + (rows - 1) * ldo + C) * 2, "out");
  TORCH_CHECK(ps >= (rows - 1) * ldo + C, "hcb.split_planes: planes overlap");
  hcb::launch_split_planes(x.data_ptr<float>(), (int)ldx, rows, (int)C, (uint16_t*)out.data_ptr(), (int)ldo, ps,
                           cur_stream());
}

void merge_planes(const Tensor& in, int64_t ldi, int64_t rows, int64_t C, const Tensor& y, int64_t ldy) {
  const int64_t ps = check_planes(in, "in");
  check_f32(y, "y");
  TORCH_CHECK(C % 8 == 0 && ldi % 8 == 0 && ldy % 8 == 0, "hcb.merge_planes: C / ld % 8");
  check_align16(y.data_ptr(), "y");
  check_range(in, (2 * ps + (rows - 1) * ldi + C) * 2, "in");
  check_range(y, ((rows - 1) * ldy + C) * 4, "y");
  hcb::launch_merge_planes((const uint16_t*)in.data_ptr(), (int)ldi, ps, rows, (int)C, y.data_ptr<float>(), (int)ldy,
                           cur_stream());
}

void gap_fwd_p3(const Tensor& x, const Tensor& y, int64_t N, int64_t HW, int64_t C) {
  const int64_t xps = check_planes(x, "x"), yps = check_planes(y, "y");
  TORCH_CHECK(C % 8 == 0, "hcb.gap_fwd_p3: C % 8");
  check_range(x, (2 * xps + N * HW * C) * 2, "x");
  check_range(y, (2 * yps + N * C) * 2, "y");
  hcb::launch_gap_fwd_p3((const uint16_t*)x.data_ptr(), xps, (uint16_t*)y.data_ptr(), yps, (int)N, (int)HW, (int)C,
                         cur_stream());
}

void set_deterministic(bool on) { hcb::set_deterministic(on); }

}  // namespace


HCB_TORCH_LIBRARY(hcb, m) {
  m.def("conv_igemm(Tensor x, Tensor w, Tensor(a!) y, Tensor? yres, Tensor? bias, Tensor(b!)? stats, int[] geom, int cfg, Tensor? stats_shift=None) -> ()");
  m.def("conv_igemm_bnb(Tensor x, Tensor w, Tensor(a!) y, Tensor? yres, int[] geom, int cfg, Tensor z, Tensor? yact, int ld, Tensor mean, Tensor invstd, Tensor gamma, Tensor beta, Tensor(b!) acc, int R, int mode) -> ()");
  m.def("conv_igemm_inf(Tensor x, Tensor w, Tensor(a!) y, Tensor? res, int[] geom, int cfg, Tensor gamma, Tensor beta, Tensor mean, Tensor var, float eps) -> ()");
  m.def("gemm_cfg_table(str family) -> int[]", gemm_cfg_table);
  m.def("p3_patch_fit(int cfg, int H, int W, bool bnb) -> int[]", p3_patch_fit);
  m.def("conv_geom_fields(str kind) -> str[]", conv_geom_fields);
  m.def("set_splitk_workspace(Tensor ws, Tensor cnt) -> ()");
  m.def("conv_wgrad(Tensor dy, Tensor x, Tensor(a!) dw, int[] geom, int cfg, int splits) -> ()");
  m.def("bn_apply(Tensor x, int ldx, Tensor(a!) y, int ldy, Tensor? res, int ldr, int M, int C, Tensor mean, Tensor invstd, Tensor gamma, Tensor beta, int relu, float? act_max=None) -> ()");
  m.def("pool_fwd(Tensor x, Tensor(a!) y, Tensor(b!)? idx, int[] geom) -> ()");
  m.def("pool_bwd(Tensor dy, Tensor x, Tensor y, Tensor? idx, Tensor(a!) dx, int[] geom, bool accumulate) -> ()");
  m.def("pool_fwd_p3(Tensor x, Tensor(a!) y, Tensor(b!)? idx, int[] geom) -> ()");
  m.def("gap_fwd(Tensor x, Tensor(a!) y, int N, int HW, int C) -> ()");
  m.def("gap_bwd(Tensor dy, Tensor(a!) dx, int N, int HW, int C) -> ()");
  m.def("softmax_xent(Tensor logits, int ld, Tensor labels, int ncls, Tensor(a!) row_loss, Tensor(b!) dlogits, int lddl, float scale, Tensor? scale_dev=None, Tensor(c!)? dl32=None, float label_smoothing=0.0) -> ()");
  m.def("eval_metrics(Tensor logits, int ld, Tensor labels, int ncls, Tensor(a!) counters) -> ()");
  m.def("nonfinite(Tensor g, Tensor(a!) flag) -> ()");
  m.def("loss_total(Tensor row_loss, int B, Tensor? l2, float half_wd, Tensor(a!) loss) -> ()");
  m.def("loss_scale_update(Tensor(a!) hyper, float world, bool dynamic) -> ()");
  m.def("colsum(Tensor g, int ld, int M, int N, Tensor(a!) out) -> ()");
  m.def("zero_bufs(Tensor(a!)[] ts) -> ()");
  m.def("sgd_momentum(Tensor(a!) w, Tensor(b!) mom, Tensor g, int n_decay, Tensor hyper, Tensor(c!)? l2, bool nesterov) -> ()");
  m.def("rmsprop(Tensor(a!) w, Tensor(b!) mom, Tensor(c!) ms, Tensor g, int n_decay, Tensor hyper, Tensor ohyper, Tensor(d!)? l2) -> ()");
  m.def("adam(Tensor(a!) w, Tensor(b!) m, Tensor(c!) v, Tensor g, int n_decay, Tensor hyper, Tensor ohyper, Tensor state, Tensor(d!)? l2) -> ()");
  m.def("adam_advance(Tensor(a!) state, Tensor ohyper, Tensor hyper) -> ()");
  m.def("weight_pack(Tensor master, Tensor(a!) pack, Tensor table, int max_work, int lo=0) -> ()");
  m.def("add_bf16(Tensor a, Tensor b, Tensor(a!) y) -> ()");
  m.def("relu_bwd(Tensor dy, Tensor y, Tensor(a!) dz) -> ()");
  m.def("bn_apply_acc(Tensor x, int ldx, Tensor(a!) y, int ldy, Tensor? res, int ldr, int M, int C, Tensor acc, int R, float eps, float momentum, Tensor gamma, Tensor beta, int relu, Tensor(b!) saved_mean, Tensor(c!) saved_invstd, Tensor(d!)? running_mean, Tensor(e!)? running_var, Tensor? shift=None, Tensor? res_acc=None, Tensor? res_gamma=None, Tensor? res_beta=None, Tensor(g!)? res_saved_mean=None, Tensor(h!)? res_saved_invstd=None, Tensor(i!)? res_running_mean=None, Tensor(j!)? res_running_var=None, Tensor? res_shift=None, float? act_max=None) -> ()");
  m.def("bn_bwd_reduce_acc(Tensor dy, int lddy, Tensor? y, int ldyv, Tensor x, int ldx, int M, int C, Tensor mean, Tensor invstd, Tensor gamma, Tensor beta, int relu, Tensor(a!) acc, int R, Tensor(b!)? gout, int ldg, Tensor? pool_amax=None, int[]? pool_geom=None) -> ()");
  m.def("bn_bwd_apply_acc(Tensor dy, int lddy, Tensor? y, int ldyv, Tensor x, int ldx, Tensor(a!) dx, int lddx, int M, int C, Tensor mean, Tensor invstd, Tensor gamma, Tensor beta, Tensor acc, int R, Tensor(b!) dgamma, Tensor(c!) dbeta, int relu, Tensor(d!)? shift_out=None, Tensor? pool_amax=None, int[]? pool_geom=None, Tensor? add=None, int ldadd=0) -> ()");
  m.def("bn_stats_acc(Tensor x, int ldx, int M, int C, Tensor(a!) acc, int R, Tensor? shift=None) -> ()");
  m.def("dwconv_fwd(Tensor x, Tensor w, Tensor(a!) z, int[] geom, Tensor(b!)? stats=None, int stats_R=0, Tensor? stats_shift=None) -> ()");
  m.def("dwconv_dgrad(Tensor dz, Tensor w, Tensor(a!) dx, int[] geom, bool accumulate) -> ()");
  m.def("dwconv_wgrad(Tensor dz, Tensor x, Tensor(a!) ws, Tensor(b!) dw, int[] geom) -> ()");
  m.def("dwconv_wgrad_blocks(int[] geom) -> int", dwconv_wgrad_blocks);
  m.def("preprocess_images(Tensor src, Tensor desc, Tensor desc_host, Tensor(a!) out, float[] scale, float[] bias) -> ()");
  m.def("preprocess_distort(Tensor src, Tensor desc, Tensor desc_host, Tensor params, Tensor params_host, "
        "Tensor(a!) out, Tensor(b!) work, float[] scale, float[] bias) -> ()");
  m.def("cifar_batch(Tensor data, Tensor labels_all, Tensor desc, Tensor desc_host, Tensor(a!) out, Tensor(b!) labels_out) -> ()");
  m.def("jpeg_idct(Tensor coef, Tensor segs, Tensor segs_host, Tensor(a!) planes) -> ()");
  m.def("jpeg_crop_rgb(Tensor planes, Tensor imgs, Tensor imgs_host, Tensor desc, Tensor desc_host, Tensor(a!) stage) -> ()");
  m.def("shortcut_pad_fwd(Tensor x, Tensor(a!) y, int s) -> ()");
  m.def("shortcut_pad_bwd(Tensor g, Tensor(a!) dx, int s) -> ()");
  m.def("lrn_fwd(Tensor x, Tensor(a!) y, int r, float bias, float alpha, float beta) -> ()");
  m.def("lrn_bwd(Tensor dy, Tensor x, Tensor(a!) dx, int r, float bias, float alpha, float beta) -> ()");
  m.def("bn_relu_maxpool_acc(Tensor z, Tensor(a!) y, Tensor(b!) amax, int[] geom, Tensor acc, int R, float eps, "
        "float momentum, Tensor gamma, Tensor beta, Tensor(c!) saved_mean, Tensor(d!) saved_invstd, "
        "Tensor(e!) run_mean, Tensor(f!) run_var, Tensor? shift=None) -> ()");
  m.def("dropout_fwd(Tensor x, Tensor(a!) y, Tensor(b!) mask, float keep, int seed, Tensor step) -> ()");
  m.def("dropout_bwd(Tensor dy, Tensor mask, Tensor(a!) dx, float keep) -> ()");
  m.def("synth_images(Tensor(a!) out, int C, int Cpad, float mean, float std, int seed) -> ()");
  m.def("synth_labels(Tensor(a!) out, int ncls, int seed) -> ()");
  m.def("bucket_pack(Tensor src, Tensor(a!) dst, float scale) -> ()");
  m.def("bucket_unpack(Tensor src, Tensor(a!) dst, float scale) -> ()");
  m.def("fusion_pack(Tensor table, Tensor(a!) flat, float scale) -> ()");
  m.def("fusion_unpack(Tensor table, Tensor flat, float scale) -> ()");
  m.def("fusion_chunk() -> int", fusion_chunk);
  m.def("stem_s2d(Tensor x, Tensor(a!) out, int pad) -> ()");
  m.def("set_deterministic(bool on) -> ()", set_deterministic);
  m.def("stem_wfold(Tensor w, Tensor(a!) wp) -> ()");
  m.def("stem_wgrad_unfold(Tensor dwp, Tensor(a!) dw) -> ()");
  m.def("conv_p3(Tensor x, Tensor w, Tensor w_lo, Tensor(a!) y, Tensor? yres, Tensor? bias, Tensor(b!)? stats, int[] geom, int cfg, Tensor? stats_shift=None) -> ()");
  m.def("conv_wgrad_p3(Tensor dy, Tensor x, Tensor(a!) dw, int[] geom, int cfg, int splits) -> ()");
  m.def("conv_p3_bnb(Tensor x, Tensor w, Tensor w_lo, Tensor(a!) y, Tensor? yres, int[] geom, int cfg, Tensor z, Tensor? yact, int ld, Tensor mean, Tensor invstd, Tensor gamma, Tensor beta, Tensor(b!) acc, int R, int mode) -> ()");
  m.def("conv_p3_inf(Tensor x, Tensor w, Tensor w_lo, Tensor(a!) y, Tensor? res, int[] geom, int cfg, Tensor gamma, Tensor beta, Tensor mean, Tensor var, float eps) -> ()");
  m.def("split_planes(Tensor x, int ldx, int rows, int C, Tensor(a!) out, int ldo) -> ()");
  m.def("merge_planes(Tensor x, int ldi, int rows, int C, Tensor(a!) y, int ldy) -> ()");
  m.def("gap_fwd_p3(Tensor x, Tensor(a!) y, int N, int HW, int C) -> ()");
}

HCB_TORCH_LIBRARY_IMPL(hcb, CUDA, m) {
  m.impl("conv_igemm", conv_igemm);
  m.impl("conv_igemm_bnb", conv_igemm_bnb);
  m.impl("conv_igemm_inf", conv_igemm_inf);
  m.impl("eval_metrics", eval_metrics);
  m.impl("nonfinite", nonfinite);
  m.impl("loss_total", loss_total);
  m.impl("loss_scale_update", loss_scale_update);
  m.impl("set_splitk_workspace", set_splitk_workspace);
  m.impl("conv_wgrad", conv_wgrad);
  m.impl("bn_apply", bn_apply);
  m.impl("pool_fwd", pool_fwd);
  m.impl("pool_bwd", pool_bwd);
  m.impl("pool_fwd_p3", pool_fwd_p3);
  m.impl("gap_fwd", gap_fwd);
  m.impl("gap_bwd", gap_bwd);
  m.impl("softmax_xent", softmax_xent);
  m.impl("colsum", colsum);
  m.impl("zero_bufs", zero_bufs);
  m.impl("sgd_momentum", sgd_momentum);
  m.impl("rmsprop", rmsprop);
  m.impl("adam", adam);
  m.impl("adam_advance", adam_advance);
  m.impl("weight_pack", weight_pack);
  m.impl("add_bf16", add_bf16);
  m.impl("relu_bwd", relu_bwd);
  m.impl("bn_apply_acc", bn_apply_acc);
  m.impl("bn_bwd_reduce_acc", bn_bwd_reduce_acc);
  m.impl("bn_bwd_apply_acc", bn_bwd_apply_acc);
  m.impl("bn_stats_acc", bn_stats_acc);
  m.impl("dwconv_fwd", dwconv_fwd);
  m.impl("dwconv_dgrad", dwconv_dgrad);
  m.impl("dwconv_wgrad", dwconv_wgrad);
  m.impl("synth_images", synth_images);
  m.impl("dropout_fwd", dropout_fwd);
  m.impl("bn_relu_maxpool_acc", bn_relu_maxpool_acc);
  m.impl("dropout_bwd", dropout_bwd);
  m.impl("preprocess_images", preprocess_images);
  m.impl("preprocess_distort", preprocess_distort);
  m.impl("cifar_batch", cifar_batch);
  m.impl("jpeg_idct", jpeg_idct);
  m.impl("jpeg_crop_rgb", jpeg_crop_rgb);
  m.impl("shortcut_pad_fwd", shortcut_pad_fwd);
  m.impl("shortcut_pad_bwd", shortcut_pad_bwd);
  m.impl("lrn_fwd", lrn_fwd);
  m.impl("lrn_bwd", lrn_bwd);
  m.impl("synth_labels", synth_labels);
  m.impl("bucket_pack", bucket_pack);
  m.impl("bucket_unpack", bucket_unpack);
  m.impl("fusion_pack", fusion_pack);
  m.impl("fusion_unpack", fusion_unpack);
  m.impl("stem_s2d", stem_s2d);
  m.impl("stem_wfold", stem_wfold);
  m.impl("stem_wgrad_unfold", stem_wgrad_unfold);
  m.impl("conv_p3", conv_p3);
  m.impl("conv_wgrad_p3", conv_wgrad_p3);
  m.impl("conv_p3_bnb", conv_p3_bnb);
  m.impl("conv_p3_inf", conv_p3_inf);
  m.impl("split_planes", split_planes);
  m.impl("merge_planes", merge_planes);
  m.impl("gap_fwd_p3", gap_fwd_p3);
}
