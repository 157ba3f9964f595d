// Launch of one implicit-GEMM main loop (conv_igemm.hip, conv_p3_fwd.h): the (CBIG, LHSDIL)
// instantiation that fits the problem's im2col path.
#pragma once
#include <type_traits>

#include "kernels.h"

namespace hcb {

// a kernel may ask for all of the CU's LDS as dynamic shared memory
template <typename K>
static hipError_t set_lds_max(K kern) {
  return hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}

// kern(std::bool_constant<CBIG>, std::bool_constant<LHSDIL>) names a kernel instantiation; its LDS
// limit is raised once, at its first launch (Kern is a lambda type of the calling launcher, so the
// flag is per instantiation)
template <bool CBIG, bool LHSDIL, typename Kern>
static void launch_igemm_variant(Kern kern, int grid, int block, size_t lds, hipStream_t st, const ConvParams& p) {
  void (*const k)(ConvParams) = kern(std::bool_constant<CBIG>{}, std::bool_constant<LHSDIL>{});
  static const hipError_t once = set_lds_max(k);
  (void)once;
  hipLaunchKernelGGL(k, dim3(grid), dim3(block), lds, st, p);
}

// CBIG: whole 64-channel k-steps lie in one filter tap; LHSDIL: lhs-dilated input (strided data
// gradients). The inference epilogue serves forward problems only: no LHSDIL instantiation of an
// INF kernel exists.
template <bool INF, typename Kern>
static void launch_igemm(Kern kern, int grid, int block, size_t lds, hipStream_t st, const ConvParams& p) {
  const bool cbig = (p.C % 64) == 0;
  if constexpr (!INF) {
    if (p.idil_h > 1 || p.idil_w > 1) {
      if (cbig)
        launch_igemm_variant<true, true>(kern, grid, block, lds, st, p);
      else
        launch_igemm_variant<false, true>(kern, grid, block, lds, st, p);
      return;
    }
  }
  if (cbig)
    launch_igemm_variant<true, false>(kern, grid, block, lds, st, p);
  else
    launch_igemm_variant<false, false>(kern, grid, block, lds, st, p);
}

}  // namespace hcb
