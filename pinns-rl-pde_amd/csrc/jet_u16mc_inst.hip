// Inverse-problem instantiations of the 16-point fused kernel on the merged stream set (jet_kernel_u16.h, MRG = true,
// COEF = true): the coefficient comes from a device array and its cotangent is the sum of the coefficient partials.
// One translation unit per activation family (-DPINN_WIDE_ACT=<0..4>), reverse launch only, same flags and fallback
// rules as the jet_u16c_* units.
#include "jet_kernel_u16.h"

#if !defined(PINN_WIDE_ACT)
#error "compile with -DPINN_WIDE_ACT=<0..4>"
#endif

#define PINN_CAT2(a, b) a##b
#define PINN_CATM(a, b) PINN_CAT2(a, b)

namespace pinn {
hipError_t PINN_CATM(launch_jetumc_a, PINN_WIDE_ACT)(const KernelArgs& a, int grid, hipStream_t stream) {
  return launch_jet_u16m_coef<PINN_WIDE_ACT>(a, grid, stream);
}
}  // namespace pinn
