// Inverse-problem instantiations of the fixed-shape merged units (jet_kernel_u16.h, MRG = true, COEF = true,
// FIXED = true).  One translation unit per activation family (-DPINN_WIDE_ACT=<0..4>), reverse launch only, same flags
// and fallback rules as the jet_u16mc_* units.
#include "jet_kernel_u16.h"

#if !defined(PINN_WIDE_ACT)
#error "compile with -DPINN_WIDE_ACT=<0..4>"
#endif

#define PINN_CAT2(a, b) a##b
#define PINN_CATM(a, b) PINN_CAT2(a, b)

namespace pinn {
hipError_t PINN_CATM(launch_jetumfc_a, PINN_WIDE_ACT)(const KernelArgs& a, int grid, hipStream_t stream) {
  return launch_jet_u16m_coef<PINN_WIDE_ACT, true>(a, grid, stream);
}
}  // namespace pinn
