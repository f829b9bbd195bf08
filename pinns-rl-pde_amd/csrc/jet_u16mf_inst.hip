// Instantiations of the 16-point fused kernel on the merged stream set with the network's shape compiled in
// (jet_kernel_u16.h, MRG = true, FIXED = true), one translation unit per activation family (-DPINN_WIDE_ACT=<0..4>),
// same flags and fallback rules as the jet_u16m_* units.  A family is routed to only if this unit and its jet_u16mfc_*
// unit both are (pinn_abi.hip: use_fixed_shape).
#include "jet_kernel_u16.h"

#if !defined(PINN_WIDE_ACT)
#error "compile with -DPINN_WIDE_ACT=<0..4>"
#endif

#define PINN_CAT2(a, b) a##b
#define PINN_CATM(a, b) PINN_CAT2(a, b)

namespace pinn {
hipError_t PINN_CATM(launch_jetumf_a, PINN_WIDE_ACT)(const KernelArgs& a, bool bwd, int grid, hipStream_t stream) {
  return launch_jet_u16m_act<PINN_WIDE_ACT, true>(a, bwd, grid, stream);
}
}  // namespace pinn
