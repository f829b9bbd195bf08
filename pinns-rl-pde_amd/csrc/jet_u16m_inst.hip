// Instantiations of the 16-point fused kernel on the merged stream set (jet_kernel_u16.h, MRG = true: Burgers on the
// streams u, u_t - nu u_xx, u_x), one translation unit per activation family (-DPINN_WIDE_ACT=<0..4>), same flags and
// fallback rules as the jet_u16_* units.  A family is routed to only if this unit and its jet_u16mc_* unit both are.
#include "jet_kernel_u16.h"

#if !defined(PINN_WIDE_ACT)
#error "compile with -DPINN_WIDE_ACT=<0..4>"
#endif

#define PINN_CAT2(a, b) a##b
#define PINN_CATM(a, b) PINN_CAT2(a, b)

namespace pinn {
hipError_t PINN_CATM(launch_jetum_a, PINN_WIDE_ACT)(const KernelArgs& a, bool bwd, int grid, hipStream_t stream) {
  return launch_jet_u16m_act<PINN_WIDE_ACT>(a, bwd, grid, stream);
}
}  // namespace pinn
