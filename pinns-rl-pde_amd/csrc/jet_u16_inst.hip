// Instantiations of the 16-point fused reverse kernel (jet_kernel_u16.h), one translation unit per stream set and
// activation family (-DPINN_NT=.. -DPINN_NX=.. -DPINN_WIDE_ACT=<0..4>), compiled with VGPR-form MFMAs like the
// jet_wide_* units.  A unit whose kernels use scratch is recorded in build/*.fallback (pinn_build_info()) and is not
// routed to: its calls keep the 32-point kernel.
#include "jet_kernel_u16.h"

#if !defined(PINN_NT) || !defined(PINN_WIDE_ACT)
#error "compile with -DPINN_NT=<0..2> -DPINN_NX=<0..4> -DPINN_WIDE_ACT=<0..4>"
#endif

#define PINN_CAT4(a, b, c, d) a##b##_##c##_a##d
#define PINN_CATA(a, b, c, d) PINN_CAT4(a, b, c, d)

namespace pinn {
hipError_t PINN_CATA(launch_jetu_, PINN_NT, PINN_NX, PINN_WIDE_ACT)(const KernelArgs& a, bool bwd, int grid, hipStream_t stream) {
  return launch_jet_u16_act<PINN_WIDE_ACT, PINN_NT, PINN_NX>(a, bwd, grid, stream);
}
}  // namespace pinn
