// Inverse-problem instantiations of the fused tile-major kernel (jet_kernel_wide.h, COEF = true): PDE coefficients read
// from a device array, coefficient cotangents flushed next to the loss sum.  One translation unit per stream set and
// activation family (-DPINN_NT=.. -DPINN_NX=.. -DPINN_WIDE_ACT=<0..4>), reverse launches only, built like the
// jet_wide_* units (VGPR-form MFMAs, default form where that fails: build/*.fallback, pinn_build_info()).
#include "jet_kernel_wide.h"

#if !defined(PINN_NT) || !defined(PINN_WIDE_ACT)
#error "compile with -DPINN_NT=<1..2> -DPINN_NX=<0..4> -DPINN_WIDE_ACT=<0..4>"
#endif

#define PINN_CAT4(a, b, c, d) a##b##_##c##_a##d
#define PINN_CATA(a, b, c, d) PINN_CAT4(a, b, c, d)

namespace pinn {
hipError_t PINN_CATA(launch_jetwc_, PINN_NT, PINN_NX, PINN_WIDE_ACT)(const KernelArgs& a, int grid, hipStream_t stream) {
  return launch_jet_wide_coef<PINN_WIDE_ACT, PINN_NT, PINN_NX>(a, grid, stream);
}
}  // namespace pinn
