// Inverse-problem instantiations of the 16-point fused reverse kernel (jet_kernel_u16.h, COEF = true): PDE coefficients
// read from a device array, coefficient cotangents reduced next to the loss sum.  One translation unit per stream set
// and activation family (-DPINN_NT=.. -DPINN_NX=.. -DPINN_WIDE_ACT=<0..4>), reverse launch only, same flags and
// fallback rules as the jet_u16_* units: a unit whose kernel uses scratch is recorded in build/*.fallback
// (pinn_build_info()) and is not routed to — its calls take the jet_widec_* unit.
#include "jet_kernel_u16.h"

#if !defined(PINN_NT) || !defined(PINN_WIDE_ACT)
#error "compile with -DPINN_NT=<1..2> -DPINN_NX=<0..2> -DPINN_WIDE_ACT=<0..4>"
#endif

#define PINN_CAT4(a, b, c, d) a##b##_##c##_a##d
#define PINN_CATA(a, b, c, d) PINN_CAT4(a, b, c, d)

namespace pinn {
hipError_t PINN_CATA(launch_jetuc_, PINN_NT, PINN_NX, PINN_WIDE_ACT)(const KernelArgs& a, int grid, hipStream_t stream) {
  return launch_jet_u16_coef<PINN_WIDE_ACT, PINN_NT, PINN_NX>(a, grid, stream);
}
}  // namespace pinn
