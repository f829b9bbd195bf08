// Coupled PDE systems with mixed derivatives (include/pinn_jet.h, "term residuals of coupled systems with mixed
// derivatives"): level MIXED of term_system_kernel.h, u_xy, u_xz, u_yz of every field by the polarisation formula of
// term_mixed_kernels.hip.  The pure factors round exactly as at level PLAIN.
#include "term_system_host.h"

extern "C" int pinn_term_residual_system_mixed(const PinnTermPdeSystemMixed* pde, const float* coef_values, const float* const* jets,
                                               const float* x, const float* t, int64_t N, float grad_scale,
                                               const float* residual_cotangent, float* residual_out, float* loss_sum_out,
                                               float* eq_loss_sums, float* const* jet_cotangents, float* coef_grads, double* scratch,
                                               void* stream) {
  const SysCall a = {coef_values, jets, x, t, nullptr, nullptr, nullptr, (long long)N, grad_scale, residual_cotangent, residual_out,
                     loss_sum_out, eq_loss_sums, jet_cotangents, coef_grads, nullptr, scratch, static_cast<hipStream_t>(stream)};
  return sys_residual<MIXED>("pinn_term_residual_system_mixed", pde, a);
}
