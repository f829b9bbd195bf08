// Coupled PDE systems given as data (include/pinn_jet.h, "term residuals of coupled systems"): level PLAIN of
// term_system_kernel.h, up to 4 x 13 values and 4 x 11 derivative accumulators per point.
#include "term_system_host.h"

extern "C" int pinn_term_residual_system(const PinnTermPdeSystem* pde, const float* coef_values, const float* const* jets,
                                         const float* x, const float* t, int64_t N, float grad_scale,
                                         const float* residual_cotangent, float* residual_out, float* loss_sum_out,
                                         float* eq_loss_sums, float* const* jet_cotangents, float* coef_grads, double* scratch,
                                         void* stream) {
  const SysCall a = {coef_values, jets, x, t, nullptr, nullptr, nullptr, (long long)N, grad_scale, residual_cotangent, residual_out,
                     loss_sum_out, eq_loss_sums, jet_cotangents, coef_grads, nullptr, scratch, static_cast<hipStream_t>(stream)};
  return sys_residual<PLAIN>("pinn_term_residual_system", pde, a);
}
