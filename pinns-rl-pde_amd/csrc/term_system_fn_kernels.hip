// Coupled PDE systems with known functions of (x, t) as factors (include/pinn_jet.h, "term residuals of coupled systems with
// known functions"): level FN of term_system_kernel.h.  A known function g_k is one more value row, four rows are 4 KB of LDS;
// held in registers behind a wave-uniform switch instead, the function values pushed the forms with coefficient sums, whose
// term loop is unrolled over 32 terms of scalar operands, from scalar spills into scratch memory.
#include "term_system_host.h"

extern "C" int pinn_term_residual_system_fn(const PinnTermPdeSystemFn* pde, const float* coef_values, const float* const* jets,
                                            const float* x, const float* t, const float* fn_values, int64_t N, float grad_scale,
                                            const float* residual_cotangent, float* residual_out, float* loss_sum_out,
                                            float* eq_loss_sums, float* const* jet_cotangents, float* coef_grads, double* scratch,
                                            void* stream) {
  const SysCall a = {coef_values, jets, x, t, fn_values, nullptr, nullptr, (long long)N, grad_scale, residual_cotangent, residual_out,
                     loss_sum_out, eq_loss_sums, jet_cotangents, coef_grads, nullptr, scratch, static_cast<hipStream_t>(stream)};
  return sys_residual<FN>("pinn_term_residual_system_fn", pde, a);
}
