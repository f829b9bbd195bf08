// Coupled PDE systems with nonlinear functions of the unknowns as factors (include/pinn_jet.h, "term residuals of coupled systems
// with nonlinear functions of the unknowns"): level NL of term_system_kernel.h, w_k = g_k(shift + scale * s_k) as value rows
// and cotangent targets of their own.
#include "term_system_host.h"

extern "C" int pinn_term_residual_system_nl(const PinnTermPdeSystemNl* pde, const float* coef_values, const float* const* jets,
                                            const float* x, const float* t, const float* fn_values, const float* nl_params, int64_t N,
                                            float grad_scale, const float* residual_cotangent, float* residual_out, float* loss_sum_out,
                                            float* eq_loss_sums, float* const* jet_cotangents, float* coef_grads, double* scratch,
                                            void* stream) {
  const SysCall a = {coef_values, jets, x, t, fn_values, nl_params, nullptr, (long long)N, grad_scale, residual_cotangent, residual_out,
                     loss_sum_out, eq_loss_sums, jet_cotangents, coef_grads, nullptr, scratch, static_cast<hipStream_t>(stream)};
  return sys_residual<NL>("pinn_term_residual_system_nl", pde, a);
}
