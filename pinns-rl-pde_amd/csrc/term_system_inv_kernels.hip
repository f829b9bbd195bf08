// Coupled PDE systems with learnable parameters (include/pinn_jet.h, "term residuals of coupled systems with learnable
// parameters"): level INV of term_system_kernel.h.  The gradient of the parameters is a combination of sums over the points:
// the coefficient sums G_m, and, where a learnable nonlinear entry is evaluated, the twelve sums H_kj.  The finish launch adds
// the per-block partials in block order and combines them in double.
#include "term_system_host.h"

namespace {

constexpr int kSiRow = SysLevel<INV>::kRow;

// Thread k < 48: row k of the block partials summed in block order, in double, into LDS (rows the launch did not form count as
// 0: `with_g`, `with_h`).  Then thread k < 4: the loss sum of equation k, added to eq_loss_sums[k]; thread 0 also adds
// sum_e w_e S_e (ascending e, in double) to loss_sum_out.  4 <= k < 36: coefficient sum k - 4.  Thread 48 + q: parameter q,
//   param_grads[q] += sum_{m: coef_param[m] = q} coef_values[m] G_m + sum_{(k, j): nl_param[k][j] = q} nl_params[3 k + j] H_kj,
// the combination in double over m, then (k, j), ascending; one rounding at the add.  Every sum is taken once, by one thread:
// a parameter that many terms name costs no more than one row.
__global__ void term_system_inv_finish_kernel(const double* partial, int blocks, int n_eq, int n_terms, double w0, double w1, double w2,
                                              double w3, float* loss_sum_out, float* eq_loss_sums, float* coef_grads, SysParamMap map,
                                              int uses_nl, const float* coef_values, const float* nl_params, int with_g, int with_h,
                                              float* param_grads) {
  __shared__ double rowsum[kSiRow];
  const int k = threadIdx.x;
  if (k < kSiRow) {
    const bool formed = k < kSyG ? k < n_eq : (k < kSyH ? (with_g && k - kSyG < n_terms) : (with_h != 0));
    rowsum[k] = formed ? sys_row_sum(partial, blocks, kSiRow, k) : 0.0;
  }
  __syncthreads();
  if (k >= kSiRow) {
    const int q = k - kSiRow;
    if (!param_grads || q >= map.n_params) return;
    double acc = 0.0;
    for (int m = 0; m < n_terms; ++m)
      if (map.coef_param[m] == q) acc += (double)coef_values[m] * rowsum[kSyG + m];
    if (with_h) {
      for (int kj = 0; kj < kSyNlp; ++kj)
        if (map.nl_param[kj] == q && ((uses_nl >> (kj / 3)) & 1)) acc += (double)nl_params[kj] * rowsum[kSyH + kj];
    }
    param_grads[q] = (float)((double)param_grads[q] + acc);
    return;
  }
  if (k >= kSyH) return;
  if (k == 0 && loss_sum_out) {
    const double w[PINN_SYSTEM_MAX_EQUATIONS] = {w0, w1, w2, w3};
    double total = 0.0;
    for (int e = 0; e < n_eq; ++e) total += w[e] * rowsum[e];
    loss_sum_out[0] = (float)((double)loss_sum_out[0] + total);
  }
  float* out = nullptr;
  if (k < kSyG) {
    if (k < n_eq && eq_loss_sums) out = eq_loss_sums + k;
  } else if (k - kSyG < n_terms && coef_grads) {
    out = coef_grads + (k - kSyG);
  }
  if (!out) return;
  out[0] = (float)((double)out[0] + rowsum[k]);
}

}  // namespace

extern "C" int pinn_term_residual_system_inv(const PinnTermPdeSystemInv* pde, const float* coef_values, const float* const* jets,
                                             const float* x, const float* t, const float* fn_values, const float* nl_params,
                                             const float* param_values, int64_t N, float grad_scale, const float* residual_cotangent,
                                             float* residual_out, float* loss_sum_out, float* eq_loss_sums, float* const* jet_cotangents,
                                             float* coef_grads, float* param_grads, double* scratch, void* stream) {
  const SysCall a = {coef_values, jets, x, t, fn_values, nl_params, param_values, (long long)N, grad_scale, residual_cotangent, residual_out,
                     loss_sum_out, eq_loss_sums, jet_cotangents, coef_grads, param_grads, scratch, static_cast<hipStream_t>(stream)};
  SysProg<INV> p;
  int blocks;
  const char* who = "pinn_term_residual_system_inv";
  int rc = sys_parse<INV>(who, pde, a, p, &blocks);
  if (rc || !blocks) return rc;
  // the H sums only where a learnable nonlinear entry is inside the mask: every other launch keeps the registers of level NL
  bool hs = false;
  for (int kj = 0; kj < kSyNlp && param_grads; ++kj) hs = hs || (p.nl_param[kj] >= 0 && ((p.uses_nl >> (kj / 3)) & 1));
  rc = sys_launch<INV>(who, p, pde->n_fields, blocks, a, hs);
  if (rc || !a.reduce()) return rc;
  hipLaunchKernelGGL(term_system_inv_finish_kernel, dim3(1), dim3(64), 0, a.stream, scratch, blocks, p.n_eq, p.n_terms, p.w[0], p.w[1],
                     p.w[2], p.w[3], loss_sum_out, eq_loss_sums, coef_grads, static_cast<const SysParamMap&>(p), p.uses_nl, coef_values,
                     nl_params, a.coef_sums() ? 1 : 0, hs ? 1 : 0, param_grads);
  return sys_launched(who, "term_system_inv_finish_kernel");
}
