// Host side of the five coupled-system residual entry points: one descriptor parser, one launch dispatch and one finish launch
// behind pinn_term_residual_system, _mixed, _fn, _nl and _inv (term_system_kernel.h has the levels and the kernel).  Every
// message carries the entry point's name (`who`).
#pragma once
#include "term_system_kernel.h"

namespace {

// the arguments of an entry point; what a level does not have is null
struct SysCall {
  const float* coef_values;
  const float* const* jets;
  const float *x, *t, *fn_values, *nl_params, *param_values;
  long long N;
  float grad_scale;
  const float* residual_cotangent;
  float *residual_out, *loss_sum_out, *eq_loss_sums;
  float* const* jet_cotangents;
  float *coef_grads, *param_grads;
  double* scratch;
  hipStream_t stream;
  bool reduce() const { return loss_sum_out || eq_loss_sums || coef_grads || param_grads; }
  bool coef_sums() const { return coef_grads || param_grads; }  // the parameter gradients are built on the G sums
};

// the stream sets the library has axis-0 units for (csrc/Makefile: SETS)
bool sys_set_compiled(int nt, int nx) {
  static const int sets[][2] = {{0, 0}, {1, 0}, {1, 1}, {1, 2}, {1, 3}, {1, 4}, {2, 0}, {2, 2}};
  for (const auto& s : sets)
    if (s[0] == nt && s[1] == nx) return true;
  return false;
}

constexpr int kPairA[3] = {0, 0, 1}, kPairB[3] = {1, 2, 2};  // the axes of pair k

// Checks the descriptor and the call and builds the kernel's program.  *blocks is the grid, 0 when there is nothing to launch.
template <int LEVEL, class Desc>
int sys_parse(const char* who, const Desc* pde, const SysCall& a, SysProg<LEVEL>& p, int* blocks) {
  using L = SysLevel<LEVEL>;
  char msg[256];
  *blocks = 0;
#define SYS_BAD(...)                                   \
  do {                                                 \
    snprintf(msg, sizeof(msg), __VA_ARGS__);           \
    return pinn_internal_fail(PINN_ERR_BAD_DESC, msg); \
  } while (0)
  if (!pde) SYS_BAD("%s: null descriptor", who);
  const int dim = pde->dimension, C = pde->n_fields, E = pde->n_equations;
  if (dim < 1 || dim > 3) SYS_BAD("%s: dimension %d outside [1, 3]", who, dim);
  if (C < 1 || C > PINN_SYSTEM_MAX_FIELDS) SYS_BAD("%s: n_fields %d outside [1, %d]", who, C, PINN_SYSTEM_MAX_FIELDS);
  if (E < 1 || E > PINN_SYSTEM_MAX_EQUATIONS) SYS_BAD("%s: n_equations %d outside [1, %d]", who, E, PINN_SYSTEM_MAX_EQUATIONS);
  if (pde->n_terms < 0 || pde->n_terms > PINN_SYSTEM_MAX_TERMS)
    SYS_BAD("%s: n_terms %d outside [0, %d]", who, (int)pde->n_terms, PINN_SYSTEM_MAX_TERMS);
  [[maybe_unused]] int K = 0, KN = 0;
  [[maybe_unused]] bool any_param = false;
  if constexpr (L::kFns) {
    K = pde->n_functions;
    if (K < 0 || K > PINN_SYSTEM_MAX_FUNCTIONS) SYS_BAD("%s: n_functions %d outside [0, %d]", who, K, PINN_SYSTEM_MAX_FUNCTIONS);
  }
  if constexpr (L::kNl) {
    KN = pde->n_nonlinear;
    if (KN < 0 || KN > PINN_SYSTEM_MAX_NONLINEAR) SYS_BAD("%s: n_nonlinear %d outside [0, %d]", who, KN, PINN_SYSTEM_MAX_NONLINEAR);
  }
  memset(&p, 0, sizeof(p));
  if constexpr (L::kEff) {
    // the parameter maps: no index reaches the device unchecked (entries beyond n_terms / n_nonlinear are not read)
    const int P = pde->n_params;
    if (P < 0 || P > PINN_SYSTEM_MAX_PARAMS) SYS_BAD("%s: n_params %d outside [0, %d]", who, P, PINN_SYSTEM_MAX_PARAMS);
    for (int m = 0; m < pde->n_terms; ++m) {
      const int q = pde->coef_param[m];
      if (q < -1 || q >= P) SYS_BAD("%s: term %d: coef_param %d outside [-1, %d)", who, m, q, P);
      any_param = any_param || q >= 0;
    }
    for (int k = 0; k < KN; ++k) {
      static const char* const entry[3] = {"shift", "scale", "exponent"};
      for (int j = 0; j < 3; ++j) {
        const int q = pde->nl_param[k][j];
        if (q < -1 || q >= P) SYS_BAD("%s: nonlinear function %d: nl_param of its %s, %d, outside [-1, %d)", who, k, entry[j], q, P);
        any_param = any_param || q >= 0;
      }
      if (pde->nl_param[k][2] >= 0 && pde->nl_op[k] != PINN_NL_POW)
        SYS_BAD("%s: nonlinear function %d: a learnable exponent needs PINN_NL_POW (operation %d)", who, k, (int)pde->nl_op[k]);
    }
    p.n_params = P;
    for (int m = 0; m < PINN_SYSTEM_MAX_TERMS; ++m) p.coef_param[m] = (signed char)(m < pde->n_terms ? pde->coef_param[m] : -1);
    for (int k = 0; k < PINN_SYSTEM_MAX_NONLINEAR; ++k)
      for (int j = 0; j < 3; ++j) p.nl_param[3 * k + j] = (signed char)(k < KN ? pde->nl_param[k][j] : -1);
  }
  p.n_terms = pde->n_terms;
  p.n_eq = E;
  p.dim = dim;
  p.loss = pde->loss;
  p.huber_delta = pde->huber_delta;
  for (int c = 0; c < C; ++c) {
    const int nt = pde->time_order[c], nx0 = pde->space_order[c][0];
    if (!sys_set_compiled(nt, nx0)) SYS_BAD("%s: field %d: axis-0 stream set (nt=%d, nx=%d) is not compiled", who, c, nt, nx0);
    for (int ax = 1; ax < 3; ++ax) {
      const int so = pde->space_order[c][ax];
      if (so < 0 || so > (ax < dim ? 2 : 0))
        SYS_BAD("%s: field %d: space_order[%d] = %d outside [0, %d] (dimension %d)", who, c, ax, so, ax < dim ? 2 : 0, dim);
    }
    p.nt[c] = nt;
    p.nx0[c] = nx0;
    p.nx1[c] = pde->space_order[c][1];
    p.nx2[c] = pde->space_order[c][2];
    if constexpr (L::kPairs) {
      for (int k = 0; k < 3; ++k) {
        const int po = pde->pair_order[c][k];
        if (po != 0 && po != 2)
          SYS_BAD("%s: field %d: pair_order[%d] = %d on the pair of axes (%d, %d) (0 or 2)", who, c, k, po, kPairA[k], kPairB[k]);
        if (po != 0 && dim < 2)
          SYS_BAD("%s: field %d: pair_order[%d] = %d on the pair of axes (%d, %d) in dimension %d (a mixed derivative needs 2 or 3)", who, c, k,
                  po, kPairA[k], kPairB[k], dim);
        if (po != 0 && kPairB[k] >= dim)
          SYS_BAD("%s: field %d: pair_order[%d] = %d on the pair of axes (%d, %d), dimension %d", who, c, k, po, kPairA[k], kPairB[k], dim);
        if (po) p.pairs |= 1u << (3 * c + k);
      }
    }
  }
  for (int e = 0; e < E; ++e) {
    const float w = pde->eq_weight[e];
    if (!std::isfinite(w) || w < 0.0f) SYS_BAD("%s: eq_weight[%d] = %g is negative or not finite", who, e, (double)w);
    p.gw[e] = a.grad_scale * w;
    p.w[e] = (double)w;
  }
  // the slot of a factor that belongs to a field (a stream, sin / cos when `trig`, u_ab), checked against what the descriptor
  // holds; -1 with the message in msg.  `where` is "term m, factor f" or "nonlinear function k".
  auto field_slot = [&](const char* where, int code, int field, bool trig) -> int {
    const int vs = sys_value_slot<L>(code);
#define SYS_MSG(...) return (snprintf(msg, sizeof(msg), __VA_ARGS__), -1)
    if (L::kPairs && code >= PINN_TERM_UYYY && code <= PINN_TERM_UZZZZ)
      SYS_MSG("%s: %s: code %d (u_yyy, u_yyyy, u_zzz, u_zzzz): orders above 2 along y and z are not available in systems", who, where, code);
    if (L::kPairs && code >= PINN_TERM_UXXYY && code <= PINN_TERM_UYYZZ)
      SYS_MSG("%s: %s: code %d (u_xxyy, u_xxzz, u_yyzz): u_aabb is not available in systems", who, where, code);
    if (vs < 0)
      SYS_MSG("%s: %s: unknown factor code %d%s", who, where, code, L::kPairs ? "" : " (mixed derivatives are not available in systems)");
    if (!trig && (vs == 7 || vs == 8))
      SYS_MSG("%s: %s: the source (code %d) is neither a stream of a field nor an earlier nonlinear function", who, where, code);
    if (field >= C) SYS_MSG("%s: %s names field %d of %d", who, where, field, C);
    bool held = true;
    if (code < 7) held = sys_row0(code, p.nt[field], p.nx0[field]) >= 0;
    else if (code == PINN_TERM_UY || code == PINN_TERM_UYY) held = p.nx1[field] >= code - PINN_TERM_UY + 1;
    else if (code == PINN_TERM_UZ || code == PINN_TERM_UZZ) held = p.nx2[field] >= code - PINN_TERM_UZ + 1;
    if (vs >= 13) {  // MIXED on
      const int k = vs - 13;
      const int order[3] = {p.nx0[field], p.nx1[field], p.nx2[field]};
      const int po = (p.pairs >> (3 * field + k)) & 1u ? 2 : 0;
      if (po != 2 || order[kPairA[k]] < 2 || order[kPairB[k]] < 2)
        SYS_MSG("%s: %s names the mixed derivative (code %d) of field %d along the pair of axes (%d, %d), which needs "
                "pair_order[%d][%d] = 2 and order >= 2 on both axes (pair_order %d, orders %d, %d)", who, where, code, field, kPairA[k],
                kPairB[k], field, k, po, order[kPairA[k]], order[kPairB[k]]);
    }
    if (!held)
      SYS_MSG("%s: %s names a stream (code %d) that field %d (nt=%d, space orders %d, %d, %d) does not hold", who, where, code, field,
              p.nt[field], p.nx0[field], p.nx1[field], p.nx2[field]);
#undef SYS_MSG
    if (vs == 7 || vs == 8) p.uses_trig[field] = 1;
    return field * L::kVals + vs;
  };
  const int slot_fn = C * L::kVals, slot_w = slot_fn + kSyFns;  // SysLevel<LEVEL, C>::kFn and kW, C at run time
  char where[48];
  if constexpr (L::kNl) {
    // the nonlinear functions: operation and source of every declared one, named by a term or not
    for (int k = 0; k < KN; ++k) {
      const int op = pde->nl_op[k], byte = pde->nl_source[k];
      if (op < PINN_NL_EXP || op > PINN_NL_COS) SYS_BAD("%s: nonlinear function %d: unknown operation %d", who, k, op);
      if (byte < 0 || byte > 255) SYS_BAD("%s: nonlinear function %d: %d is not one byte (field * 32 + code)", who, k, byte);
      const int code = byte & 31, field = byte >> 5;
      int slot, acc;
      if (code == PINN_TERM_NL) {
        if (field >= k) SYS_BAD("%s: nonlinear function %d: its source, nonlinear function %d, is not an earlier one", who, k, field);
        slot = slot_w + field;
        acc = C * L::kAcc + field;
      } else if (code == PINN_TERM_X || code == PINN_TERM_Y || code == PINN_TERM_Z || code == PINN_TERM_T ||
                 (code >= PINN_TERM_FN0 && code <= PINN_TERM_FN3)) {
        SYS_BAD("%s: nonlinear function %d: the source (code %d) is neither a stream of a field nor an earlier nonlinear function", who, k,
                code);
      } else {
        snprintf(where, sizeof(where), "nonlinear function %d", k);
        slot = field_slot(where, code, field, false);
        if (slot < 0) return pinn_internal_fail(PINN_ERR_BAD_DESC, msg);
        acc = sys_target<L>((unsigned)slot);
      }
      p.nl_op |= (unsigned)op << (8 * k);
      p.nl_src |= (unsigned)slot << (8 * k);
      p.nl_acc |= (unsigned)acc << (8 * k);
    }
  }
  for (int m = 0; m < PINN_SYSTEM_MAX_TERMS; ++m) p.slots[m] = 0xffffffffu;
  for (int m = 0; m < pde->n_terms; ++m) {
    const PinnTermPdeTerm& tm = pde->terms[m];
    const int eq = pde->equation_of[m];
    if (eq < 0 || eq >= E) SYS_BAD("%s: equation_of[%d] = %d outside [0, %d)", who, m, eq, E);
    if (tm.n_factors < 0 || tm.n_factors > PINN_TERM_MAX_FACTORS)
      SYS_BAD("%s: term %d has n_factors %d outside [0, %d]", who, m, (int)tm.n_factors, PINN_TERM_MAX_FACTORS);
    unsigned packed = 0xffffffffu;
    for (int f = 0; f < tm.n_factors; ++f) {
      const int byte = tm.factor[f];
      if (byte < 0 || byte > 255) SYS_BAD("%s: term %d, factor %d: %d is not one byte (field * 32 + code)", who, m, f, byte);
      const int code = byte & 31, field = byte >> 5;
      int slot;
      if (code == PINN_TERM_X || code == PINN_TERM_Y || code == PINN_TERM_Z || code == PINN_TERM_T) {  // the field bits are ignored
        if ((code == PINN_TERM_Y && dim < 2) || (code == PINN_TERM_Z && dim < 3))
          SYS_BAD("%s: term %d, factor %d names a coordinate (code %d) that dimension %d does not hold", who, m, f, code, dim);
        p.uses_coord |= code == PINN_TERM_X ? USE_X : (code == PINN_TERM_Y ? USE_Y : (code == PINN_TERM_Z ? USE_Z : USE_T));
        slot = L::kCoord + (code == PINN_TERM_X ? 0 : (code == PINN_TERM_Y ? 1 : (code == PINN_TERM_Z ? 2 : 3)));
      } else if (L::kFns && code >= PINN_TERM_FN0 && code <= PINN_TERM_FN3) {  // the field bits are ignored here too
        const int k = code - PINN_TERM_FN0;
        if (k >= K) SYS_BAD("%s: term %d, factor %d names function %d (code %d) of %d (n_functions)", who, m, f, k, code, K);
        if constexpr (L::kFns) p.uses_fn |= 1 << k;
        slot = slot_fn + k;
      } else if (L::kNl && code == PINN_TERM_NL) {  // the field bits carry k
        if (field >= KN)
          SYS_BAD("%s: term %d, factor %d names nonlinear function %d (code %d) of %d (n_nonlinear)", who, m, f, field, code, KN);
        if constexpr (L::kNl) p.uses_nl |= 1 << field;
        slot = slot_w + field;
      } else {
        snprintf(where, sizeof(where), "term %d, factor %d", m, f);
        slot = field_slot(where, code, field, true);
        if (slot < 0) return pinn_internal_fail(PINN_ERR_BAD_DESC, msg);
      }
      packed = (packed & ~(255u << (8 * f))) | ((unsigned)slot << (8 * f));
    }
    p.slots[m] = packed;
    p.n_factors[m] = (unsigned char)tm.n_factors;
    p.eq[m] = (unsigned char)eq;
  }
  // the mask: the functions a term names, closed under "is the source of a masked function" (sources are earlier: descending k)
  if constexpr (L::kNl) {
    for (int k = KN - 1; k > 0; --k) {
      const unsigned src = (p.nl_src >> (8 * k)) & 255u;
      if (((p.uses_nl >> k) & 1) && src >= (unsigned)slot_w) p.uses_nl |= 1 << (int)(src - slot_w);
    }
  }
  if (a.N < 0) SYS_BAD("%s: N < 0", who);
  if (a.N == 0) return PINN_OK;
  if (!a.jets || !a.coef_values) SYS_BAD("%s: null jets table or coef_values", who);
  for (int c = 0; c < C; ++c) {
    const int so[3] = {1, p.nx1[c], p.nx2[c]};  // block (c, 0) always holds the value stream
    for (int ax = 0; ax < 3; ++ax) {
      const bool need = ax < dim && so[ax] > 0;
      p.jets[3 * c + ax] = need ? a.jets[3 * c + ax] : nullptr;
      p.cot[3 * c + ax] = (a.jet_cotangents && need) ? a.jet_cotangents[3 * c + ax] : nullptr;
      if (need && (!p.jets[3 * c + ax] || (a.jet_cotangents && !p.cot[3 * c + ax])))
        SYS_BAD("%s: null block (field %d, axis %d) of the jets or jet_cotangents table", who, c, ax);
    }
    if constexpr (L::kPairs) {
      for (int k = 0; k < 3; ++k) {
        const int b = 3 * C + 3 * c + k;
        const bool need = (p.pairs >> (3 * c + k)) & 1u;
        p.jets[b] = need ? a.jets[b] : nullptr;
        p.cot[b] = (a.jet_cotangents && need) ? a.jet_cotangents[b] : nullptr;
        if (need && (!p.jets[b] || (a.jet_cotangents && !p.cot[b])))
          SYS_BAD("%s: null block %d of the jets or jet_cotangents table (the P block of field %d, pair of axes (%d, %d))", who, b, c,
                  kPairA[k], kPairB[k]);
      }
    }
  }
  if (((p.uses_coord & (USE_X | USE_Y | USE_Z)) && !a.x) || ((p.uses_coord & USE_T) && !a.t))
    SYS_BAD("%s: a term names X / Y / Z / T but the coordinate array is null", who);
  if (p.uses_fn && !a.fn_values) {
    int m = 0, k = 0;  // the first term that names a function, for the message
    for (; m < pde->n_terms; ++m) {
      bool found = false;
      for (int f = 0; f < p.n_factors[m] && !found; ++f) {
        const int slot = (int)((p.slots[m] >> (8 * f)) & 255u);
        if (slot >= slot_fn && slot < slot_w) found = true, k = slot - slot_fn;
      }
      if (found) break;
    }
    SYS_BAD("%s: term %d names function %d but fn_values is null", who, m, k);
  }
  if (p.uses_nl && !a.nl_params) {
    int k = 0;
    while (!((p.uses_nl >> k) & 1)) ++k;
    SYS_BAD("%s: nonlinear function %d is evaluated but nl_params is null", who, k);
  }
  if constexpr (L::kEff) {
    if (any_param && !a.param_values) {
      for (int m = 0; m < pde->n_terms; ++m)
        if (pde->coef_param[m] >= 0) SYS_BAD("%s: term %d has a learnable coefficient but param_values is null", who, m);
      int k = 0;
      while (pde->nl_param[k][0] < 0 && pde->nl_param[k][1] < 0 && pde->nl_param[k][2] < 0) ++k;
      SYS_BAD("%s: nonlinear function %d has a learnable entry but param_values is null", who, k);
    }
    if (a.param_grads && !a.scratch) SYS_BAD("%s: param_grads without scratch", who);
  }
  if (a.reduce() && !a.scratch) SYS_BAD("%s: null scratch with a loss or coefficient sum", who);
#undef SYS_BAD
  if (reinterpret_cast<uintptr_t>(a.scratch) & 7u) {
    snprintf(msg, sizeof(msg), "%s: scratch must be 8-byte aligned", who);
    return pinn_internal_fail(PINN_ERR_MISALIGNED, msg);
  }
  const long long nb = (a.N + 255) / 256;
  *blocks = (int)(nb > kSyBlocks ? kSyBlocks : nb);
  return PINN_OK;
}

template <int LEVEL, int C, bool REDUCE, bool COEF, bool NLP>
void sys_launch_form(const SysProg<LEVEL>& p, int blocks, const SysCall& a) {
  using F = const float;
  const dim3 grid(blocks), block(256);
  if constexpr (LEVEL == INV)
    hipLaunchKernelGGL((term_system_kernel<LEVEL, C, REDUCE, COEF, NLP, F, F, F>), grid, block, 0, a.stream, p, a.coef_values, a.x, a.t,
                       a.fn_values, a.nl_params, a.param_values, a.N, a.residual_cotangent, a.residual_out, a.scratch);
  else if constexpr (LEVEL == NL)
    hipLaunchKernelGGL((term_system_kernel<LEVEL, C, REDUCE, COEF, NLP, F, F>), grid, block, 0, a.stream, p, a.coef_values, a.x, a.t,
                       a.fn_values, a.nl_params, a.N, a.residual_cotangent, a.residual_out, a.scratch);
  else if constexpr (LEVEL == FN)
    hipLaunchKernelGGL((term_system_kernel<LEVEL, C, REDUCE, COEF, NLP, F>), grid, block, 0, a.stream, p, a.coef_values, a.x, a.t,
                       a.fn_values, a.N, a.residual_cotangent, a.residual_out, a.scratch);
  else
    hipLaunchKernelGGL((term_system_kernel<LEVEL, C, REDUCE, COEF, NLP>), grid, block, 0, a.stream, p, a.coef_values, a.x, a.t, a.N,
                       a.residual_cotangent, a.residual_out, a.scratch);
}

template <int LEVEL, int C>
void sys_launch_fields(const SysProg<LEVEL>& p, int blocks, const SysCall& a, bool nl_sums) {
  if (!a.reduce()) return sys_launch_form<LEVEL, C, false, false, false>(p, blocks, a);
  if constexpr (LEVEL == INV)
    if (nl_sums) return sys_launch_form<LEVEL, C, true, true, true>(p, blocks, a);
  if (a.coef_sums()) return sys_launch_form<LEVEL, C, true, true, false>(p, blocks, a);
  sys_launch_form<LEVEL, C, true, false, false>(p, blocks, a);
}

// the element-wise launch; nl_sums (INV): the sums H_kj are wanted too
template <int LEVEL>
int sys_launch(const char* who, const SysProg<LEVEL>& p, int C, int blocks, const SysCall& a, bool nl_sums = false) {
  switch (C) {
    case 1: sys_launch_fields<LEVEL, 1>(p, blocks, a, nl_sums); break;
    case 2: sys_launch_fields<LEVEL, 2>(p, blocks, a, nl_sums); break;
    case 3: sys_launch_fields<LEVEL, 3>(p, blocks, a, nl_sums); break;
    default: sys_launch_fields<LEVEL, 4>(p, blocks, a, nl_sums); break;
  }
  return sys_launched(who, "term_system_kernel");
}

// PLAIN .. NL: parse, launch, finish
template <int LEVEL, class Desc>
int sys_residual(const char* who, const Desc* pde, const SysCall& a) {
  SysProg<LEVEL> p;
  int blocks;
  int rc = sys_parse<LEVEL>(who, pde, a, p, &blocks);
  if (rc || !blocks) return rc;
  rc = sys_launch<LEVEL>(who, p, pde->n_fields, blocks, a);
  if (rc || !a.reduce()) return rc;
  hipLaunchKernelGGL(term_system_finish_kernel<SysLevel<LEVEL>::kRow>, dim3(1), dim3(64), 0, a.stream, a.scratch, blocks, p.n_eq, p.n_terms,
                     p.w[0], p.w[1], p.w[2], p.w[3], a.loss_sum_out, a.eq_loss_sums, a.coef_grads);
  return sys_launched(who, "term_system_finish_kernel");
}

}  // namespace
