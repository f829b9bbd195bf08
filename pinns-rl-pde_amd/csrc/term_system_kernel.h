// The element-wise kernel of the coupled-system residuals, one source for the five entry points pinn_term_residual_system,
// _mixed, _fn, _nl and _inv (include/pinn_jet.h).  sys_loss below is term_kernels.hip::term_loss, the same function.
//   one pinn_jet_forward per (field, axis with streams) and per (field, pair of order 2: a component launch along e_a + e_b)
//   -> pinn_term_residual_system* -> one pinn_jet_backward per block,
// where field c of a C-output network is a component launch.  One thread per point per grid-stride round, the term list in the
// kernel arguments, per-block partials in double summed in block order.  A point's numbers (up to 4 x 16 values and 4 x 14
// derivative accumulators) sit in LDS, one column per thread, and a factor's slot is a wave-uniform row offset into it.  No
// thread reads another's column: there is no barrier in the point loop.
//
// The levels are cumulative, PLAIN < MIXED < FN < NL < INV, and a level compiles only what it has (SysLevel, `if constexpr`):
//   MIXED  three more value rows per field, u_xy, u_xz, u_yz, derived at load by u_ab = 0.5f * ((P_2 - A_2) - B_2), and three
//          more accumulators, their cotangents g, which the write-out spreads over row 2 of the P block and the order-2 rows
//          of the two axis blocks
//   FN     up to four known functions g_k(x, t): row 16 C + k, read once per round if a term names it; no cotangent target
//   NL     up to four w_k = g_k(shift + scale * s_k) in ascending k: row 16 C + 4 + k, d_k = g_k'(arg) * scale in row
//          16 C + 8 + k, a cotangent target of its own (accumulator 14 C + k) pushed to its source in descending k
//   INV    coefficients and triples are the stored value or the stored value times a parameter (one rounding), formed once per
//          block into LDS; with NLP the sums H_kj of the learnable nonlinear entries, for which row 16 C + 8 + k holds the
//          slope without the scale and d_k is formed at the push (the same single rounding)
// The order of every product and sum, and which expressions are statements of their own, is what the fp32 models of
// tests/term_system*_model.py reproduce bit for bit.  Resources per instantiation: profiles/term_system_one_source.md.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "../../include/pinn_jet.h"

extern "C" int pinn_internal_fail(int code, const char* msg);  // pinn_abi.hip: sets pinn_last_error()

namespace {

enum SysLevelId { PLAIN, MIXED, FN, NL, INV };

constexpr int kSyBlocks = 64;                                               // fixed grid: the partials are summed in block order
constexpr int kSyG = PINN_SYSTEM_MAX_EQUATIONS;                             // partial rows 0 .. 3: equation loss sums
constexpr int kSyH = PINN_SYSTEM_MAX_EQUATIONS + PINN_SYSTEM_MAX_TERMS;     // rows 4 .. 35: coefficient sums G_m
constexpr int kSyNlp = 3 * PINN_SYSTEM_MAX_NONLINEAR;                       // INV, rows 36 .. 47: the sums H_kj, k * 3 + j
constexpr int kSyEff = PINN_SYSTEM_MAX_TERMS + kSyNlp;                      // INV, effective values in LDS: c_m, then the triples
constexpr int kSyFns = PINN_SYSTEM_MAX_FUNCTIONS;
constexpr int kSyNl = PINN_SYSTEM_MAX_NONLINEAR;

static_assert(PINN_SYSTEM_SCRATCH_DOUBLES == kSyBlocks * kSyH, "scratch constant and grid disagree");
static_assert(PINN_SYSTEM_INV_SCRATCH_DOUBLES == kSyBlocks * (kSyH + kSyNlp), "scratch constant and grid disagree");
static_assert(PINN_SYSTEM_MAX_FIELDS == 4 && PINN_SYSTEM_MAX_EQUATIONS == 4, "the kernel unrolls over four fields and four equations");
static_assert(PINN_SYSTEM_MAX_FUNCTIONS == 4 && PINN_TERM_FN3 - PINN_TERM_FN0 == 3, "four known functions");
static_assert(PINN_SYSTEM_MAX_NONLINEAR == 4 && PINN_TERM_NL == 31, "four nonlinear functions, named by code 31");
static_assert(PINN_SYSTEM_MAX_PARAMS == 8 && kSyEff + PINN_SYSTEM_MAX_PARAMS <= 64, "one finish thread per sum");

enum { USE_X = 1, USE_Y = 2, USE_Z = 4, USE_T = 8 };

// What a level has, and the rows of a thread's LDS columns for C fields.  A factor's slot is field * kVals + value slot,
// kFn + k the known function g_k, kW + k the nonlinear function w_k, kCoord .. kCoord + 3 a coordinate, 255 unused.
template <int LEVEL, int C = PINN_SYSTEM_MAX_FIELDS>
struct SysLevel {
  static constexpr bool kPairs = LEVEL >= MIXED, kFns = LEVEL >= FN, kNl = LEVEL >= NL, kEff = LEVEL == INV;
  static constexpr int kVals = kPairs ? 16 : 13;  // value slots of a field: codes 0 .. 6, sin, cos, u_y, u_yy, u_z, u_zz[, u_xy, u_xz, u_yz]
  static constexpr int kAcc = kPairs ? 14 : 11;   // derivative accumulators: codes 0 .. 6, u_y, u_yy, u_z, u_zz[, g of the three pairs]
  static constexpr int kBlocks = (kPairs ? 6 : 3) * PINN_SYSTEM_MAX_FIELDS;  // block pointers in the kernel arguments
  static constexpr int kFn = C * kVals, kW = kFn + (kFns ? kSyFns : 0), kD = kW + (kNl ? kSyNl : 0);
  static constexpr int kValRows = kD + (kNl ? kSyNl : 0);
  static constexpr int kWbar = C * kAcc, kAccRows = kWbar + (kNl ? kSyNl : 0);
  static constexpr int kCoord = PINN_SYSTEM_MAX_FIELDS * kVals + (kD - kFn);  // 52, 64, 68, 72, 72: x, y, z, t (registers, not LDS)
  static constexpr int kRow = kEff ? kSyH + kSyNlp : kSyH;                    // doubles per block of the partials
  // Register pressure, not arithmetic; each choice was made by building all instantiations and reading their resource usage
  // (no scratch memory, no spilled vector register: the Makefile refuses either).  From MIXED on the field loops run one field
  // after the other, so that only one field's block pointers are held in scalar registers at a time.  From FN on the term
  // index of the coefficient sums goes through an opaque scalar once per round: otherwise the descriptor loads of all 32 terms
  // are hoisted out of the grid-stride loop and held in scalar registers across it, which, with the function rows, no longer
  // fit (they spilled into scratch memory).  MIXED with coefficient sums has neither: it holds all 32 terms in scalar
  // registers (over 1000 scalar spills into vector lanes), and with serial field loops or the opaque index the allocator left
  // a dead 20-byte stack slot behind, which makes the kernel reserve scratch, or spilled a vector register.  With unrolled field loops and a compiler fence
  // between the loads and the sweeps (these forms alone: in the others the fence costs 0.2 - 0.3 us of a 18 us call) it does not.
  static constexpr int field_unroll(bool coef) { return kFns || (kPairs && !coef) ? 1 : C; }
  static constexpr bool load_fence(bool coef) { return kPairs && !kFns && coef; }
  static constexpr bool kOpaqueTerm = kFns;
};

// the parameter maps of INV: -1, or the parameter an entry is a multiple of (checked on the host)
struct SysParamMap {
  int n_params;
  signed char coef_param[PINN_SYSTEM_MAX_TERMS];
  signed char nl_param[kSyNlp];  // entry j of the triple of function k, at 3 k + j
};

// What only some levels have in the kernel arguments, as bases of SysProg: a level without a part has an empty base whose
// constants read as "none", so PLAIN's argument block is the common members alone.
template <bool HAS> struct SysPairPart { static constexpr unsigned pairs = 0; };
template <> struct SysPairPart<true> {
  unsigned pairs;                             // bit 3 c + k: field c has pair k of (x,y), (x,z), (y,z) (pair_order 2)
};
template <bool HAS> struct SysFnPart { static constexpr int uses_fn = 0; };
template <> struct SysFnPart<true> {
  int uses_fn;                                // bit k: a term names g_k (a row no term names is never read)
};
template <bool HAS> struct SysNlPart { static constexpr int uses_nl = 0; static constexpr unsigned nl_src = 0; };
template <> struct SysNlPart<true> {
  int uses_nl;                                // bit k: w_k is evaluated (named by a term, or the source of such a function)
  unsigned nl_op, nl_src, nl_acc;             // byte k: PINN_NL_* of w_k, the slot of its source, the accumulator of its source
};
struct SysNoParamMap {};

// the descriptor as the kernel reads it
template <int LEVEL>
struct SysProg : SysPairPart<(LEVEL >= MIXED)>, SysFnPart<(LEVEL >= FN)>, SysNlPart<(LEVEL >= NL)>,
                 std::conditional_t<LEVEL == INV, SysParamMap, SysNoParamMap> {
  int n_terms, n_eq, dim, loss;
  float huber_delta;
  int uses_coord;
  int nt[PINN_SYSTEM_MAX_FIELDS], nx0[PINN_SYSTEM_MAX_FIELDS], nx1[PINN_SYSTEM_MAX_FIELDS], nx2[PINN_SYSTEM_MAX_FIELDS];
  int uses_trig[PINN_SYSTEM_MAX_FIELDS];
  float gw[PINN_SYSTEM_MAX_EQUATIONS];        // grad_scale * eq_weight[e], rounded once on the host
  double w[PINN_SYSTEM_MAX_EQUATIONS];        // eq_weight[e]
  unsigned slots[PINN_SYSTEM_MAX_TERMS];      // byte f = slot of factor f
  unsigned char n_factors[PINN_SYSTEM_MAX_TERMS];
  unsigned char eq[PINN_SYSTEM_MAX_TERMS];
  const float* jets[SysLevel<LEVEL>::kBlocks];  // 3 c + a: axis block (c, a);  3 C + 3 c + k: the P block of (c, pair k)
  float* cot[SysLevel<LEVEL>::kBlocks];       // all null when no cotangents are wanted
};

// l(r) and l'(r) of PDEBase._apply_loss_fn per sample
__device__ __forceinline__ float sys_loss(int kind, float d, float r, float* dl) {
  if (kind == PINN_LOSS_MAE) {
    *dl = r > 0.0f ? 1.0f : (r < 0.0f ? -1.0f : 0.0f);
    return fabsf(r);
  }
  if (kind == PINN_LOSS_HUBER) {
    const float a = fabsf(r);
    if (a < d) {
      *dl = r;
      return 0.5f * r * r;
    }
    *dl = r > 0.0f ? d : -d;
    return d * (a - 0.5f * d);
  }
  *dl = 2.0f * r;
  return r * r;
}

// row of block (c, 0) that holds code s (0 .. 6) in the (nt, nx) set, or -1 when the set does not hold it
__host__ __device__ inline int sys_row0(int code, int nt, int nx) {
  if (code == 0) return 0;
  if (code <= 2) return code <= nt ? code : -1;
  return code - 2 <= nx ? nt + code - 2 : -1;
}

// value slot (0 .. kVals - 1) of a stream / trig / mixed code, or -1 for any other code
template <class L>
int sys_value_slot(int code) {
  if (code >= 0 && code <= 6) return code;
  if (code == PINN_TERM_SIN_U) return 7;
  if (code == PINN_TERM_COS_U) return 8;
  if (code >= PINN_TERM_UY && code <= PINN_TERM_UZZ) return 9 + (code - PINN_TERM_UY);
  if (L::kPairs && code >= PINN_TERM_UXY && code <= PINN_TERM_UYZ) return 13 + (code - PINN_TERM_UXY);
  return -1;
}

// accumulator (field * kAcc + k) the derivative of a value slot goes to: u, sin(u) and cos(u) all go to the value stream
template <class L>
__host__ __device__ inline int sys_target(unsigned slot) {
  const int c = (int)slot / L::kVals, v = (int)slot - c * L::kVals;
  return c * L::kAcc + (v < 7 ? v : (v < 9 ? 0 : v - 2));
}

// the value of a slot: a wave-uniform row of this thread's LDS column (a field's value or a function), or a coordinate register
template <class L>
__device__ __forceinline__ float sys_value(const float* col, unsigned slot, float cx, float cy, float cz, float ct) {
  if (slot < (unsigned)L::kCoord) return col[slot * 256];
  switch (slot - L::kCoord) {
    case 0: return cx;
    case 1: return cy;
    case 2: return cz;
    default: return ct;
  }
}

// One float per equation, handed between the stages by value: an array that a stage reached through a reference and indexed
// by a term's equation would stay in memory (scratch, or LDS the compiler takes for it) instead of four registers.
struct SysEq {
  float v[PINN_SYSTEM_MAX_EQUATIONS];
};

// rbar of the term's equation
__device__ __forceinline__ float sys_rbar_of(SysEq rbar, int eq) {
  float rb = rbar.v[0];
#pragma unroll
  for (int e = 1; e < PINN_SYSTEM_MAX_EQUATIONS; ++e)
    if (e == eq) rb = rbar.v[e];
  return rb;
}

// INV: the effective values, once per block: thread m < 32 the coefficient of term m, thread 32 + 3 k + j entry j of the triple
// of function k (only inside the mask: the parameters of a function that is not evaluated are never read).  The index was
// checked against n_params on the host.
template <class Prog>
__device__ __forceinline__ void sys_effective(const Prog& p, const float* coef_in, const float* nlp_in, const float* pv, float* seff) {
  if (threadIdx.x < kSyEff) {
    const int i = threadIdx.x;
    float v = 0.0f;
    if (i < PINN_SYSTEM_MAX_TERMS) {
      if (i < p.n_terms) {
        const int q = p.coef_param[i];
        v = q < 0 ? coef_in[i] : __fmul_rn(coef_in[i], pv[q]);
      }
    } else {
      const int kj = i - PINN_SYSTEM_MAX_TERMS;
      if ((p.uses_nl >> (kj / 3)) & 1) {
        const int q = p.nl_param[kj];
        v = q < 0 ? nlp_in[kj] : __fmul_rn(nlp_in[kj], pv[q]);
      }
    }
    seff[i] = v;
  }
  __syncthreads();
}

// ---- the values of every field, the derived u_ab in the evaluation order the header states ----
template <class L, int C, int UNROLL, class Prog>
__device__ __forceinline__ void sys_load_fields(const Prog& p, float* vcol, long long N, long long n) {
#pragma unroll UNROLL
  for (int c = 0; c < C; ++c) {
    const float* __restrict__ j0 = p.jets[3 * c];
    float* v = vcol + c * L::kVals * 256;
#pragma unroll
    for (int s = 0; s < 7; ++s) {
      const int row = sys_row0(s, p.nt[c], p.nx0[c]);
      v[s * 256] = row >= 0 ? j0[(long long)row * N + n] : 0.0f;
    }
    if (p.uses_trig[c]) {
      const float u = v[0];
      v[7 * 256] = sinf(u);
      v[8 * 256] = cosf(u);
    }
    const float* __restrict__ j1 = p.jets[3 * c + 1];
    const float* __restrict__ j2 = p.jets[3 * c + 2];
    v[9 * 256] = p.nx1[c] >= 1 ? j1[N + n] : 0.0f;
    v[10 * 256] = p.nx1[c] >= 2 ? j1[2 * N + n] : 0.0f;
    v[11 * 256] = p.nx2[c] >= 1 ? j2[N + n] : 0.0f;
    v[12 * 256] = p.nx2[c] >= 2 ? j2[2 * N + n] : 0.0f;
    if constexpr (L::kPairs) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float* __restrict__ pk = p.jets[3 * C + 3 * c + k];
        const int sa = k == 2 ? 10 : 4, sb = k == 0 ? 10 : 12;  // value slots of the order-2 rows of the pair's two axes
        v[(13 + k) * 256] = ((p.pairs >> (3 * c + k)) & 1u) ? 0.5f * ((pk[2 * N + n] - v[sa * 256]) - v[sb * 256]) : 0.0f;
      }
    }
  }
}

// ---- function k at fn + k N; the mask is the host's, so a row that no term names is not touched (its LDS row is never read).
// Not unrolled: unrolled, the C = 3 and C = 4 forms with coefficient sums reserved scratch memory ----
template <class L, class Prog>
__device__ __forceinline__ void sys_load_functions(const Prog& p, float* vcol, const float* fn, long long N, long long n) {
#pragma unroll 1
  for (int k = 0; k < kSyFns; ++k)
    if ((p.uses_fn >> k) & 1) vcol[(L::kFn + k) * 256] = fn[(long long)k * N + n];
}

// ---- the nonlinear functions in ascending k (a source may be an earlier one); outside the mask neither evaluated nor are its
// parameters read.  The operation is wave-uniform ----
template <class L, bool NLP, class Prog>
__device__ __forceinline__ void sys_eval_nonlinear(const Prog& p, float* vcol, const float* nlp, bool want_cot) {
  if (!p.uses_nl) return;
#pragma unroll 1
  for (int k = 0; k < kSyNl; ++k) {
    if (!((p.uses_nl >> k) & 1)) continue;
    const float shift = nlp[3 * k], scale = nlp[3 * k + 1];
    const float arg = fmaf(scale, vcol[((p.nl_src >> (8 * k)) & 255u) * 256], shift);
    float w, slope;
    switch ((p.nl_op >> (8 * k)) & 255u) {
      case PINN_NL_EXP: w = expf(arg); slope = w; break;
      case PINN_NL_LOG: w = logf(arg); slope = 1.0f / arg; break;
      case PINN_NL_RECIP: w = 1.0f / arg; slope = -(w * w); break;
      case PINN_NL_SQRT: w = sqrtf(arg); slope = 0.5f / w; break;
      case PINN_NL_POW: {
        const float e = nlp[3 * k + 2];
        w = powf(arg, e);
        slope = want_cot ? e * powf(arg, e - 1.0f) : 0.0f;
        break;
      }
      case PINN_NL_TANH: w = tanhf(arg); slope = 1.0f - w * w; break;
      case PINN_NL_SINH: w = sinhf(arg); slope = want_cot ? coshf(arg) : 0.0f; break;
      case PINN_NL_COSH: w = coshf(arg); slope = want_cot ? sinhf(arg) : 0.0f; break;
      case PINN_NL_SIN: w = sinf(arg); slope = want_cot ? cosf(arg) : 0.0f; break;
      default: w = cosf(arg); slope = want_cot ? -sinf(arg) : 0.0f; break;
    }
    vcol[(L::kW + k) * 256] = w;
    if constexpr (L::kEff) {
      if (want_cot) vcol[(L::kD + k) * 256] = NLP ? slope : __fmul_rn(slope, scale);
    } else {
      if (want_cot) vcol[(L::kD + k) * 256] = slope * scale;
    }
  }
}

// ---- sweep 1: r_e = sum_{m: equation_of[m] = e} c_m prod_f phi_{m,f}, terms in ascending m ----
template <class L, class Prog>
__device__ __forceinline__ SysEq sys_sweep1(const Prog& p, const float* vcol, float cx, float cy, float cz, float ct, const float* coef) {
  SysEq r;
#pragma unroll
  for (int e = 0; e < PINN_SYSTEM_MAX_EQUATIONS; ++e) r.v[e] = 0.0f;
  for (int m = 0; m < p.n_terms; ++m) {
    const unsigned slots = p.slots[m];
    const int nf = p.n_factors[m];
    const int eq = p.eq[m];
    float prod = coef[m];
#pragma unroll
    for (int f = 0; f < PINN_TERM_MAX_FACTORS; ++f)
      if (f < nf) prod *= sys_value<L>(vcol, (slots >> (8 * f)) & 255u, cx, cy, cz, ct);
#pragma unroll
    for (int e = 0; e < PINN_SYSTEM_MAX_EQUATIONS; ++e)
      if (e == eq) r.v[e] += prod;
  }
  return r;
}

// ---- the loss and rbar_e of every equation ----
template <bool REDUCE, class Prog>
__device__ __forceinline__ SysEq sys_loss_rbar(const Prog& p, SysEq r, const float* rbar_in, float* residual_out, long long N, long long n,
                                               double (&loss_acc)[PINN_SYSTEM_MAX_EQUATIONS]) {
  SysEq rbar;
#pragma unroll
  for (int e = 0; e < PINN_SYSTEM_MAX_EQUATIONS; ++e) {
    rbar.v[e] = 0.0f;
    if (e < p.n_eq) {
      float dl;
      const float lv = sys_loss(p.loss, p.huber_delta, r.v[e], &dl);
      rbar.v[e] = rbar_in ? rbar_in[(long long)e * N + n] : p.gw[e] * dl;
      if (residual_out) residual_out[(long long)e * N + n] = r.v[e];
      if (REDUCE) loss_acc[e] += (double)lv;
    }
  }
  return rbar;
}

// ---- sweep 2: terms in ascending m again.  The derivative summands of ONE term that go to the same (field, stream)
// accumulator (at most four) are summed first, in ascending factor order, multiplied by rbar of the term's equation and
// then added to the accumulator ----
template <class L, class Prog>
__device__ __forceinline__ void sys_sweep2(const Prog& p, const float* vcol, float* acol, float cx, float cy, float cz, float ct,
                                           const float* coef, SysEq rbar) {
#pragma unroll
  for (int k = 0; k < L::kAccRows; ++k) acol[k * 256] = 0.0f;
  for (int m = 0; m < p.n_terms; ++m) {
    const float c = coef[m];
    const unsigned slots = p.slots[m];
    const int nf = p.n_factors[m];
    const float rb = sys_rbar_of(rbar, p.eq[m]);
    float phi[PINN_TERM_MAX_FACTORS];
#pragma unroll
    for (int f = 0; f < PINN_TERM_MAX_FACTORS; ++f) phi[f] = f < nf ? sys_value<L>(vcol, (slots >> (8 * f)) & 255u, cx, cy, cz, ct) : 1.0f;
    // contribution of factor f to its target: c * prod_{g != f} phi_g, times cos(u) / -sin(u) under sin(u) / cos(u)
    float contrib[PINN_TERM_MAX_FACTORS];
    int target[PINN_TERM_MAX_FACTORS];
#pragma unroll
    for (int f = 0; f < PINN_TERM_MAX_FACTORS; ++f) {
      contrib[f] = 0.0f;
      target[f] = -1;
      const unsigned slot = (slots >> (8 * f)) & 255u;
      const bool is_nl = L::kNl && slot >= (unsigned)L::kW && slot < (unsigned)L::kD;
      if (f < nf && (slot < (unsigned)L::kFn || is_nl)) {  // coordinates and known functions carry no cotangent
        float others = c;
#pragma unroll
        for (int g = 0; g < PINN_TERM_MAX_FACTORS; ++g)
          if (g != f && g < nf) others *= phi[g];
        if (is_nl) {  // w_k: a target of its own
          contrib[f] = others;
          target[f] = L::kWbar + ((int)slot - L::kW);
        } else {
          const int fc = (int)slot / L::kVals, fv = (int)slot - fc * L::kVals;
          if (fv == 7) others = others * vcol[(fc * L::kVals + 8) * 256];
          else if (fv == 8) others = -(others * vcol[(fc * L::kVals + 7) * 256]);
          contrib[f] = others;
          target[f] = sys_target<L>(slot);
        }
      }
    }
#pragma unroll
    for (int f = 0; f < PINN_TERM_MAX_FACTORS; ++f) {
      if (target[f] < 0) continue;
      bool first = true;
#pragma unroll
      for (int g = 0; g < f; ++g)
        if (target[g] == target[f]) first = false;
      if (!first) continue;  // summed with the first factor of this target
      float sum = 0.0f;
#pragma unroll
      for (int g = f; g < PINN_TERM_MAX_FACTORS; ++g)
        if (target[g] == target[f]) sum += contrib[g];
      acol[target[f] * 256] += rb * sum;
    }
  }
}

// ---- the cotangents of the nonlinear functions go to their sources, in descending k: wbar_k * d_k, rounded, then added.
// With NLP the same pushes, unrolled so that hg[] stays in registers.  When function k is pushed its accumulator is complete
// (the later functions have pushed already): wbar_k.  Row kD + k holds the slope without the scale then.
//   H_k0 += wbar slope,  H_k1 += (wbar slope) s,  H_k2 += (wbar w) logf(arg)  (POW only), each product rounded ----
template <class L, bool NLP, class Prog>
__device__ __forceinline__ void sys_push_nonlinear(const Prog& p, const float* vcol, float* acol, const float* nlp,
                                                   double (&hg)[NLP ? kSyNlp : 1]) {
  if constexpr (NLP) {
#pragma unroll
    for (int k = kSyNl - 1; k >= 0; --k) {
      if ((p.uses_nl >> k) & 1) {
        const float wbar = acol[(L::kWbar + k) * 256];
        const float slope = vcol[(L::kD + k) * 256];
        const float scale = nlp[3 * k + 1];
        const float push = __fmul_rn(wbar, __fmul_rn(slope, scale));
        acol[((p.nl_acc >> (8 * k)) & 255u) * 256] += push;
        const float s = vcol[((p.nl_src >> (8 * k)) & 255u) * 256];
        const float h0 = __fmul_rn(wbar, slope);
        if (p.nl_param[3 * k] >= 0) hg[3 * k] += (double)h0;
        if (p.nl_param[3 * k + 1] >= 0) hg[3 * k + 1] += (double)__fmul_rn(h0, s);
        if (p.nl_param[3 * k + 2] >= 0) {  // POW, checked on the host
          const float arg = fmaf(scale, s, nlp[3 * k]);
          hg[3 * k + 2] += (double)__fmul_rn(__fmul_rn(wbar, vcol[(L::kW + k) * 256]), logf(arg));
        }
      }
    }
  } else if (p.uses_nl) {
#pragma unroll 1
    for (int k = kSyNl - 1; k >= 0; --k) {
      if (!((p.uses_nl >> k) & 1)) continue;
      const float push = __fmul_rn(acol[(L::kWbar + k) * 256], vcol[(L::kD + k) * 256]);
      acol[((p.nl_acc >> (8 * k)) & 255u) * 256] += push;
    }
  }
}

// ---- the coefficient sums: rbar_e(m) prod_f phi_{m,f}, the product from 1.0f in ascending f.  The loop is unrolled so that
// cg[] stays in registers ----
template <class L, class Prog>
__device__ __forceinline__ void sys_coef_sums(const Prog& p, const float* vcol, float cx, float cy, float cz, float ct,
                                              SysEq rbar, double (&cg)[PINN_SYSTEM_MAX_TERMS]) {
  int mb = 0;
  if constexpr (L::kOpaqueTerm) asm volatile("" : "+s"(mb));
#pragma unroll
  for (int m = 0; m < PINN_SYSTEM_MAX_TERMS; ++m) {
    if (m < p.n_terms) {
      const unsigned slots = p.slots[mb + m];
      const int nf = p.n_factors[mb + m];
      const float rb = sys_rbar_of(rbar, p.eq[mb + m]);
      float prod = 1.0f;
#pragma unroll
      for (int f = 0; f < PINN_TERM_MAX_FACTORS; ++f)
        if (f < nf) prod *= sys_value<L>(vcol, (slots >> (8 * f)) & 255u, cx, cy, cz, ct);
      cg[m] += (double)(rb * prod);
    }
  }
}

// ---- the cotangent blocks: every row of every block is written.  The transposed polarisation first, per field and in
// ascending pair index: p_k = g_k / 2 to row 2 of the P block, and subtracted from the order-2 accumulators of the pair's
// two axes (accumulators 4, 8, 10: u_xx, u_yy, u_zz) ----
template <class L, int C, int UNROLL, class Prog>
__device__ __forceinline__ void sys_write_cotangents(const Prog& p, float* acol, long long N, long long n) {
#pragma unroll UNROLL
  for (int c = 0; c < C; ++c) {
    float* a = acol + c * L::kAcc * 256;
    if constexpr (L::kPairs) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if ((p.pairs >> (3 * c + k)) & 1u) {
          const int ta = k == 2 ? 8 : 4, tb = k == 0 ? 8 : 10;
          const float pk = 0.5f * a[(11 + k) * 256];
          a[ta * 256] -= pk;
          a[tb * 256] -= pk;
          float* __restrict__ cp = p.cot[3 * C + 3 * c + k];  // rows 0 and 1 of a P block are never read: zeros
          cp[n] = 0.0f;
          cp[N + n] = 0.0f;
          cp[2 * N + n] = pk;
        }
      }
    }
    float* __restrict__ c0 = p.cot[3 * c];
#pragma unroll
    for (int s = 0; s < 7; ++s) {
      const int row = sys_row0(s, p.nt[c], p.nx0[c]);
      if (row >= 0) c0[(long long)row * N + n] = a[s * 256];
    }
    if (p.nx1[c] >= 1) {  // row 0 of a further block is zero: the whole cotangent of the value went to block (c, 0)
      float* __restrict__ c1 = p.cot[3 * c + 1];
      c1[n] = 0.0f;
      c1[N + n] = a[7 * 256];
      if (p.nx1[c] >= 2) c1[2 * N + n] = a[8 * 256];
    }
    if (p.nx2[c] >= 1) {
      float* __restrict__ c2 = p.cot[3 * c + 2];
      c2[n] = 0.0f;
      c2[N + n] = a[9 * 256];
      if (p.nx2[c] >= 2) c2[2 * N + n] = a[10 * 256];
    }
  }
}

// ---- one row of the partials: the block's 256 values summed by halving, in double ----
__device__ __forceinline__ void sys_block_reduce(double* red, double v, double* out) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = red[0];
  __syncthreads();
}

// C: the number of fields (sizes the LDS block);  REDUCE: loss and / or coefficient sums are wanted (per-block partials);
// COEF: coefficient sums are wanted.  partial[b * kRow + e] = sum l(r_e,n), partial[b * kRow + 4 + m] = sum rbar_e(m),n
// prod_f phi_{m,f} over block b's points.  NLP (INV, needs COEF): the sums H_kj are wanted too, partial[b * kRow + 36 + 3 k + j];
// sweep 2 then runs whether or not cotangent blocks are written.  `extra` is what the level has of fn_values, nl_params and
// param_values, in this order: nothing for PLAIN and MIXED, one pointer for FN, two for NL, three for INV.
// pointer I of a level's extra kernel arguments, null beyond them
template <int I, class... P>
__device__ __forceinline__ const float* sys_extra(P... p) {
  const float* all[] = {p..., nullptr};
  return I < (int)sizeof...(P) ? all[I] : nullptr;
}

template <int LEVEL, int C, bool REDUCE, bool COEF, bool NLP, class... X>
__global__ __launch_bounds__(256) void term_system_kernel(SysProg<LEVEL> p, const float* __restrict__ coef_in, const float* __restrict__ x,
                                                          const float* __restrict__ t, X* __restrict__... extra, long long N,
                                                          const float* __restrict__ rbar_in, float* __restrict__ residual_out,
                                                          double* __restrict__ partial) {
  using L = SysLevel<LEVEL, C>;
  static_assert(!NLP || (L::kEff && COEF), "the H sums belong to INV and need the coefficient sums");
  __shared__ float sval[L::kValRows * 256];
  __shared__ float sacc[L::kAccRows * 256];
  float* vcol = sval + threadIdx.x;
  float* acol = sacc + threadIdx.x;
  const float* coef = coef_in;
  static_assert(sizeof...(X) == (L::kFns ? 1 : 0) + (L::kNl ? 1 : 0) + (L::kEff ? 1 : 0), "the level's pointers, no more");
  const float* fn = sys_extra<0>(extra...);
  const float* nlp_in = sys_extra<1>(extra...);
  const float* nlp = nlp_in;
  if constexpr (L::kEff) {
    __shared__ float seff[kSyEff];
    sys_effective(p, coef_in, nlp_in, sys_extra<2>(extra...), seff);
    coef = seff;
    nlp = seff + PINN_SYSTEM_MAX_TERMS;
  }
  double loss_acc[PINN_SYSTEM_MAX_EQUATIONS];
#pragma unroll
  for (int e = 0; e < PINN_SYSTEM_MAX_EQUATIONS; ++e) loss_acc[e] = 0.0;
  double cg[COEF ? PINN_SYSTEM_MAX_TERMS : 1];
#pragma unroll
  for (int m = 0; m < (COEF ? PINN_SYSTEM_MAX_TERMS : 1); ++m) cg[m] = 0.0;
  double hg[NLP ? kSyNlp : 1];
#pragma unroll
  for (int i = 0; i < (NLP ? kSyNlp : 1); ++i) hg[i] = 0.0;
  const bool write_cot = p.cot[0] != nullptr;
  const bool want_cot = write_cot || NLP;  // sweep 2 and the slopes: for the cotangent blocks, or for wbar_k alone

  for (long long n = (long long)blockIdx.x * 256 + threadIdx.x; n < N; n += (long long)gridDim.x * 256) {
    sys_load_fields<L, C, L::field_unroll(COEF)>(p, vcol, N, n);
    const float cx = (p.uses_coord & USE_X) ? x[n * p.dim] : 0.0f;
    const float cy = (p.uses_coord & USE_Y) ? x[n * p.dim + 1] : 0.0f;
    const float cz = (p.uses_coord & USE_Z) ? x[n * p.dim + 2] : 0.0f;
    const float ct = (p.uses_coord & USE_T) ? t[n] : 0.0f;
    if constexpr (L::load_fence(COEF)) asm volatile("" ::: "memory");  // see SysLevel
    if constexpr (L::kFns) sys_load_functions<L>(p, vcol, fn, N, n);
    if constexpr (L::kNl) sys_eval_nonlinear<L, NLP>(p, vcol, nlp, want_cot);
    const SysEq r = sys_sweep1<L>(p, vcol, cx, cy, cz, ct, coef);
    const SysEq rbar = sys_loss_rbar<REDUCE>(p, r, rbar_in, residual_out, N, n, loss_acc);
    if (want_cot) {
      sys_sweep2<L>(p, vcol, acol, cx, cy, cz, ct, coef, rbar);
      if constexpr (L::kNl) sys_push_nonlinear<L, NLP>(p, vcol, acol, nlp, hg);
    }
    if constexpr (COEF) sys_coef_sums<L>(p, vcol, cx, cy, cz, ct, rbar, cg);
    if (write_cot) sys_write_cotangents<L, C, L::field_unroll(COEF)>(p, acol, N, n);
  }

  if (REDUCE) {
    __shared__ double red[256];
    const int rows = NLP ? L::kRow : (COEF ? kSyH : kSyG);  // the rows a launch does not form are not read by its finish launch
#pragma unroll
    for (int k = 0; k < L::kRow; ++k)
      if (k < rows)
        sys_block_reduce(red, k < kSyG ? loss_acc[k < kSyG ? k : 0] : (k < kSyH ? cg[COEF ? k - kSyG : 0] : hg[NLP ? k - kSyH : 0]),
                         partial + blockIdx.x * L::kRow + k);
  }
}

// row k of the block partials summed in block order, in double
__device__ __forceinline__ double sys_row_sum(const double* partial, int blocks, int row_width, int k) {
  double s = 0.0;
#pragma unroll 8
  for (int b = 0; b < blocks; ++b) s += partial[b * row_width + k];
  return s;
}

// PLAIN .. NL.  Thread k: sum k of the block partials.  k < 4: the loss sum of equation k, added to eq_loss_sums[k]; thread 0
// also adds sum_e w_e S_e (ascending e, in double) to loss_sum_out.  k >= 4: coefficient sum k - 4.  A template only so that
// the INV unit, which has a finish kernel of its own (the parameter map), does not compile it.
template <int ROW>
__global__ void term_system_finish_kernel(const double* partial, int blocks, int n_eq, int n_terms, double w0, double w1, double w2,
                                          double w3, float* loss_sum_out, float* eq_loss_sums, float* coef_grads) {
  const int k = threadIdx.x;
  if (k == 0 && loss_sum_out) {
    const double w[PINN_SYSTEM_MAX_EQUATIONS] = {w0, w1, w2, w3};
    double total = 0.0;
    for (int e = 0; e < n_eq; ++e) total += w[e] * sys_row_sum(partial, blocks, ROW, e);
    loss_sum_out[0] = (float)((double)loss_sum_out[0] + total);
  }
  float* out = nullptr;
  if (k < kSyG) {
    if (k < n_eq && eq_loss_sums) out = eq_loss_sums + k;
  } else if (k - kSyG < n_terms && coef_grads) {
    out = coef_grads + (k - kSyG);
  }
  if (!out) return;
  out[0] = (float)((double)out[0] + sys_row_sum(partial, blocks, ROW, k));
}

int sys_launched(const char* who, const char* what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return PINN_OK;
  char msg[256];
  snprintf(msg, sizeof(msg), "HIP error %d: %s (%s: %s)", (int)e, hipGetErrorString(e), who, what);
  return pinn_internal_fail(PINN_ERR_HIP, msg);
}

}  // namespace
