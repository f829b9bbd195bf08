// Coupled PDE systems with learnable parameters (include/pinn_jet.h, "term residuals of coupled systems with learnable
// parameters"): the element-wise middle of
//   one pinn_jet_forward per (field, axis with streams) and per (field, pair of order 2: a component launch along e_a + e_b)
//   -> pinn_term_residual_system_inv -> one pinn_jet_backward per block.
// The kernel is term_system_nl_kernels.hip's, kept in a translation unit of its own so that that kernel's code does not move.
// What differs: a coefficient c_m and each entry of a nonlinear triple {shift, scale, exponent} is either the stored value or
// the stored value times one of up to eight parameters (one rounding), formed once per block into LDS from the device arrays,
// so a captured graph follows the optimiser.  Every point then runs the sibling's arithmetic on those effective values.  The
// gradient of the parameters is a combination of sums over the points: the sibling's coefficient sums G_m, and, behind the
// template flag NLP, the twelve sums H_kj of the nonlinear entries.  H needs the complete cotangent wbar_k of w_k, which the
// descending push loop holds at the moment it pushes function k; with NLP row 16 C + 8 + k holds the slope g'(arg) without the
// scale, and d_k = slope * scale is formed at the push (the same single rounding).  The finish launch adds the per-block
// partials in block order and combines them in double.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/pinn_jet.h"

namespace {

constexpr int kSiBlocks = 64;                                             // fixed grid: the partials are summed in block order
constexpr int kSiNlp = 3 * PINN_SYSTEM_MAX_NONLINEAR;                     // the sums H_kj, k * 3 + j
constexpr int kSiRow = PINN_SYSTEM_MAX_EQUATIONS + PINN_SYSTEM_MAX_TERMS + kSiNlp;  // doubles per block: {equation loss sums, G_m, H_kj}
constexpr int kSiEff = PINN_SYSTEM_MAX_TERMS + kSiNlp;                    // effective values in LDS: c_m, then the triples
constexpr int kSiVals = 16;  // value slots of a field: codes 0 .. 6, sin, cos, u_y, u_yy, u_z, u_zz, u_xy, u_xz, u_yz
constexpr int kSiAcc = 14;   // derivative accumulators of a field: codes 0 .. 6, u_y, u_yy, u_z, u_zz, then g of the three pairs
constexpr int kSiFns = PINN_SYSTEM_MAX_FUNCTIONS;  // function rows behind the C fields' value rows: slot 16 C + k is g_k
constexpr int kSiNl = PINN_SYSTEM_MAX_NONLINEAR;  // rows behind those: slot 16 C + 4 + k is w_k, row 16 C + 8 + k is d_k (no slot)
constexpr int kSiCoord = PINN_SYSTEM_MAX_FIELDS * kSiVals + kSiFns + kSiNl;  // slots 72 .. 75: x, y, z, t (registers, not LDS)

static_assert(PINN_SYSTEM_INV_SCRATCH_DOUBLES == kSiBlocks * kSiRow, "scratch constant and grid disagree");
static_assert(PINN_SYSTEM_MAX_FIELDS == 4 && PINN_SYSTEM_MAX_EQUATIONS == 4, "the kernel unrolls over four fields and four equations");
static_assert(PINN_SYSTEM_MAX_FUNCTIONS == 4 && PINN_TERM_FN3 - PINN_TERM_FN0 == 3, "the kernel holds four function values in registers");

static_assert(PINN_SYSTEM_MAX_NONLINEAR == 4 && PINN_TERM_NL == 31, "four nonlinear functions, named by code 31");
static_assert(PINN_SYSTEM_MAX_PARAMS == 8 && PINN_SYSTEM_MAX_TERMS + kSiNlp + PINN_SYSTEM_MAX_PARAMS <= 64, "one finish thread per sum");

enum { USE_X = 1, USE_Y = 2, USE_Z = 4, USE_T = 8 };

// the descriptor as the kernel reads it: one byte per factor = its slot (field * 16 + value slot, 16 C + k the known function
// g_k, 16 C + 4 + k the nonlinear function w_k, 72 .. 75 a coordinate, 255 unused)
struct SysInvProg {
  int n_terms, n_eq, dim, loss;
  float huber_delta;
  int uses_coord;
  int uses_fn;                                // bit k: a term names g_k (a row no term names is never read)
  int uses_nl;                                // bit k: w_k is evaluated (named by a term, or the source of such a function)
  unsigned nl_op, nl_src, nl_acc;             // byte k: PINN_NL_* of w_k, the slot of its source, the accumulator of its source
  int nt[PINN_SYSTEM_MAX_FIELDS], nx0[PINN_SYSTEM_MAX_FIELDS], nx1[PINN_SYSTEM_MAX_FIELDS], nx2[PINN_SYSTEM_MAX_FIELDS];
  int uses_trig[PINN_SYSTEM_MAX_FIELDS];
  float gw[PINN_SYSTEM_MAX_EQUATIONS];        // grad_scale * eq_weight[e], rounded once on the host
  double w[PINN_SYSTEM_MAX_EQUATIONS];        // eq_weight[e]
  unsigned slots[PINN_SYSTEM_MAX_TERMS];      // byte f = slot of factor f
  unsigned char n_factors[PINN_SYSTEM_MAX_TERMS];
  unsigned char eq[PINN_SYSTEM_MAX_TERMS];
  unsigned pairs;                             // bit 3 c + k: field c has pair k of (x,y), (x,z), (y,z) (pair_order 2)
  const float* jets[6 * PINN_SYSTEM_MAX_FIELDS];  // 3 c + a: axis block (c, a);  3 C + 3 c + k: the P block of (c, pair k)
  float* cot[6 * PINN_SYSTEM_MAX_FIELDS];     // all null when no cotangents are wanted
  int n_params;
  signed char coef_param[PINN_SYSTEM_MAX_TERMS];  // -1, or the parameter c_m is a multiple of (checked on the host)
  signed char nl_param[kSiNlp];               // the same for entry j of the triple of function k, at 3 k + j
};

// what the finish launch reads of it
struct SysInvMap {
  int n_params, uses_nl;
  signed char coef_param[PINN_SYSTEM_MAX_TERMS];
  signed char nl_param[kSiNlp];
};

// l(r) and l'(r) of PDEBase._apply_loss_fn per sample (term_kernels.hip::term_loss)
__device__ __forceinline__ float sxi_loss(int kind, float d, float r, float* dl) {
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
__host__ __device__ inline int sxi_row0(int code, int nt, int nx) {
  if (code == 0) return 0;
  if (code <= 2) return code <= nt ? code : -1;
  return code - 2 <= nx ? nt + code - 2 : -1;
}

// value slot (0 .. 15) of a stream / trig / mixed code, or -1 for a coordinate or an unknown code
__host__ inline int sxi_value_slot(int code) {
  if (code >= 0 && code <= 6) return code;
  if (code == PINN_TERM_SIN_U) return 7;
  if (code == PINN_TERM_COS_U) return 8;
  if (code >= PINN_TERM_UY && code <= PINN_TERM_UZZ) return 9 + (code - PINN_TERM_UY);
  if (code >= PINN_TERM_UXY && code <= PINN_TERM_UYZ) return 13 + (code - PINN_TERM_UXY);
  return -1;
}

// accumulator (field * 14 + k) the derivative of a value slot goes to: u, sin(u) and cos(u) all go to the value stream
__host__ __device__ inline int sxi_target(unsigned slot) {
  const int c = (int)slot / kSiVals, v = (int)slot - c * kSiVals;
  return c * kSiAcc + (v < 7 ? v : (v < 9 ? 0 : v - 2));
}

// the value of a slot: a wave-uniform row of this thread's LDS column (a field's value or a known function), or a coordinate
// register
__device__ __forceinline__ float sxi_value(const float* col, unsigned slot, float cx, float cy, float cz, float ct) {
  if (slot < (unsigned)kSiCoord) return col[slot * 256];
  switch (slot - kSiCoord) {
    case 0: return cx;
    case 1: return cy;
    case 2: return cz;
    default: return ct;
  }
}

// C: the number of fields (sizes the LDS block);  REDUCE: loss and / or coefficient sums are wanted (per-block partials);
// COEF: coefficient sums are wanted.  partial[b * kSiRow + e] = sum l(r_e,n), partial[b * kSiRow + 4 + m] = sum rbar_e(m),n
// prod_f phi_{m,f} over block b's points.  NLP: the sums H_kj of the learnable nonlinear entries are wanted too (needs COEF):
// partial[b * kSiRow + 36 + 3 k + j]; sweep 2 then runs whether or not cotangent blocks are written.
template <int C, bool REDUCE, bool COEF, bool NLP>
__global__ __launch_bounds__(256) void term_system_inv_kernel(SysInvProg p, const float* __restrict__ coef_in, const float* __restrict__ x,
                                                          const float* __restrict__ t, const float* __restrict__ fn, const float* __restrict__ nlp_in,
                                                          const float* __restrict__ pv, long long N, const float* __restrict__ rbar_in,
                                                          float* __restrict__ residual_out, double* __restrict__ partial) {
  __shared__ float sval[(C * kSiVals + kSiFns + 2 * kSiNl) * 256];
  __shared__ float sacc[(C * kSiAcc + kSiNl) * 256];
  __shared__ float seff[kSiEff];
  float* vcol = sval + threadIdx.x;
  float* acol = sacc + threadIdx.x;
  // the effective values, once per block: thread m < 32 the coefficient of term m, thread 32 + 3 k + j entry j of the triple of
  // function k (only inside the mask: the parameters of a function that is not evaluated are never read).  The index was
  // checked against n_params on the host.
  if (threadIdx.x < kSiEff) {
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
  const float* coef = seff;
  const float* nlp = seff + PINN_SYSTEM_MAX_TERMS;
  double loss_acc[PINN_SYSTEM_MAX_EQUATIONS];
#pragma unroll
  for (int e = 0; e < PINN_SYSTEM_MAX_EQUATIONS; ++e) loss_acc[e] = 0.0;
  double cg[COEF ? PINN_SYSTEM_MAX_TERMS : 1];
#pragma unroll
  for (int m = 0; m < (COEF ? PINN_SYSTEM_MAX_TERMS : 1); ++m) cg[m] = 0.0;
  double hg[NLP ? kSiNlp : 1];
#pragma unroll
  for (int i = 0; i < (NLP ? kSiNlp : 1); ++i) hg[i] = 0.0;
  const bool write_cot = p.cot[0] != nullptr;
  const bool want_cot = write_cot || NLP;  // sweep 2 and the slopes: for the cotangent blocks, or for wbar_k alone

  for (long long n = (long long)blockIdx.x * 256 + threadIdx.x; n < N; n += (long long)gridDim.x * 256) {
    // ---- the values of every field ----
    // the fields one after the other (not unrolled): only one field's block pointers are held in scalar registers at a time
#pragma unroll 1
    for (int c = 0; c < C; ++c) {
      const float* __restrict__ j0 = p.jets[3 * c];
      float* v = vcol + c * kSiVals * 256;
#pragma unroll
      for (int s = 0; s < 7; ++s) {
        const int row = sxi_row0(s, p.nt[c], p.nx0[c]);
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
      // the derived factors, in the evaluation order the header states: u_ab = 0.5f * ((P_2 - A_2) - B_2)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float* __restrict__ pk = p.jets[3 * C + 3 * c + k];
        const int sa = k == 2 ? 10 : 4, sb = k == 0 ? 10 : 12;  // value slots of the order-2 rows of the pair's two axes
        v[(13 + k) * 256] = ((p.pairs >> (3 * c + k)) & 1u) ? 0.5f * ((pk[2 * N + n] - v[sa * 256]) - v[sb * 256]) : 0.0f;
      }
    }
    const float cx = (p.uses_coord & USE_X) ? x[n * p.dim] : 0.0f;
    const float cy = (p.uses_coord & USE_Y) ? x[n * p.dim + 1] : 0.0f;
    const float cz = (p.uses_coord & USE_Z) ? x[n * p.dim + 2] : 0.0f;
    const float ct = (p.uses_coord & USE_T) ? t[n] : 0.0f;
    // function k at fn + k N; the mask is the host's, so a row that no term names is not touched (its LDS row is never read).
    // Not unrolled, like the field loop above: unrolled, the C = 3 and C = 4 forms with coefficient sums reserved scratch memory.
#pragma unroll 1
    for (int k = 0; k < kSiFns; ++k)
      if ((p.uses_fn >> k) & 1) vcol[(C * kSiVals + k) * 256] = fn[(long long)k * N + n];
    // the nonlinear functions in ascending k (a source may be an earlier one); outside the mask neither evaluated nor are its
    // parameters read.  The operation is wave-uniform.
    if (p.uses_nl) {
#pragma unroll 1
      for (int k = 0; k < kSiNl; ++k) {
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
        vcol[(C * kSiVals + kSiFns + k) * 256] = w;
        if (want_cot) vcol[(C * kSiVals + kSiFns + kSiNl + k) * 256] = NLP ? slope : __fmul_rn(slope, scale);
      }
    }

    // ---- sweep 1: r_e = sum_{m: equation_of[m] = e} c_m prod_f phi_{m,f}, terms in ascending m ----
    float r[PINN_SYSTEM_MAX_EQUATIONS];
#pragma unroll
    for (int e = 0; e < PINN_SYSTEM_MAX_EQUATIONS; ++e) r[e] = 0.0f;
    for (int m = 0; m < p.n_terms; ++m) {
      const unsigned slots = p.slots[m];
      const int nf = p.n_factors[m];
      const int eq = p.eq[m];
      float prod = coef[m];
#pragma unroll
      for (int f = 0; f < PINN_TERM_MAX_FACTORS; ++f)
        if (f < nf) prod *= sxi_value(vcol, (slots >> (8 * f)) & 255u, cx, cy, cz, ct);
#pragma unroll
      for (int e = 0; e < PINN_SYSTEM_MAX_EQUATIONS; ++e)
        if (e == eq) r[e] += prod;
    }

    // ---- the loss and rbar_e of every equation ----
    float rbar[PINN_SYSTEM_MAX_EQUATIONS];
#pragma unroll
    for (int e = 0; e < PINN_SYSTEM_MAX_EQUATIONS; ++e) {
      rbar[e] = 0.0f;
      if (e < p.n_eq) {
        float dl;
        const float lv = sxi_loss(p.loss, p.huber_delta, r[e], &dl);
        rbar[e] = rbar_in ? rbar_in[(long long)e * N + n] : p.gw[e] * dl;
        if (residual_out) residual_out[(long long)e * N + n] = r[e];
        if (REDUCE) loss_acc[e] += (double)lv;
      }
    }

    // ---- sweep 2: terms in ascending m again.  The derivative summands of ONE term that go to the same (field, stream)
    // accumulator (at most four) are summed first, in ascending factor order, multiplied by rbar of the term's equation and
    // then added to the accumulator ----
    if (want_cot) {
#pragma unroll
      for (int k = 0; k < C * kSiAcc + kSiNl; ++k) acol[k * 256] = 0.0f;
      for (int m = 0; m < p.n_terms; ++m) {
        const float c = coef[m];
        const unsigned slots = p.slots[m];
        const int nf = p.n_factors[m];
        const int eq = p.eq[m];
        float rb = rbar[0];
#pragma unroll
        for (int e = 1; e < PINN_SYSTEM_MAX_EQUATIONS; ++e)
          if (e == eq) rb = rbar[e];
        float phi[PINN_TERM_MAX_FACTORS];
#pragma unroll
        for (int f = 0; f < PINN_TERM_MAX_FACTORS; ++f)
          phi[f] = f < nf ? sxi_value(vcol, (slots >> (8 * f)) & 255u, cx, cy, cz, ct) : 1.0f;
        {
          // contribution of factor f to its target: c * prod_{g != f} phi_g, times cos(u) / -sin(u) under sin(u) / cos(u)
          float contrib[PINN_TERM_MAX_FACTORS];
          int target[PINN_TERM_MAX_FACTORS];
#pragma unroll
          for (int f = 0; f < PINN_TERM_MAX_FACTORS; ++f) {
            contrib[f] = 0.0f;
            target[f] = -1;
            const unsigned slot = (slots >> (8 * f)) & 255u;
            const bool is_nl = slot >= (unsigned)(C * kSiVals + kSiFns) && slot < (unsigned)(C * kSiVals + kSiFns + kSiNl);
            if (f < nf && (slot < (unsigned)(C * kSiVals) || is_nl)) {  // coordinates and known functions carry no cotangent
              float others = c;
#pragma unroll
              for (int g = 0; g < PINN_TERM_MAX_FACTORS; ++g)
                if (g != f && g < nf) others *= phi[g];
              if (is_nl) {  // w_k: a target of its own, accumulator 14 C + k
                contrib[f] = others;
                target[f] = C * kSiAcc + ((int)slot - (C * kSiVals + kSiFns));
              } else {
                const int fc = (int)slot / kSiVals, fv = (int)slot - fc * kSiVals;
                if (fv == 7) others = others * vcol[(fc * kSiVals + 8) * 256];
                else if (fv == 8) others = -(others * vcol[(fc * kSiVals + 7) * 256]);
                contrib[f] = others;
                target[f] = sxi_target(slot);
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
      // the cotangents of the nonlinear functions go to their sources, in descending k: wbar_k * d_k, rounded, then added
      if (NLP) {
        // the same pushes, unrolled so that hg[] stays in registers.  When function k is pushed its accumulator is complete
        // (the later functions have pushed already): wbar_k.  Row 16 C + 8 + k holds the slope without the scale here.
        //   H_k0 += wbar slope,  H_k1 += (wbar slope) s,  H_k2 += (wbar w) logf(arg)  (POW only), each product rounded
#pragma unroll
        for (int k = kSiNl - 1; k >= 0; --k) {
          if ((p.uses_nl >> k) & 1) {
            const float wbar = acol[(C * kSiAcc + k) * 256];
            const float slope = vcol[(C * kSiVals + kSiFns + kSiNl + k) * 256];
            const float scale = nlp[3 * k + 1];
            const float push = __fmul_rn(wbar, __fmul_rn(slope, scale));
            acol[((p.nl_acc >> (8 * k)) & 255u) * 256] += push;
            const float s = vcol[((p.nl_src >> (8 * k)) & 255u) * 256];
            const float h0 = __fmul_rn(wbar, slope);
            if (p.nl_param[3 * k] >= 0) hg[NLP ? 3 * k : 0] += (double)h0;
            if (p.nl_param[3 * k + 1] >= 0) hg[NLP ? 3 * k + 1 : 0] += (double)__fmul_rn(h0, s);
            if (p.nl_param[3 * k + 2] >= 0) {  // POW, checked on the host
              const float arg = fmaf(scale, s, nlp[3 * k]);
              hg[NLP ? 3 * k + 2 : 0] += (double)__fmul_rn(__fmul_rn(wbar, vcol[(C * kSiVals + kSiFns + k) * 256]), logf(arg));
            }
          }
        }
      } else if (p.uses_nl) {
#pragma unroll 1
        for (int k = kSiNl - 1; k >= 0; --k) {
          if (!((p.uses_nl >> k) & 1)) continue;
          const float push = __fmul_rn(acol[(C * kSiAcc + k) * 256], vcol[(C * kSiVals + kSiFns + kSiNl + k) * 256]);
          acol[((p.nl_acc >> (8 * k)) & 255u) * 256] += push;
        }
      }
    }

    // ---- the coefficient sums: rbar_e(m) prod_f phi_{m,f}, the product from 1.0f in ascending f ----
    if (COEF) {
      // The loop is unrolled so that cg[] stays in registers.  The term index goes through an opaque scalar once per round:
      // otherwise the descriptor loads of all 32 terms are hoisted out of the grid-stride loop and held in scalar registers
      // across it, which, with the function rows, no longer fit (they spilled into scratch memory).
      int mb = 0;
      asm volatile("" : "+s"(mb));
#pragma unroll
      for (int m = 0; m < PINN_SYSTEM_MAX_TERMS; ++m) {
        if (m < p.n_terms) {
          const unsigned slots = p.slots[mb + m];
          const int nf = p.n_factors[mb + m];
          const int eq = p.eq[mb + m];
          float rb = rbar[0];
#pragma unroll
          for (int e = 1; e < PINN_SYSTEM_MAX_EQUATIONS; ++e)
            if (e == eq) rb = rbar[e];
          float prod = 1.0f;
#pragma unroll
          for (int f = 0; f < PINN_TERM_MAX_FACTORS; ++f)
            if (f < nf) prod *= sxi_value(vcol, (slots >> (8 * f)) & 255u, cx, cy, cz, ct);
          cg[m] += (double)(rb * prod);
        }
      }
    }

    // ---- the cotangent blocks: every row of every block is written.  The transposed polarisation first, per field and in
    // ascending pair index: p_k = g_k / 2 to row 2 of the P block, and subtracted from the order-2 accumulators of the pair's
    // two axes (accumulators 4, 8, 10: u_xx, u_yy, u_zz) ----
    if (write_cot) {
#pragma unroll 1
      for (int c = 0; c < C; ++c) {
        float* a = acol + c * kSiAcc * 256;
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
        float* __restrict__ c0 = p.cot[3 * c];
#pragma unroll
        for (int s = 0; s < 7; ++s) {
          const int row = sxi_row0(s, p.nt[c], p.nx0[c]);
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
  }

  if (REDUCE) {
    __shared__ double red[256];
    constexpr int kG = PINN_SYSTEM_MAX_EQUATIONS, kH = PINN_SYSTEM_MAX_EQUATIONS + PINN_SYSTEM_MAX_TERMS;
    const int rows = NLP ? kSiRow : (COEF ? kH : kG);  // the rows a launch does not form are not read by its finish launch
#pragma unroll
    for (int k = 0; k < kSiRow; ++k) {
      if (k < rows) {
        red[threadIdx.x] = k < kG ? loss_acc[k < kG ? k : 0] : (k < kH ? cg[COEF ? k - kG : 0] : hg[NLP ? k - kH : 0]);
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
          if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
          __syncthreads();
        }
        if (threadIdx.x == 0) partial[blockIdx.x * kSiRow + k] = red[0];
        __syncthreads();
      }
    }
  }
}

// Thread k < 48: row k of the block partials summed in block order, in double, into LDS (rows the launch did not form count as
// 0: `with_g`, `with_h`).  Then thread k < 4: the loss sum of equation k, added to eq_loss_sums[k]; thread 0 also adds
// sum_e w_e S_e (ascending e, in double) to loss_sum_out.  4 <= k < 36: coefficient sum k - 4.  Thread 48 + q: parameter q,
//   param_grads[q] += sum_{m: coef_param[m] = q} coef_values[m] G_m + sum_{(k, j): nl_param[k][j] = q} nl_params[3 k + j] H_kj,
// the combination in double over m, then (k, j), ascending; one rounding at the add.  Every sum is taken once, by one thread:
// a parameter that many terms name costs no more than one row.
__global__ void term_system_inv_finish_kernel(const double* partial, int blocks, int n_eq, int n_terms, double w0, double w1, double w2,
                                          double w3, float* loss_sum_out, float* eq_loss_sums, float* coef_grads, SysInvMap map,
                                          const float* coef_values, const float* nl_params, int with_g, int with_h, float* param_grads) {
  constexpr int kG = PINN_SYSTEM_MAX_EQUATIONS, kH = PINN_SYSTEM_MAX_EQUATIONS + PINN_SYSTEM_MAX_TERMS;
  __shared__ double rowsum[kSiRow];
  const int k = threadIdx.x;
  if (k < kSiRow) {
    const bool formed = k < kG ? k < n_eq : (k < kH ? (with_g && k - kG < n_terms) : (with_h != 0));
    double s = 0.0;
    if (formed) {
#pragma unroll 8
      for (int b = 0; b < blocks; ++b) s += partial[b * kSiRow + k];
    }
    rowsum[k] = s;
  }
  __syncthreads();
  if (k >= 48) {
    const int q = k - 48;
    if (!param_grads || q >= map.n_params) return;
    double acc = 0.0;
    for (int m = 0; m < n_terms; ++m)
      if (map.coef_param[m] == q) acc += (double)coef_values[m] * rowsum[kG + m];
    if (with_h) {
      for (int kj = 0; kj < kSiNlp; ++kj)
        if (map.nl_param[kj] == q && ((map.uses_nl >> (kj / 3)) & 1)) acc += (double)nl_params[kj] * rowsum[kH + kj];
    }
    param_grads[q] = (float)((double)param_grads[q] + acc);
    return;
  }
  if (k >= kH) return;
  if (k == 0 && loss_sum_out) {
    const double w[PINN_SYSTEM_MAX_EQUATIONS] = {w0, w1, w2, w3};
    double total = 0.0;
    for (int e = 0; e < n_eq; ++e) total += w[e] * rowsum[e];
    loss_sum_out[0] = (float)((double)loss_sum_out[0] + total);
  }
  float* out = nullptr;
  if (k < kG) {
    if (k < n_eq && eq_loss_sums) out = eq_loss_sums + k;
  } else if (k - kG < n_terms && coef_grads) {
    out = coef_grads + (k - kG);
  }
  if (!out) return;
  out[0] = (float)((double)out[0] + rowsum[k]);
}

// the stream sets the library has axis-0 units for (csrc/Makefile: SETS)
bool sxi_set_compiled(int nt, int nx) {
  static const int sets[][2] = {{0, 0}, {1, 0}, {1, 1}, {1, 2}, {1, 3}, {1, 4}, {2, 0}, {2, 2}};
  for (const auto& s : sets)
    if (s[0] == nt && s[1] == nx) return true;
  return false;
}

constexpr int kPairA[3] = {0, 0, 1}, kPairB[3] = {1, 2, 2};  // the axes of pair k

template <int C>
void sxi_launch(bool reduce, bool coef_sums, bool nl_sums, int blocks, hipStream_t st, const SysInvProg& p, const float* coef, const float* x,
                const float* t, const float* fn, const float* nlp, const float* pv, long long N, const float* rbar_in, float* residual_out,
                double* partial) {
  if (!reduce)
    hipLaunchKernelGGL((term_system_inv_kernel<C, false, false, false>), dim3(blocks), dim3(256), 0, st, p, coef, x, t, fn, nlp, pv, N, rbar_in, residual_out, partial);
  else if (nl_sums)
    hipLaunchKernelGGL((term_system_inv_kernel<C, true, true, true>), dim3(blocks), dim3(256), 0, st, p, coef, x, t, fn, nlp, pv, N, rbar_in, residual_out, partial);
  else if (coef_sums)
    hipLaunchKernelGGL((term_system_inv_kernel<C, true, true, false>), dim3(blocks), dim3(256), 0, st, p, coef, x, t, fn, nlp, pv, N, rbar_in, residual_out, partial);
  else
    hipLaunchKernelGGL((term_system_inv_kernel<C, true, false, false>), dim3(blocks), dim3(256), 0, st, p, coef, x, t, fn, nlp, pv, N, rbar_in, residual_out, partial);
}

}  // namespace

extern "C" int pinn_internal_fail(int code, const char* msg);  // pinn_abi.hip: sets pinn_last_error()

static int sxi_launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return PINN_OK;
  char msg[256];
  snprintf(msg, sizeof(msg), "HIP error %d: %s (%s)", (int)e, hipGetErrorString(e), what);
  return pinn_internal_fail(PINN_ERR_HIP, msg);
}

extern "C" int pinn_term_residual_system_inv(const PinnTermPdeSystemInv* pde, const float* coef_values, const float* const* jets,
                                         const float* x, const float* t, const float* fn_values, const float* nl_params,
                                         const float* param_values, int64_t N, float grad_scale, const float* residual_cotangent,
                                         float* residual_out, float* loss_sum_out, float* eq_loss_sums, float* const* jet_cotangents,
                                         float* coef_grads, float* param_grads, double* scratch, void* stream) {
  char msg[256];
#define SXI_BAD(...)                                  \
  do {                                                \
    snprintf(msg, sizeof(msg), __VA_ARGS__);          \
    return pinn_internal_fail(PINN_ERR_BAD_DESC, msg); \
  } while (0)
  if (!pde) SXI_BAD("pinn_term_residual_system_inv: null descriptor");
  const int dim = pde->dimension, C = pde->n_fields, E = pde->n_equations;
  if (dim < 1 || dim > 3) SXI_BAD("pinn_term_residual_system_inv: dimension %d outside [1, 3]", dim);
  if (C < 1 || C > PINN_SYSTEM_MAX_FIELDS) SXI_BAD("pinn_term_residual_system_inv: n_fields %d outside [1, %d]", C, PINN_SYSTEM_MAX_FIELDS);
  if (E < 1 || E > PINN_SYSTEM_MAX_EQUATIONS)
    SXI_BAD("pinn_term_residual_system_inv: n_equations %d outside [1, %d]", E, PINN_SYSTEM_MAX_EQUATIONS);
  if (pde->n_terms < 0 || pde->n_terms > PINN_SYSTEM_MAX_TERMS)
    SXI_BAD("pinn_term_residual_system_inv: n_terms %d outside [0, %d]", (int)pde->n_terms, PINN_SYSTEM_MAX_TERMS);
  const int K = pde->n_functions;
  if (K < 0 || K > PINN_SYSTEM_MAX_FUNCTIONS)
    SXI_BAD("pinn_term_residual_system_inv: n_functions %d outside [0, %d]", K, PINN_SYSTEM_MAX_FUNCTIONS);
  const int KN = pde->n_nonlinear;
  if (KN < 0 || KN > PINN_SYSTEM_MAX_NONLINEAR)
    SXI_BAD("pinn_term_residual_system_inv: n_nonlinear %d outside [0, %d]", KN, PINN_SYSTEM_MAX_NONLINEAR);
  // the parameter maps: no index reaches the device unchecked (entries beyond n_terms / n_nonlinear are not read)
  const int P = pde->n_params;
  if (P < 0 || P > PINN_SYSTEM_MAX_PARAMS)
    SXI_BAD("pinn_term_residual_system_inv: n_params %d outside [0, %d]", P, PINN_SYSTEM_MAX_PARAMS);
  bool any_param = false;
  for (int m = 0; m < pde->n_terms; ++m) {
    const int q = pde->coef_param[m];
    if (q < -1 || q >= P) SXI_BAD("pinn_term_residual_system_inv: term %d: coef_param %d outside [-1, %d)", m, q, P);
    any_param = any_param || q >= 0;
  }
  for (int k = 0; k < KN; ++k) {
    static const char* const entry[3] = {"shift", "scale", "exponent"};
    for (int j = 0; j < 3; ++j) {
      const int q = pde->nl_param[k][j];
      if (q < -1 || q >= P)
        SXI_BAD("pinn_term_residual_system_inv: nonlinear function %d: nl_param of its %s, %d, outside [-1, %d)", k, entry[j], q, P);
      any_param = any_param || q >= 0;
    }
    if (pde->nl_param[k][2] >= 0 && pde->nl_op[k] != PINN_NL_POW)
      SXI_BAD("pinn_term_residual_system_inv: nonlinear function %d: a learnable exponent needs PINN_NL_POW (operation %d)", k,
              (int)pde->nl_op[k]);
  }
  SysInvProg p;
  memset(&p, 0, sizeof(p));
  p.n_params = P;
  for (int m = 0; m < PINN_SYSTEM_MAX_TERMS; ++m) p.coef_param[m] = (signed char)(m < pde->n_terms ? pde->coef_param[m] : -1);
  for (int k = 0; k < PINN_SYSTEM_MAX_NONLINEAR; ++k)
    for (int j = 0; j < 3; ++j) p.nl_param[3 * k + j] = (signed char)(k < KN ? pde->nl_param[k][j] : -1);
  p.n_terms = pde->n_terms;
  p.n_eq = E;
  p.dim = dim;
  p.loss = pde->loss;
  p.huber_delta = pde->huber_delta;
  for (int c = 0; c < C; ++c) {
    const int nt = pde->time_order[c], nx0 = pde->space_order[c][0];
    if (!sxi_set_compiled(nt, nx0))
      SXI_BAD("pinn_term_residual_system_inv: field %d: axis-0 stream set (nt=%d, nx=%d) is not compiled", c, nt, nx0);
    for (int a = 1; a < 3; ++a) {
      const int so = pde->space_order[c][a];
      if (so < 0 || so > (a < dim ? 2 : 0))
        SXI_BAD("pinn_term_residual_system_inv: field %d: space_order[%d] = %d outside [0, %d] (dimension %d)", c, a, so, a < dim ? 2 : 0, dim);
    }
    p.nt[c] = nt;
    p.nx0[c] = nx0;
    p.nx1[c] = pde->space_order[c][1];
    p.nx2[c] = pde->space_order[c][2];
    for (int k = 0; k < 3; ++k) {
      const int po = pde->pair_order[c][k];
      if (po != 0 && po != 2)
        SXI_BAD("pinn_term_residual_system_inv: field %d: pair_order[%d] = %d on the pair of axes (%d, %d) (0 or 2)", c, k, po, kPairA[k], kPairB[k]);
      if (po != 0 && dim < 2)
        SXI_BAD("pinn_term_residual_system_inv: field %d: pair_order[%d] = %d on the pair of axes (%d, %d) in dimension %d (a mixed derivative needs 2 or 3)",
                c, k, po, kPairA[k], kPairB[k], dim);
      if (po != 0 && kPairB[k] >= dim)
        SXI_BAD("pinn_term_residual_system_inv: field %d: pair_order[%d] = %d on the pair of axes (%d, %d), dimension %d", c, k, po, kPairA[k],
                kPairB[k], dim);
      if (po) p.pairs |= 1u << (3 * c + k);
    }
  }
  for (int e = 0; e < E; ++e) {
    const float w = pde->eq_weight[e];
    if (!std::isfinite(w) || w < 0.0f) SXI_BAD("pinn_term_residual_system_inv: eq_weight[%d] = %g is negative or not finite", e, (double)w);
    p.gw[e] = grad_scale * w;
    p.w[e] = (double)w;
  }
  // the slot of a factor that belongs to a field (a stream, sin / cos when `trig`, u_ab), checked against what the descriptor
  // holds; -1 with the message in msg.  `where` is "term m, factor f" or "nonlinear function k".
  auto field_slot = [&](const char* where, int code, int field, bool trig) -> int {
    const int vs = sxi_value_slot(code);
#define SXI_MSG(...) return (snprintf(msg, sizeof(msg), __VA_ARGS__), -1)
    if (code >= PINN_TERM_UYYY && code <= PINN_TERM_UZZZZ)
      SXI_MSG("pinn_term_residual_system_inv: %s: code %d (u_yyy, u_yyyy, u_zzz, u_zzzz): orders above 2 along y and z are "
              "not available in systems", where, code);
    if (code >= PINN_TERM_UXXYY && code <= PINN_TERM_UYYZZ)
      SXI_MSG("pinn_term_residual_system_inv: %s: code %d (u_xxyy, u_xxzz, u_yyzz): u_aabb is not available in systems", where, code);
    if (vs < 0) SXI_MSG("pinn_term_residual_system_inv: %s: unknown factor code %d", where, code);
    if (!trig && (vs == 7 || vs == 8))
      SXI_MSG("pinn_term_residual_system_inv: %s: the source (code %d) is neither a stream of a field nor an earlier nonlinear function", where, code);
    if (field >= C) SXI_MSG("pinn_term_residual_system_inv: %s names field %d of %d", where, field, C);
    bool held = true;
    if (code < 7) held = sxi_row0(code, p.nt[field], p.nx0[field]) >= 0;
    else if (code == PINN_TERM_UY || code == PINN_TERM_UYY) held = p.nx1[field] >= code - PINN_TERM_UY + 1;
    else if (code == PINN_TERM_UZ || code == PINN_TERM_UZZ) held = p.nx2[field] >= code - PINN_TERM_UZ + 1;
    if (vs >= 13) {
      const int k = vs - 13;
      const int order[3] = {p.nx0[field], p.nx1[field], p.nx2[field]};
      const int po = (p.pairs >> (3 * field + k)) & 1u ? 2 : 0;
      if (po != 2 || order[kPairA[k]] < 2 || order[kPairB[k]] < 2)
        SXI_MSG("pinn_term_residual_system_inv: %s names the mixed derivative (code %d) of field %d along the pair of axes "
                "(%d, %d), which needs pair_order[%d][%d] = 2 and order >= 2 on both axes (pair_order %d, orders %d, %d)", where, code, field,
                kPairA[k], kPairB[k], field, k, po, order[kPairA[k]], order[kPairB[k]]);
    }
    if (!held)
      SXI_MSG("pinn_term_residual_system_inv: %s names a stream (code %d) that field %d (nt=%d, space orders %d, %d, %d) does not hold",
              where, code, field, p.nt[field], p.nx0[field], p.nx1[field], p.nx2[field]);
#undef SXI_MSG
    if (vs == 7 || vs == 8) p.uses_trig[field] = 1;
    return field * kSiVals + vs;
  };
  // the nonlinear functions: operation and source of every declared one, named by a term or not
  for (int k = 0; k < KN; ++k) {
    const int op = pde->nl_op[k], byte = pde->nl_source[k];
    if (op < PINN_NL_EXP || op > PINN_NL_COS) SXI_BAD("pinn_term_residual_system_inv: nonlinear function %d: unknown operation %d", k, op);
    if (byte < 0 || byte > 255) SXI_BAD("pinn_term_residual_system_inv: nonlinear function %d: %d is not one byte (field * 32 + code)", k, byte);
    const int code = byte & 31, field = byte >> 5;
    int slot, acc;
    if (code == PINN_TERM_NL) {
      if (field >= k)
        SXI_BAD("pinn_term_residual_system_inv: nonlinear function %d: its source, nonlinear function %d, is not an earlier one", k, field);
      slot = C * kSiVals + kSiFns + field;
      acc = C * kSiAcc + field;
    } else if (code == PINN_TERM_X || code == PINN_TERM_Y || code == PINN_TERM_Z || code == PINN_TERM_T ||
               (code >= PINN_TERM_FN0 && code <= PINN_TERM_FN3)) {
      SXI_BAD("pinn_term_residual_system_inv: nonlinear function %d: the source (code %d) is neither a stream of a field nor an earlier "
              "nonlinear function", k, code);
    } else {
      char where[48];
      snprintf(where, sizeof(where), "nonlinear function %d", k);
      slot = field_slot(where, code, field, false);
      if (slot < 0) return pinn_internal_fail(PINN_ERR_BAD_DESC, msg);
      acc = sxi_target((unsigned)slot);
    }
    p.nl_op |= (unsigned)op << (8 * k);
    p.nl_src |= (unsigned)slot << (8 * k);
    p.nl_acc |= (unsigned)acc << (8 * k);
  }
  for (int m = 0; m < PINN_SYSTEM_MAX_TERMS; ++m) p.slots[m] = 0xffffffffu;
  for (int m = 0; m < pde->n_terms; ++m) {
    const PinnTermPdeTerm& tm = pde->terms[m];
    const int eq = pde->equation_of[m];
    if (eq < 0 || eq >= E) SXI_BAD("pinn_term_residual_system_inv: equation_of[%d] = %d outside [0, %d)", m, eq, E);
    if (tm.n_factors < 0 || tm.n_factors > PINN_TERM_MAX_FACTORS)
      SXI_BAD("pinn_term_residual_system_inv: term %d has n_factors %d outside [0, %d]", m, (int)tm.n_factors, PINN_TERM_MAX_FACTORS);
    unsigned packed = 0xffffffffu;
    for (int f = 0; f < tm.n_factors; ++f) {
      const int byte = tm.factor[f];
      if (byte < 0 || byte > 255) SXI_BAD("pinn_term_residual_system_inv: term %d, factor %d: %d is not one byte (field * 32 + code)", m, f, byte);
      const int code = byte & 31, field = byte >> 5;
      int slot;
      if (code == PINN_TERM_X || code == PINN_TERM_Y || code == PINN_TERM_Z || code == PINN_TERM_T) {  // the field bits are ignored
        if ((code == PINN_TERM_Y && dim < 2) || (code == PINN_TERM_Z && dim < 3))
          SXI_BAD("pinn_term_residual_system_inv: term %d, factor %d names a coordinate (code %d) that dimension %d does not hold", m, f, code, dim);
        p.uses_coord |= code == PINN_TERM_X ? USE_X : (code == PINN_TERM_Y ? USE_Y : (code == PINN_TERM_Z ? USE_Z : USE_T));
        slot = kSiCoord + (code == PINN_TERM_X ? 0 : (code == PINN_TERM_Y ? 1 : (code == PINN_TERM_Z ? 2 : 3)));
      } else if (code >= PINN_TERM_FN0 && code <= PINN_TERM_FN3) {  // the field bits are ignored here too
        const int k = code - PINN_TERM_FN0;
        if (k >= K)
          SXI_BAD("pinn_term_residual_system_inv: term %d, factor %d names function %d (code %d) of %d (n_functions)", m, f, k, code, K);
        p.uses_fn |= 1 << k;
        slot = C * kSiVals + k;
      } else if (code == PINN_TERM_NL) {  // the field bits carry k
        if (field >= KN)
          SXI_BAD("pinn_term_residual_system_inv: term %d, factor %d names nonlinear function %d (code %d) of %d (n_nonlinear)", m, f, field, code, KN);
        p.uses_nl |= 1 << field;
        slot = C * kSiVals + kSiFns + field;
      } else {
        char where[48];
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
  for (int k = KN - 1; k > 0; --k) {
    const unsigned src = (p.nl_src >> (8 * k)) & 255u;
    if (((p.uses_nl >> k) & 1) && src >= (unsigned)(C * kSiVals + kSiFns)) p.uses_nl |= 1 << (int)(src - (C * kSiVals + kSiFns));
  }
  if (N < 0) SXI_BAD("pinn_term_residual_system_inv: N < 0");
  if (N == 0) return PINN_OK;
  if (!jets || !coef_values) SXI_BAD("pinn_term_residual_system_inv: null jets table or coef_values");
  for (int c = 0; c < C; ++c) {
    const int so[3] = {1, p.nx1[c], p.nx2[c]};  // block (c, 0) always holds the value stream
    for (int a = 0; a < 3; ++a) {
      const bool need = a < dim && so[a] > 0;
      p.jets[3 * c + a] = need ? jets[3 * c + a] : nullptr;
      p.cot[3 * c + a] = (jet_cotangents && need) ? jet_cotangents[3 * c + a] : nullptr;
      if (need && (!p.jets[3 * c + a] || (jet_cotangents && !p.cot[3 * c + a])))
        SXI_BAD("pinn_term_residual_system_inv: null block (field %d, axis %d) of the jets or jet_cotangents table", c, a);
    }
    for (int k = 0; k < 3; ++k) {
      const int b = 3 * C + 3 * c + k;
      const bool need = (p.pairs >> (3 * c + k)) & 1u;
      p.jets[b] = need ? jets[b] : nullptr;
      p.cot[b] = (jet_cotangents && need) ? jet_cotangents[b] : nullptr;
      if (need && (!p.jets[b] || (jet_cotangents && !p.cot[b])))
        SXI_BAD("pinn_term_residual_system_inv: null block %d of the jets or jet_cotangents table (the P block of field %d, pair of axes (%d, %d))",
                b, c, kPairA[k], kPairB[k]);
    }
  }
  if (((p.uses_coord & (USE_X | USE_Y | USE_Z)) && !x) || ((p.uses_coord & USE_T) && !t))
    SXI_BAD("pinn_term_residual_system_inv: a term names X / Y / Z / T but the coordinate array is null");
  if (p.uses_fn && !fn_values) {
    int m = 0, k = 0;  // the first term that names a function, for the message
    for (; m < pde->n_terms; ++m) {
      bool found = false;
      for (int f = 0; f < p.n_factors[m] && !found; ++f) {
        const unsigned slot = (p.slots[m] >> (8 * f)) & 255u;
        if (slot >= (unsigned)(C * kSiVals) && slot < (unsigned)(C * kSiVals + kSiFns)) found = true, k = (int)slot - C * kSiVals;
      }
      if (found) break;
    }
    SXI_BAD("pinn_term_residual_system_inv: term %d names function %d but fn_values is null", m, k);
  }
  if (p.uses_nl && !nl_params) {
    int k = 0;
    while (!((p.uses_nl >> k) & 1)) ++k;
    SXI_BAD("pinn_term_residual_system_inv: nonlinear function %d is evaluated but nl_params is null", k);
  }
  if (any_param && !param_values) {
    for (int m = 0; m < pde->n_terms; ++m)
      if (pde->coef_param[m] >= 0) SXI_BAD("pinn_term_residual_system_inv: term %d has a learnable coefficient but param_values is null", m);
    int k = 0;
    while (pde->nl_param[k][0] < 0 && pde->nl_param[k][1] < 0 && pde->nl_param[k][2] < 0) ++k;
    SXI_BAD("pinn_term_residual_system_inv: nonlinear function %d has a learnable entry but param_values is null", k);
  }
  const bool reduce = loss_sum_out || eq_loss_sums || coef_grads || param_grads;
  if (param_grads && !scratch) SXI_BAD("pinn_term_residual_system_inv: param_grads without scratch");
  if (reduce && !scratch) SXI_BAD("pinn_term_residual_system_inv: null scratch with a loss or coefficient sum");
#undef SXI_BAD
  if (reinterpret_cast<uintptr_t>(scratch) & 7u)
    return pinn_internal_fail(PINN_ERR_MISALIGNED, "pinn_term_residual_system_inv: scratch must be 8-byte aligned");

  long long nb = ((long long)N + 255) / 256;
  const int blocks = (int)(nb > kSiBlocks ? kSiBlocks : nb);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool cs = coef_grads != nullptr || param_grads != nullptr;  // the parameter gradients are built on the G sums
  // the H sums only where a learnable nonlinear entry is inside the mask: every other launch keeps the sibling's registers
  bool hs = false;
  for (int kj = 0; kj < kSiNlp && param_grads; ++kj) hs = hs || (p.nl_param[kj] >= 0 && ((p.uses_nl >> (kj / 3)) & 1));
  const float* pv = param_values;
  switch (C) {
    case 1: sxi_launch<1>(reduce, cs, hs, blocks, st, p, coef_values, x, t, fn_values, nl_params, pv, (long long)N, residual_cotangent, residual_out, scratch); break;
    case 2: sxi_launch<2>(reduce, cs, hs, blocks, st, p, coef_values, x, t, fn_values, nl_params, pv, (long long)N, residual_cotangent, residual_out, scratch); break;
    case 3: sxi_launch<3>(reduce, cs, hs, blocks, st, p, coef_values, x, t, fn_values, nl_params, pv, (long long)N, residual_cotangent, residual_out, scratch); break;
    default: sxi_launch<4>(reduce, cs, hs, blocks, st, p, coef_values, x, t, fn_values, nl_params, pv, (long long)N, residual_cotangent, residual_out, scratch); break;
  }
  int rc = sxi_launched("term_system_inv_kernel");
  if (rc || !reduce) return rc;
  SysInvMap map;
  memset(&map, 0, sizeof(map));
  map.n_params = P;
  map.uses_nl = p.uses_nl;
  memcpy(map.coef_param, p.coef_param, sizeof(map.coef_param));
  memcpy(map.nl_param, p.nl_param, sizeof(map.nl_param));
  hipLaunchKernelGGL(term_system_inv_finish_kernel, dim3(1), dim3(64), 0, st, scratch, blocks, E, (int)p.n_terms, p.w[0], p.w[1], p.w[2], p.w[3],
                     loss_sum_out, eq_loss_sums, coef_grads, map, coef_values, nl_params, cs ? 1 : 0, hs ? 1 : 0, param_grads);
  return sxi_launched("term_system_inv_finish_kernel");
}
