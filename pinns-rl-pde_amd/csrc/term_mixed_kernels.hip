// Residuals given as data with mixed derivatives (include/pinn_jet.h, "term residuals with mixed derivatives"): the
// element-wise middle of the chain
//   pinn_jet_forward per axis block and per direction block (PINN_FLAG_SPACE_DIRECTION) -> pinn_term_residual_mixed ->
//   pinn_jet_backward per block.
// The scheme is term_axes_kernels.hip's: one thread per point, factor values in registers indexed by factor code through
// wave-uniform switches, the term list a kernel argument, the coefficients read from the device at launch time.  The derived
// factors u_ab, u_aabb are evaluated into the factor-value array first, dr/dfactor is accumulated per code by the per-term
// loop of the axes kernel, and the fixed linear maps (the transposes of the two polarisation formulas) are applied once per
// point.  An HBM-bound pass: only the rows the program names are loaded (`need`, a wave-uniform mask made on the host), and
// from a P / Q block only the rows 2 and 4.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../../include/pinn_jet.h"

namespace {

constexpr int kMxBlocks = 64;                    // fixed grid: the partials are summed in block order
constexpr int kMxRow = 1 + PINN_TERM_MAX_TERMS;  // doubles per block: {loss, coefficient sums}
constexpr int kMxCodes = 27;                     // factor codes 0 .. 26
// derivative accumulators (`slots`): codes 0 .. 6, then u_y .. u_yyyy (7 .. 10), u_z .. u_zzzz (11 .. 14),
// u_xy, u_xz, u_yz (15 .. 17), u_xxyy, u_xxzz, u_yyzz (18 .. 20)
constexpr int kMxSlots = 21;
constexpr float kTwelfth = (float)(1.0 / 12.0);

static_assert(PINN_TERM_SCRATCH_DOUBLES == kMxBlocks * kMxRow, "scratch constant and grid disagree");

enum { USE_X = 1, USE_Y = 2, USE_Z = 4, USE_T = 8 };

// the descriptor as the kernel reads it: factor codes packed one byte each, unused positions = 255
struct MixedProg {
  int n_terms, dim, nt, nx0, nx1, nx2, loss;
  int po[3];  // pair orders of (x,y), (x,z), (y,z)
  float huber_delta;
  int uses_trig, uses_coord;
  unsigned need;  // bit s: slot s is read (a mixed slot also sets the slots of the axis rows its formula reads)
  unsigned factors[PINN_TERM_MAX_TERMS];  // byte f = code of factor f
  int n_factors[PINN_TERM_MAX_TERMS];
  const float* jets[PINN_TERM_MIXED_BLOCKS];  // null where the descriptor has no such block
  float* cot[PINN_TERM_MIXED_BLOCKS];         // all null when no cotangents are wanted
};

// l(r) and l'(r) of PDEBase._apply_loss_fn per sample (term_kernels.hip::term_loss)
__device__ __forceinline__ float mixed_loss(int kind, float d, float r, float* dl) {
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

// slot of a stream code (sin / cos / coordinates have none: -1)
__host__ __device__ inline int mixed_slot(int code) {
  switch (code) {
    case 0: case 1: case 2: case 3: case 4: case 5: case 6: return code;
    case PINN_TERM_UY: return 7;
    case PINN_TERM_UYY: return 8;
    case PINN_TERM_UYYY: return 9;
    case PINN_TERM_UYYYY: return 10;
    case PINN_TERM_UZ: return 11;
    case PINN_TERM_UZZ: return 12;
    case PINN_TERM_UZZZ: return 13;
    case PINN_TERM_UZZZZ: return 14;
    case PINN_TERM_UXY: case PINN_TERM_UXZ: case PINN_TERM_UYZ: return 15 + code - PINN_TERM_UXY;
    case PINN_TERM_UXXYY: case PINN_TERM_UXXZZ: case PINN_TERM_UYYZZ: return 18 + code - PINN_TERM_UXXYY;
    default: return -1;
  }
}

// v[code] for a wave-uniform code: a scalar branch per case, every case a fixed register
__device__ __forceinline__ float mixed_value(const float (&v)[kMxCodes], unsigned code) {
#define MX_CASE(c) case c: return v[c];
  switch (code) {
    MX_CASE(0) MX_CASE(1) MX_CASE(2) MX_CASE(3) MX_CASE(4) MX_CASE(5) MX_CASE(6) MX_CASE(7) MX_CASE(8) MX_CASE(9)
    MX_CASE(10) MX_CASE(11) MX_CASE(12) MX_CASE(13) MX_CASE(14) MX_CASE(15) MX_CASE(16) MX_CASE(17) MX_CASE(18)
    MX_CASE(19) MX_CASE(20) MX_CASE(21) MX_CASE(22) MX_CASE(23) MX_CASE(24) MX_CASE(25)
    default: return v[26];
  }
#undef MX_CASE
}

// d[slot of code] += a, the same way
__device__ __forceinline__ void mixed_add(float (&d)[kMxSlots], unsigned code, float a) {
#define MX_CASE(c, s) case c: d[s] += a; break;
  switch (code) {
    MX_CASE(0, 0) MX_CASE(1, 1) MX_CASE(2, 2) MX_CASE(3, 3) MX_CASE(4, 4) MX_CASE(5, 5) MX_CASE(6, 6)
    MX_CASE(PINN_TERM_UY, 7) MX_CASE(PINN_TERM_UYY, 8) MX_CASE(PINN_TERM_UYYY, 9) MX_CASE(PINN_TERM_UYYYY, 10)
    MX_CASE(PINN_TERM_UZ, 11) MX_CASE(PINN_TERM_UZZ, 12) MX_CASE(PINN_TERM_UZZZ, 13) MX_CASE(PINN_TERM_UZZZZ, 14)
    MX_CASE(PINN_TERM_UXY, 15) MX_CASE(PINN_TERM_UXZ, 16) MX_CASE(PINN_TERM_UYZ, 17)
    MX_CASE(PINN_TERM_UXXYY, 18) MX_CASE(PINN_TERM_UXXZZ, 19)
    default: d[20] += a; break;
  }
#undef MX_CASE
}

// row of block 0 that holds code s (0 .. 6) in the (nt, nx) set, or -1 when the set does not hold it
__host__ __device__ inline int mixed_row0(int code, int nt, int nx) {
  if (code == 0) return 0;
  if (code <= 2) return code <= nt ? code : -1;
  return code - 2 <= nx ? nt + code - 2 : -1;
}

__host__ __device__ inline bool mixed_is_coord(unsigned code) {
  return code == PINN_TERM_X || code == PINN_TERM_T || code == PINN_TERM_Y || code == PINN_TERM_Z;
}

// REDUCE: loss and / or coefficient sums are wanted (per-block partials);  COEF: coefficient sums are wanted.
// partial[b * kMxRow] = sum l(r_n), partial[b * kMxRow + 1 + m] = sum rbar_n prod_f phi_{m,f} over block b's points.
template <bool REDUCE, bool COEF>
__global__ __launch_bounds__(256) void term_mixed_kernel(MixedProg p, const float* __restrict__ coef, const float* __restrict__ x,
                                                         const float* __restrict__ t, long long N, float grad_scale,
                                                         const float* __restrict__ rbar_in, float* __restrict__ residual_out,
                                                         double* __restrict__ partial) {
  double loss_acc = 0.0;
  double cg[COEF ? PINN_TERM_MAX_TERMS : 1];
#pragma unroll
  for (int m = 0; m < (COEF ? PINN_TERM_MAX_TERMS : 1); ++m) cg[m] = 0.0;
  const float* __restrict__ j0 = p.jets[0];
  const float* __restrict__ j1 = p.jets[1];
  const float* __restrict__ j2 = p.jets[2];
  const bool want_cot = p.cot[0] != nullptr;
  const unsigned need = p.need;

  for (long long n = (long long)blockIdx.x * 256 + threadIdx.x; n < N; n += (long long)gridDim.x * 256) {
    float v[kMxCodes];
#pragma unroll
    for (int s = 0; s < 7; ++s) v[s] = ((need >> s) & 1u) ? j0[(long long)mixed_row0(s, p.nt, p.nx0) * N + n] : 0.0f;
    v[7] = (p.uses_coord & USE_X) ? x[n * p.dim] : 0.0f;
    v[8] = (p.uses_coord & USE_T) ? t[n] : 0.0f;
    v[9] = 0.0f;
    v[10] = 0.0f;
    if (p.uses_trig) {
      v[9] = sinf(v[0]);
      v[10] = cosf(v[0]);
    }
    v[PINN_TERM_UY] = ((need >> 7) & 1u) ? j1[N + n] : 0.0f;
    v[PINN_TERM_UYY] = ((need >> 8) & 1u) ? j1[2 * N + n] : 0.0f;
    v[PINN_TERM_UYYY] = ((need >> 9) & 1u) ? j1[3 * N + n] : 0.0f;
    v[PINN_TERM_UYYYY] = ((need >> 10) & 1u) ? j1[4 * N + n] : 0.0f;
    v[PINN_TERM_UZ] = ((need >> 11) & 1u) ? j2[N + n] : 0.0f;
    v[PINN_TERM_UZZ] = ((need >> 12) & 1u) ? j2[2 * N + n] : 0.0f;
    v[PINN_TERM_UZZZ] = ((need >> 13) & 1u) ? j2[3 * N + n] : 0.0f;
    v[PINN_TERM_UZZZZ] = ((need >> 14) & 1u) ? j2[4 * N + n] : 0.0f;
    v[PINN_TERM_Y] = (p.uses_coord & USE_Y) ? x[n * p.dim + 1] : 0.0f;
    v[PINN_TERM_Z] = (p.uses_coord & USE_Z) ? x[n * p.dim + 2] : 0.0f;
    // the derived factors, in the evaluation order the header states (K = pair, A2 / B2 / A4 / B4 = codes of the axis rows)
#define MX_DERIVE(K, A2, B2, A4, B4)                                                                                  \
  v[PINN_TERM_UXY + K] = ((need >> (15 + K)) & 1u) ? 0.5f * ((p.jets[3 + K][2 * N + n] - v[A2]) - v[B2]) : 0.0f;      \
  v[PINN_TERM_UXXYY + K] = ((need >> (18 + K)) & 1u)                                                                  \
                               ? ((p.jets[3 + K][4 * N + n] + p.jets[6 + K][4 * N + n]) - 2.0f * (v[A4] + v[B4])) * kTwelfth \
                               : 0.0f;
    MX_DERIVE(0, PINN_TERM_UXX, PINN_TERM_UYY, PINN_TERM_UXXXX, PINN_TERM_UYYYY)
    MX_DERIVE(1, PINN_TERM_UXX, PINN_TERM_UZZ, PINN_TERM_UXXXX, PINN_TERM_UZZZZ)
    MX_DERIVE(2, PINN_TERM_UYY, PINN_TERM_UZZ, PINN_TERM_UYYYY, PINN_TERM_UZZZZ)
#undef MX_DERIVE

    // r = sum_m c_m prod_f phi and d[.] = dr/d(factor), exactly as term_axes_kernel: the derivative of one term is summed on
    // its own first (at most four summands), then added to d
    float r = 0.0f;
    float d[kMxSlots];
#pragma unroll
    for (int s = 0; s < kMxSlots; ++s) d[s] = 0.0f;
    for (int m = 0; m < p.n_terms; ++m) {
      const float c = coef[m];
      const unsigned codes = p.factors[m];
      const int nf = p.n_factors[m];
      float phi[PINN_TERM_MAX_FACTORS];
#pragma unroll
      for (int f = 0; f < PINN_TERM_MAX_FACTORS; ++f) phi[f] = f < nf ? mixed_value(v, (codes >> (8 * f)) & 255u) : 1.0f;
      float prod = c;
#pragma unroll
      for (int f = 0; f < PINN_TERM_MAX_FACTORS; ++f)
        if (f < nf) prod *= phi[f];
      r += prod;
      if (want_cot) {
        float dt[kMxSlots];
#pragma unroll
        for (int s = 0; s < kMxSlots; ++s) dt[s] = 0.0f;
#pragma unroll
        for (int f = 0; f < PINN_TERM_MAX_FACTORS; ++f) {
          if (f < nf) {
            const unsigned code = (codes >> (8 * f)) & 255u;
            if (mixed_is_coord(code)) continue;  // coordinates carry no cotangent
            float others = c;
#pragma unroll
            for (int g = 0; g < PINN_TERM_MAX_FACTORS; ++g)
              if (g != f && g < nf) others *= phi[g];
            if (code == PINN_TERM_SIN_U) mixed_add(dt, 0, others * v[10]);
            else if (code == PINN_TERM_COS_U) mixed_add(dt, 0, -(others * v[9]));
            else mixed_add(dt, code, others);
          }
        }
#pragma unroll
        for (int s = 0; s < kMxSlots; ++s) d[s] += dt[s];
      }
    }

    float dl;
    const float lv = mixed_loss(p.loss, p.huber_delta, r, &dl);
    const float rbar = rbar_in ? rbar_in[n] : grad_scale * dl;
    if (residual_out) residual_out[n] = r;
    if (want_cot) {
      // the transposes of the two formulas, once per point: g = dr/du_ab -> +g/2 on P_2, -g/2 on A_2 and B_2;
      // h = dr/du_aabb -> +h/12 on P_4 and Q_4, -h/6 on A_4 and B_4 (slots: order 2 = 4, 8, 12; order 4 = 6, 10, 14)
      float p2[3], p4[3];
#define MX_TRANSPOSE(K, SA2, SB2, SA4, SB4) \
  p2[K] = 0.5f * d[15 + K];                 \
  d[SA2] -= p2[K];                          \
  d[SB2] -= p2[K];                          \
  p4[K] = d[18 + K] * kTwelfth;             \
  d[SA4] -= 2.0f * p4[K];                   \
  d[SB4] -= 2.0f * p4[K];
      MX_TRANSPOSE(0, 4, 8, 6, 10)
      MX_TRANSPOSE(1, 4, 12, 6, 14)
      MX_TRANSPOSE(2, 8, 12, 10, 14)
#undef MX_TRANSPOSE
      float* __restrict__ c0 = p.cot[0];
#pragma unroll
      for (int s = 0; s < 7; ++s) {
        const int row = mixed_row0(s, p.nt, p.nx0);
        if (row >= 0) c0[(long long)row * N + n] = rbar * d[s];
      }
      if (p.nx1 >= 1) {  // row 0 of a further block is zero: the whole cotangent of u went to block 0
        float* __restrict__ c1 = p.cot[1];
        c1[n] = 0.0f;
#pragma unroll
        for (int k = 1; k <= 4; ++k)
          if (k <= p.nx1) c1[(long long)k * N + n] = rbar * d[6 + k];
      }
      if (p.nx2 >= 1) {
        float* __restrict__ c2 = p.cot[2];
        c2[n] = 0.0f;
#pragma unroll
        for (int k = 1; k <= 4; ++k)
          if (k <= p.nx2) c2[(long long)k * N + n] = rbar * d[10 + k];
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (p.po[k] >= 2) {  // rows 0, 1 and 3 of a P / Q block are never read: zeros
          float* __restrict__ cp = p.cot[3 + k];
          cp[n] = 0.0f;
          cp[N + n] = 0.0f;
          cp[2 * N + n] = rbar * p2[k];
          if (p.po[k] == 4) {
            float* __restrict__ cq = p.cot[6 + k];
            cp[3 * N + n] = 0.0f;
            cp[4 * N + n] = rbar * p4[k];
            cq[n] = 0.0f;
            cq[N + n] = 0.0f;
            cq[2 * N + n] = 0.0f;
            cq[3 * N + n] = 0.0f;
            cq[4 * N + n] = rbar * p4[k];
          }
        }
      }
    }
    if (REDUCE) loss_acc += (double)lv;
    if (COEF) {
#pragma unroll
      for (int m = 0; m < PINN_TERM_MAX_TERMS; ++m) {
        if (m < p.n_terms) {
          const unsigned codes = p.factors[m];
          const int nf = p.n_factors[m];
          float prod = 1.0f;
#pragma unroll
          for (int f = 0; f < PINN_TERM_MAX_FACTORS; ++f)
            if (f < nf) prod *= mixed_value(v, (codes >> (8 * f)) & 255u);
          cg[m] += (double)(rbar * prod);
        }
      }
    }
  }

  if (REDUCE) {
    __shared__ double red[256];
    const int rows = COEF ? 1 + p.n_terms : 1;
#pragma unroll
    for (int k = 0; k < kMxRow; ++k) {
      if (k < rows) {
        red[threadIdx.x] = k == 0 ? loss_acc : cg[COEF ? k - 1 : 0];
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
          if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
          __syncthreads();
        }
        if (threadIdx.x == 0) partial[blockIdx.x * kMxRow + k] = red[0];
        __syncthreads();
      }
    }
  }
}

// thread k < rows: sum k of the block partials in block order, in double, added to its output and rounded once
__global__ void term_mixed_finish_kernel(const double* partial, int blocks, int n_terms, float* loss_sum_out, float* coef_grads) {
  const int k = threadIdx.x;
  if (k > n_terms) return;
  float* out = k == 0 ? loss_sum_out : (coef_grads ? coef_grads + (k - 1) : nullptr);
  if (!out) return;
  double s = 0.0;
  for (int b = 0; b < blocks; ++b) s += partial[b * kMxRow + k];
  out[0] = (float)((double)out[0] + s);
}

// the stream sets the library has axis-0 units for (csrc/Makefile: SETS)
bool mixed_set_compiled(int nt, int nx) {
  static const int sets[][2] = {{0, 0}, {1, 0}, {1, 1}, {1, 2}, {1, 3}, {1, 4}, {2, 0}, {2, 2}};
  for (const auto& s : sets)
    if (s[0] == nt && s[1] == nx) return true;
  return false;
}

constexpr int kPairA[3] = {0, 0, 1}, kPairB[3] = {1, 2, 2};
constexpr int kSlot2[3] = {4, 8, 12}, kSlot4[3] = {6, 10, 14};  // slots of the order-2 / order-4 row of each axis

}  // namespace

extern "C" int pinn_internal_fail(int code, const char* msg);  // pinn_abi.hip: sets pinn_last_error()

static int mixed_launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return PINN_OK;
  char msg[256];
  snprintf(msg, sizeof(msg), "HIP error %d: %s (%s)", (int)e, hipGetErrorString(e), what);
  return pinn_internal_fail(PINN_ERR_HIP, msg);
}

extern "C" int pinn_term_residual_mixed(const PinnTermPdeMixed* pde, const float* coef_values, const float* const* jets,
                                        const float* x, const float* t, int64_t N, float grad_scale,
                                        const float* residual_cotangent, float* residual_out, float* loss_sum_out,
                                        float* const* jet_cotangents, float* coef_grads, double* scratch, void* stream) {
  char msg[256];
  if (!pde) return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_term_residual_mixed: null descriptor");
  const int dim = pde->dimension;
  if (dim != 2 && dim != 3) {
    snprintf(msg, sizeof(msg), "pinn_term_residual_mixed: dimension %d (2 or 3; pinn_term_residual runs 1-D problems)", dim);
    return pinn_internal_fail(PINN_ERR_BAD_DESC, msg);
  }
  if (pde->n_terms < 0 || pde->n_terms > PINN_TERM_MAX_TERMS) {
    snprintf(msg, sizeof(msg), "pinn_term_residual_mixed: n_terms %d outside [0, %d]", (int)pde->n_terms, PINN_TERM_MAX_TERMS);
    return pinn_internal_fail(PINN_ERR_BAD_DESC, msg);
  }
  const int nt = pde->time_order, nx0 = pde->space_order[0];
  if (!mixed_set_compiled(nt, nx0)) {
    snprintf(msg, sizeof(msg), "pinn_term_residual_mixed: axis-0 stream set (nt=%d, nx=%d) is not compiled", nt, nx0);
    return pinn_internal_fail(PINN_ERR_BAD_DESC, msg);
  }
  for (int a = 1; a < 3; ++a) {
    const int so = pde->space_order[a];
    if (so < 0 || so > (a < dim ? 4 : 0)) {
      snprintf(msg, sizeof(msg), "pinn_term_residual_mixed: space_order[%d] = %d outside [0, %d] (dimension %d)", a, so,
               a < dim ? 4 : 0, dim);
      return pinn_internal_fail(PINN_ERR_BAD_DESC, msg);
    }
  }
  const int order[3] = {nx0, pde->space_order[1], pde->space_order[2]};
  for (int k = 0; k < 3; ++k) {
    const int po = pde->pair_order[k];
    if (po != 0 && po != 2 && po != 4) {
      snprintf(msg, sizeof(msg), "pinn_term_residual_mixed: pair_order[%d] = %d (0, 2 or 4)", k, po);
      return pinn_internal_fail(PINN_ERR_BAD_DESC, msg);
    }
    if (po != 0 && kPairB[k] >= dim) {
      snprintf(msg, sizeof(msg), "pinn_term_residual_mixed: pair_order[%d] = %d on the pair of axes (%d, %d), dimension %d", k, po,
               kPairA[k], kPairB[k], dim);
      return pinn_internal_fail(PINN_ERR_BAD_DESC, msg);
    }
  }
  MixedProg p;
  p.n_terms = pde->n_terms;
  p.dim = dim;
  p.nt = nt;
  p.nx0 = nx0;
  p.nx1 = order[1];
  p.nx2 = order[2];
  for (int k = 0; k < 3; ++k) p.po[k] = pde->pair_order[k];
  p.loss = pde->loss;
  p.huber_delta = pde->huber_delta;
  p.uses_trig = 0;
  p.uses_coord = 0;
  p.need = 0;
  for (int m = 0; m < PINN_TERM_MAX_TERMS; ++m) {
    p.factors[m] = 0xffffffffu;
    p.n_factors[m] = 0;
  }
  for (int m = 0; m < pde->n_terms; ++m) {
    const PinnTermPdeTerm& tm = pde->terms[m];
    if (tm.n_factors < 0 || tm.n_factors > PINN_TERM_MAX_FACTORS) {
      snprintf(msg, sizeof(msg), "pinn_term_residual_mixed: term %d has n_factors %d outside [0, %d]", m, (int)tm.n_factors,
               PINN_TERM_MAX_FACTORS);
      return pinn_internal_fail(PINN_ERR_BAD_DESC, msg);
    }
    unsigned packed = 0xffffffffu;
    for (int f = 0; f < tm.n_factors; ++f) {
      const int code = tm.factor[f];
      if (code < 0 || code >= kMxCodes) {
        snprintf(msg, sizeof(msg), "pinn_term_residual_mixed: term %d, factor %d: unknown factor code %d", m, f, code);
        return pinn_internal_fail(PINN_ERR_BAD_DESC, msg);
      }
      const int slot = mixed_slot(code);
      bool held = true;
      if (code < 7) held = mixed_row0(code, nt, nx0) >= 0;
      else if (slot >= 7 && slot <= 10) held = p.nx1 >= slot - 6;
      else if (slot >= 11 && slot <= 14) held = p.nx2 >= slot - 10;
      else if (code == PINN_TERM_Z) held = dim >= 3;
      else if (slot >= 15) {
        const int k = (slot - 15) % 3, o = slot >= 18 ? 4 : 2;
        const bool ok = o == 2 ? (p.po[k] >= 2 && order[kPairA[k]] >= 2 && order[kPairB[k]] >= 2)
                               : (p.po[k] == 4 && order[kPairA[k]] == 4 && order[kPairB[k]] == 4);
        if (!ok) {
          snprintf(msg, sizeof(msg), "pinn_term_residual_mixed: term %d, factor %d names a mixed derivative (code %d) of the axes "
                   "(%d, %d), which needs pair_order %s %d and order %s %d on both axes (pair_order %d, orders %d, %d)", m, f, code,
                   kPairA[k], kPairB[k], o == 2 ? ">=" : "=", o, o == 2 ? ">=" : "=", o, p.po[k], order[kPairA[k]], order[kPairB[k]]);
          return pinn_internal_fail(PINN_ERR_BAD_DESC, msg);
        }
        p.need |= 1u << (o == 2 ? kSlot2[kPairA[k]] : kSlot4[kPairA[k]]);
        p.need |= 1u << (o == 2 ? kSlot2[kPairB[k]] : kSlot4[kPairB[k]]);
      }
      if (!held) {
        snprintf(msg, sizeof(msg), "pinn_term_residual_mixed: term %d, factor %d names a stream or coordinate (code %d) that the "
                 "descriptor (dimension %d, nt=%d, space orders %d, %d, %d) does not hold", m, f, code, dim, nt, nx0, p.nx1, p.nx2);
        return pinn_internal_fail(PINN_ERR_BAD_DESC, msg);
      }
      if (slot >= 0) p.need |= 1u << slot;
      if (code == PINN_TERM_X) p.uses_coord |= USE_X;
      if (code == PINN_TERM_Y) p.uses_coord |= USE_Y;
      if (code == PINN_TERM_Z) p.uses_coord |= USE_Z;
      if (code == PINN_TERM_T) p.uses_coord |= USE_T;
      if (code == PINN_TERM_SIN_U || code == PINN_TERM_COS_U) {
        p.uses_trig = 1;
        p.need |= 1u;
      }
      packed = (packed & ~(255u << (8 * f))) | ((unsigned)code << (8 * f));
    }
    p.factors[m] = packed;
    p.n_factors[m] = tm.n_factors;
  }
  if (N < 0) return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_term_residual_mixed: N < 0");
  if (N == 0) return PINN_OK;
  if (!jets || !coef_values) return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_term_residual_mixed: null jets table or coef_values");
  for (int b = 0; b < PINN_TERM_MIXED_BLOCKS; ++b) {
    bool has;
    if (b == 0) has = true;  // block 0 always holds the value stream
    else if (b < 3) has = b < dim && order[b] > 0;
    else if (b < 6) has = p.po[b - 3] >= 2;
    else has = p.po[b - 6] == 4;
    p.jets[b] = has ? jets[b] : nullptr;
    p.cot[b] = (jet_cotangents && has) ? jet_cotangents[b] : nullptr;
    if (has && (!p.jets[b] || (jet_cotangents && !p.cot[b]))) {
      if (b < 3) snprintf(msg, sizeof(msg), "pinn_term_residual_mixed: null block %d of the jets or jet_cotangents table (axis %d has streams)", b, b);
      else snprintf(msg, sizeof(msg), "pinn_term_residual_mixed: null block %d of the jets or jet_cotangents table (the %c block of the pair "
                    "(%d, %d), pair_order %d)", b, b < 6 ? 'P' : 'Q', kPairA[(b - 3) % 3], kPairB[(b - 3) % 3], p.po[(b - 3) % 3]);
      return pinn_internal_fail(PINN_ERR_BAD_DESC, msg);
    }
  }
  if (((p.uses_coord & (USE_X | USE_Y | USE_Z)) && !x) || ((p.uses_coord & USE_T) && !t))
    return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_term_residual_mixed: a term names X / Y / Z / T but the coordinate array is null");
  const bool reduce = loss_sum_out || coef_grads;
  if (reduce && !scratch)
    return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_term_residual_mixed: null scratch with a loss or coefficient sum");
  if (reinterpret_cast<uintptr_t>(scratch) & 7u)
    return pinn_internal_fail(PINN_ERR_MISALIGNED, "pinn_term_residual_mixed: scratch must be 8-byte aligned");

  long long nb = ((long long)N + 255) / 256;
  const int blocks = (int)(nb > kMxBlocks ? kMxBlocks : nb);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (!reduce) {
    hipLaunchKernelGGL((term_mixed_kernel<false, false>), dim3(blocks), dim3(256), 0, st, p, coef_values, x, t, (long long)N,
                       grad_scale, residual_cotangent, residual_out, scratch);
    return mixed_launched("term_mixed_kernel");
  }
  if (coef_grads)
    hipLaunchKernelGGL((term_mixed_kernel<true, true>), dim3(blocks), dim3(256), 0, st, p, coef_values, x, t, (long long)N,
                       grad_scale, residual_cotangent, residual_out, scratch);
  else
    hipLaunchKernelGGL((term_mixed_kernel<true, false>), dim3(blocks), dim3(256), 0, st, p, coef_values, x, t, (long long)N,
                       grad_scale, residual_cotangent, residual_out, scratch);
  int rc = mixed_launched("term_mixed_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(term_mixed_finish_kernel, dim3(1), dim3(64), 0, st, scratch, blocks, (int)p.n_terms, loss_sum_out, coef_grads);
  return mixed_launched("term_mixed_finish_kernel");
}
