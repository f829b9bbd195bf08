// Residuals given as data in two or three space dimensions (include/pinn_jet.h, "term residuals along every space axis"):
// the element-wise middle of the chain
//   pinn_jet_forward (axis 0) [+ pinn_jet_forward per further axis] -> pinn_term_residual_axes -> pinn_jet_backward per axis.
// The scheme is term_kernels.hip's: one thread per point, the streams of every block, the coordinates and sin / cos of the
// value in registers, indexed by factor code through wave-uniform switches; the term list is a kernel argument and the
// coefficients are read from the device at launch time.  An HBM-bound pass over the blocks, read once and written once.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../../include/pinn_jet.h"

namespace {

constexpr int kAxBlocks = 64;                      // fixed grid: the partials are summed in block order
constexpr int kAxRow = 1 + PINN_TERM_MAX_TERMS;    // doubles per block: {loss, coefficient sums}
constexpr int kAxSlots = 17;                       // factor codes 0 .. 16
constexpr int kAxStreams = 11;                     // derivative accumulators: codes 0 .. 6, then u_y, u_yy, u_z, u_zz

static_assert(PINN_TERM_SCRATCH_DOUBLES == kAxBlocks * kAxRow, "scratch constant and grid disagree");

enum { USE_X = 1, USE_Y = 2, USE_Z = 4, USE_T = 8 };

// the descriptor as the kernel reads it: factor codes packed one byte each, unused positions = 255
struct AxesProg {
  int n_terms, dim, nt, nx0, nx1, nx2, loss;
  float huber_delta;
  int uses_trig, uses_coord;
  unsigned factors[PINN_TERM_MAX_TERMS];  // byte f = code of factor f
  int n_factors[PINN_TERM_MAX_TERMS];
  const float* jets[3];                   // block a, null when the axis has no streams (a >= 1)
  float* cot[3];                          // all null when no cotangents are wanted
};

// l(r) and l'(r) of PDEBase._apply_loss_fn per sample (term_kernels.hip::term_loss)
__device__ __forceinline__ float axes_loss(int kind, float d, float r, float* dl) {
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

// v[code] for a wave-uniform code: a scalar branch per case, every case a fixed register
__device__ __forceinline__ float axes_value(const float (&v)[kAxSlots], unsigned code) {
  switch (code) {
    case 0: return v[0];
    case 1: return v[1];
    case 2: return v[2];
    case 3: return v[3];
    case 4: return v[4];
    case 5: return v[5];
    case 6: return v[6];
    case 7: return v[7];
    case 8: return v[8];
    case 9: return v[9];
    case 10: return v[10];
    case 11: return v[11];
    case 12: return v[12];
    case 13: return v[13];
    case 14: return v[14];
    case 15: return v[15];
    default: return v[16];
  }
}

// accumulator of a stream code: 0 .. 6 as they are, u_y / u_yy / u_z / u_zz behind them
__device__ __forceinline__ void axes_add(float (&d)[kAxStreams], unsigned code, float a) {
  switch (code) {
    case 0: d[0] += a; break;
    case 1: d[1] += a; break;
    case 2: d[2] += a; break;
    case 3: d[3] += a; break;
    case 4: d[4] += a; break;
    case 5: d[5] += a; break;
    case 6: d[6] += a; break;
    case PINN_TERM_UY: d[7] += a; break;
    case PINN_TERM_UYY: d[8] += a; break;
    case PINN_TERM_UZ: d[9] += a; break;
    default: d[10] += a; break;
  }
}

// row of block 0 that holds code s (0 .. 6) in the (nt, nx) set, or -1 when the set does not hold it
__host__ __device__ inline int axes_row0(int code, int nt, int nx) {
  if (code == 0) return 0;
  if (code <= 2) return code <= nt ? code : -1;
  return code - 2 <= nx ? nt + code - 2 : -1;
}

__host__ __device__ inline bool axes_is_coord(unsigned code) {
  return code == PINN_TERM_X || code == PINN_TERM_T || code == PINN_TERM_Y || code == PINN_TERM_Z;
}

// REDUCE: loss and / or coefficient sums are wanted (per-block partials);  COEF: coefficient sums are wanted.
// partial[b * kAxRow] = sum l(r_n), partial[b * kAxRow + 1 + m] = sum rbar_n prod_f phi_{m,f} over block b's points.
template <bool REDUCE, bool COEF>
__global__ __launch_bounds__(256) void term_axes_kernel(AxesProg p, const float* __restrict__ coef, const float* __restrict__ x,
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

  for (long long n = (long long)blockIdx.x * 256 + threadIdx.x; n < N; n += (long long)gridDim.x * 256) {
    float v[kAxSlots];
#pragma unroll
    for (int s = 0; s < 7; ++s) {
      const int row = axes_row0(s, p.nt, p.nx0);
      v[s] = row >= 0 ? j0[(long long)row * N + n] : 0.0f;
    }
    v[7] = (p.uses_coord & USE_X) ? x[n * p.dim] : 0.0f;
    v[8] = (p.uses_coord & USE_T) ? t[n] : 0.0f;
    v[9] = 0.0f;
    v[10] = 0.0f;
    if (p.uses_trig) {
      v[9] = sinf(v[0]);
      v[10] = cosf(v[0]);
    }
    v[11] = p.nx1 >= 1 ? j1[N + n] : 0.0f;
    v[12] = p.nx1 >= 2 ? j1[2 * N + n] : 0.0f;
    v[13] = p.nx2 >= 1 ? j2[N + n] : 0.0f;
    v[14] = p.nx2 >= 2 ? j2[2 * N + n] : 0.0f;
    v[15] = (p.uses_coord & USE_Y) ? x[n * p.dim + 1] : 0.0f;
    v[16] = (p.uses_coord & USE_Z) ? x[n * p.dim + 2] : 0.0f;

    // r = sum_m c_m prod_f phi and d[.] = dr/d(stream).  The derivative of one term is summed on its own first (at most
    // four summands), then added to d: the rounding count of d[.] is that of r, whatever the program.
    float r = 0.0f;
    float d[kAxStreams];
#pragma unroll
    for (int s = 0; s < kAxStreams; ++s) d[s] = 0.0f;
    for (int m = 0; m < p.n_terms; ++m) {
      const float c = coef[m];
      const unsigned codes = p.factors[m];
      const int nf = p.n_factors[m];
      float phi[PINN_TERM_MAX_FACTORS];
#pragma unroll
      for (int f = 0; f < PINN_TERM_MAX_FACTORS; ++f) phi[f] = f < nf ? axes_value(v, (codes >> (8 * f)) & 255u) : 1.0f;
      float prod = c;
#pragma unroll
      for (int f = 0; f < PINN_TERM_MAX_FACTORS; ++f)
        if (f < nf) prod *= phi[f];
      r += prod;
      if (want_cot) {
        float dt[kAxStreams];
#pragma unroll
        for (int s = 0; s < kAxStreams; ++s) dt[s] = 0.0f;
#pragma unroll
        for (int f = 0; f < PINN_TERM_MAX_FACTORS; ++f) {
          if (f < nf) {
            const unsigned code = (codes >> (8 * f)) & 255u;
            if (axes_is_coord(code)) continue;  // coordinates carry no cotangent
            float others = c;
#pragma unroll
            for (int g = 0; g < PINN_TERM_MAX_FACTORS; ++g)
              if (g != f && g < nf) others *= phi[g];
            if (code == PINN_TERM_SIN_U) axes_add(dt, 0, others * v[10]);
            else if (code == PINN_TERM_COS_U) axes_add(dt, 0, -(others * v[9]));
            else axes_add(dt, code, others);
          }
        }
#pragma unroll
        for (int s = 0; s < kAxStreams; ++s) d[s] += dt[s];
      }
    }

    float dl;
    const float lv = axes_loss(p.loss, p.huber_delta, r, &dl);
    const float rbar = rbar_in ? rbar_in[n] : grad_scale * dl;
    if (residual_out) residual_out[n] = r;
    if (want_cot) {
      float* __restrict__ c0 = p.cot[0];
#pragma unroll
      for (int s = 0; s < 7; ++s) {
        const int row = axes_row0(s, p.nt, p.nx0);
        if (row >= 0) c0[(long long)row * N + n] = rbar * d[s];
      }
      if (p.nx1 >= 1) {  // row 0 of a further block is zero: the whole cotangent of u went to block 0
        float* __restrict__ c1 = p.cot[1];
        c1[n] = 0.0f;
        c1[N + n] = rbar * d[7];
        if (p.nx1 >= 2) c1[2 * N + n] = rbar * d[8];
      }
      if (p.nx2 >= 1) {
        float* __restrict__ c2 = p.cot[2];
        c2[n] = 0.0f;
        c2[N + n] = rbar * d[9];
        if (p.nx2 >= 2) c2[2 * N + n] = rbar * d[10];
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
            if (f < nf) prod *= axes_value(v, (codes >> (8 * f)) & 255u);
          cg[m] += (double)(rbar * prod);
        }
      }
    }
  }

  if (REDUCE) {
    __shared__ double red[256];
    const int rows = COEF ? 1 + p.n_terms : 1;
#pragma unroll
    for (int k = 0; k < kAxRow; ++k) {
      if (k < rows) {
        red[threadIdx.x] = k == 0 ? loss_acc : cg[COEF ? k - 1 : 0];
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
          if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
          __syncthreads();
        }
        if (threadIdx.x == 0) partial[blockIdx.x * kAxRow + k] = red[0];
        __syncthreads();
      }
    }
  }
}

// thread k < rows: sum k of the block partials in block order, in double, added to its output and rounded once
__global__ void term_axes_finish_kernel(const double* partial, int blocks, int n_terms, float* loss_sum_out, float* coef_grads) {
  const int k = threadIdx.x;
  if (k > n_terms) return;
  float* out = k == 0 ? loss_sum_out : (coef_grads ? coef_grads + (k - 1) : nullptr);
  if (!out) return;
  double s = 0.0;
  for (int b = 0; b < blocks; ++b) s += partial[b * kAxRow + k];
  out[0] = (float)((double)out[0] + s);
}

// the stream sets the library has axis-0 units for (csrc/Makefile: SETS)
bool axes_set_compiled(int nt, int nx) {
  static const int sets[][2] = {{0, 0}, {1, 0}, {1, 1}, {1, 2}, {1, 3}, {1, 4}, {2, 0}, {2, 2}};
  for (const auto& s : sets)
    if (s[0] == nt && s[1] == nx) return true;
  return false;
}

}  // namespace

extern "C" int pinn_internal_fail(int code, const char* msg);  // pinn_abi.hip: sets pinn_last_error()

static int axes_launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return PINN_OK;
  char msg[256];
  snprintf(msg, sizeof(msg), "HIP error %d: %s (%s)", (int)e, hipGetErrorString(e), what);
  return pinn_internal_fail(PINN_ERR_HIP, msg);
}

extern "C" int pinn_term_residual_axes(const PinnTermPdeAxes* pde, const float* coef_values, const float* const* jets,
                                       const float* x, const float* t, int64_t N, float grad_scale,
                                       const float* residual_cotangent, float* residual_out, float* loss_sum_out,
                                       float* const* jet_cotangents, float* coef_grads, double* scratch, void* stream) {
  char msg[200];
  if (!pde) return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_term_residual_axes: null descriptor");
  const int dim = pde->dimension;
  if (dim != 2 && dim != 3) {
    snprintf(msg, sizeof(msg), "pinn_term_residual_axes: dimension %d (2 or 3; pinn_term_residual runs 1-D problems)", dim);
    return pinn_internal_fail(PINN_ERR_BAD_DESC, msg);
  }
  if (pde->n_terms < 0 || pde->n_terms > PINN_TERM_MAX_TERMS) {
    snprintf(msg, sizeof(msg), "pinn_term_residual_axes: n_terms %d outside [0, %d]", (int)pde->n_terms, PINN_TERM_MAX_TERMS);
    return pinn_internal_fail(PINN_ERR_BAD_DESC, msg);
  }
  const int nt = pde->time_order, nx0 = pde->space_order[0];
  if (!axes_set_compiled(nt, nx0)) {
    snprintf(msg, sizeof(msg), "pinn_term_residual_axes: axis-0 stream set (nt=%d, nx=%d) is not compiled", nt, nx0);
    return pinn_internal_fail(PINN_ERR_BAD_DESC, msg);
  }
  for (int a = 1; a < 3; ++a) {
    const int so = pde->space_order[a];
    if (so < 0 || so > (a < dim ? 2 : 0)) {
      snprintf(msg, sizeof(msg), "pinn_term_residual_axes: space_order[%d] = %d outside [0, %d] (dimension %d)", a, so,
               a < dim ? 2 : 0, dim);
      return pinn_internal_fail(PINN_ERR_BAD_DESC, msg);
    }
  }
  AxesProg p;
  p.n_terms = pde->n_terms;
  p.dim = dim;
  p.nt = nt;
  p.nx0 = nx0;
  p.nx1 = pde->space_order[1];
  p.nx2 = pde->space_order[2];
  p.loss = pde->loss;
  p.huber_delta = pde->huber_delta;
  p.uses_trig = 0;
  p.uses_coord = 0;
  for (int m = 0; m < PINN_TERM_MAX_TERMS; ++m) {
    p.factors[m] = 0xffffffffu;
    p.n_factors[m] = 0;
  }
  for (int m = 0; m < pde->n_terms; ++m) {
    const PinnTermPdeTerm& tm = pde->terms[m];
    if (tm.n_factors < 0 || tm.n_factors > PINN_TERM_MAX_FACTORS) {
      snprintf(msg, sizeof(msg), "pinn_term_residual_axes: term %d has n_factors %d outside [0, %d]", m, (int)tm.n_factors,
               PINN_TERM_MAX_FACTORS);
      return pinn_internal_fail(PINN_ERR_BAD_DESC, msg);
    }
    unsigned packed = 0xffffffffu;
    for (int f = 0; f < tm.n_factors; ++f) {
      const int code = tm.factor[f];
      if (code < 0 || code >= kAxSlots) {
        snprintf(msg, sizeof(msg), "pinn_term_residual_axes: term %d, factor %d: unknown factor code %d", m, f, code);
        return pinn_internal_fail(PINN_ERR_BAD_DESC, msg);
      }
      bool held = true;
      if (code < 7) held = axes_row0(code, nt, nx0) >= 0;
      else if (code == PINN_TERM_UY || code == PINN_TERM_UYY) held = p.nx1 >= code - PINN_TERM_UY + 1;
      else if (code == PINN_TERM_UZ || code == PINN_TERM_UZZ) held = p.nx2 >= code - PINN_TERM_UZ + 1;
      else if (code == PINN_TERM_Z) held = dim >= 3;
      if (!held) {
        snprintf(msg, sizeof(msg), "pinn_term_residual_axes: term %d, factor %d names a stream or coordinate (code %d) that the "
                 "descriptor (dimension %d, nt=%d, space orders %d, %d, %d) does not hold", m, f, code, dim, nt, nx0, p.nx1, p.nx2);
        return pinn_internal_fail(PINN_ERR_BAD_DESC, msg);
      }
      if (code == PINN_TERM_X) p.uses_coord |= USE_X;
      if (code == PINN_TERM_Y) p.uses_coord |= USE_Y;
      if (code == PINN_TERM_Z) p.uses_coord |= USE_Z;
      if (code == PINN_TERM_T) p.uses_coord |= USE_T;
      if (code == PINN_TERM_SIN_U || code == PINN_TERM_COS_U) p.uses_trig = 1;
      packed = (packed & ~(255u << (8 * f))) | ((unsigned)code << (8 * f));
    }
    p.factors[m] = packed;
    p.n_factors[m] = tm.n_factors;
  }
  if (N < 0) return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_term_residual_axes: N < 0");
  if (N == 0) return PINN_OK;
  if (!jets || !coef_values) return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_term_residual_axes: null jets table or coef_values");
  const int so[3] = {1, p.nx1, p.nx2};  // block 0 always holds the value stream
  for (int a = 0; a < 3; ++a) {
    p.jets[a] = (a < dim && so[a] > 0) ? jets[a] : nullptr;
    p.cot[a] = (jet_cotangents && a < dim && so[a] > 0) ? jet_cotangents[a] : nullptr;
    if (a < dim && so[a] > 0 && (!p.jets[a] || (jet_cotangents && !p.cot[a]))) {
      snprintf(msg, sizeof(msg), "pinn_term_residual_axes: null block %d of the jets or jet_cotangents table (axis %d has streams)", a, a);
      return pinn_internal_fail(PINN_ERR_BAD_DESC, msg);
    }
  }
  if (((p.uses_coord & (USE_X | USE_Y | USE_Z)) && !x) || ((p.uses_coord & USE_T) && !t))
    return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_term_residual_axes: a term names X / Y / Z / T but the coordinate array is null");
  const bool reduce = loss_sum_out || coef_grads;
  if (reduce && !scratch)
    return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_term_residual_axes: null scratch with a loss or coefficient sum");
  if (reinterpret_cast<uintptr_t>(scratch) & 7u)
    return pinn_internal_fail(PINN_ERR_MISALIGNED, "pinn_term_residual_axes: scratch must be 8-byte aligned");

  long long nb = ((long long)N + 255) / 256;
  const int blocks = (int)(nb > kAxBlocks ? kAxBlocks : nb);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (!reduce) {
    hipLaunchKernelGGL((term_axes_kernel<false, false>), dim3(blocks), dim3(256), 0, st, p, coef_values, x, t, (long long)N,
                       grad_scale, residual_cotangent, residual_out, scratch);
    return axes_launched("term_axes_kernel");
  }
  if (coef_grads)
    hipLaunchKernelGGL((term_axes_kernel<true, true>), dim3(blocks), dim3(256), 0, st, p, coef_values, x, t, (long long)N,
                       grad_scale, residual_cotangent, residual_out, scratch);
  else
    hipLaunchKernelGGL((term_axes_kernel<true, false>), dim3(blocks), dim3(256), 0, st, p, coef_values, x, t, (long long)N,
                       grad_scale, residual_cotangent, residual_out, scratch);
  int rc = axes_launched("term_axes_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(term_axes_finish_kernel, dim3(1), dim3(64), 0, st, scratch, blocks, (int)p.n_terms, loss_sum_out, coef_grads);
  return axes_launched("term_axes_finish_kernel");
}
