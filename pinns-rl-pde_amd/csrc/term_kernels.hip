// Residuals given as data (include/pinn_jet.h, "residuals given as data"): the element-wise middle of the chain
// pinn_jet_forward -> pinn_term_residual -> pinn_jet_backward.  One thread per point: the K streams of the point, its
// coordinates and sin / cos of its value sit in registers, indexed by PinnTermFactor code; the term list is a kernel
// argument (scalar loads) and the coefficients are read from the device at launch time.  Every branch on the term list is
// wave-uniform.  An HBM-bound pass over (2K + 3) * 4 bytes per point.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../../include/pinn_jet.h"

namespace {

constexpr int kTermBlocks = 64;                         // fixed grid: the partials are summed in block order
constexpr int kTermRow = 1 + PINN_TERM_MAX_TERMS;       // doubles per block: {loss, coefficient sums}
constexpr int kSlots = 11;                              // PinnTermFactor codes
constexpr int kStreams = PINN_MAX_STREAMS;              // codes 0 .. 6 are streams

static_assert(PINN_TERM_SCRATCH_DOUBLES == kTermBlocks * kTermRow, "scratch constant and grid disagree");

// the descriptor as the kernel reads it: factor codes packed one byte each, unused positions = 255
struct TermProg {
  int n_terms, nt, nx, loss;
  float huber_delta;
  int uses_trig;
  unsigned factors[PINN_TERM_MAX_TERMS];  // byte f = code of factor f
  int n_factors[PINN_TERM_MAX_TERMS];
};

// l(r) and l'(r) of PDEBase._apply_loss_fn per sample (jet_device.h::loss_term)
__device__ __forceinline__ float term_loss(int kind, float d, float r, float* dl) {
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
__device__ __forceinline__ float slot_value(const float (&v)[kSlots], unsigned code) {
  switch (code) {
    case PINN_TERM_U: return v[0];
    case PINN_TERM_UT: return v[1];
    case PINN_TERM_UTT: return v[2];
    case PINN_TERM_UX: return v[3];
    case PINN_TERM_UXX: return v[4];
    case PINN_TERM_UXXX: return v[5];
    case PINN_TERM_UXXXX: return v[6];
    case PINN_TERM_X: return v[7];
    case PINN_TERM_T: return v[8];
    case PINN_TERM_SIN_U: return v[9];
    default: return v[10];
  }
}

__device__ __forceinline__ void slot_add(float (&d)[kStreams], unsigned code, float a) {
  switch (code) {
    case 0: d[0] += a; break;
    case 1: d[1] += a; break;
    case 2: d[2] += a; break;
    case 3: d[3] += a; break;
    case 4: d[4] += a; break;
    case 5: d[5] += a; break;
    default: d[6] += a; break;
  }
}

// stream index of code s (0 .. 6) in the (nt, nx) set, or -1 when the set does not hold it
__host__ __device__ inline int stream_of_code(int code, int nt, int nx) {
  if (code == 0) return 0;
  if (code <= 2) return code <= nt ? code : -1;
  return code - 2 <= nx ? nt + code - 2 : -1;
}

// REDUCE: loss and / or coefficient sums are wanted (per-block partials);  COEF: coefficient sums are wanted.
// partial[b * kTermRow] = sum l(r_n), partial[b * kTermRow + 1 + m] = sum rbar_n prod_f phi_{m,f} over block b's points.
template <bool REDUCE, bool COEF>
__global__ __launch_bounds__(256) void term_residual_kernel(TermProg p, const float* __restrict__ coef, const float* __restrict__ jets,
                                                            const float* __restrict__ x, const float* __restrict__ t, long long N,
                                                            float grad_scale, const float* __restrict__ rbar_in,
                                                            float* __restrict__ residual_out, float* __restrict__ cot,
                                                            double* __restrict__ partial) {
  double loss_acc = 0.0;
  double cg[COEF ? PINN_TERM_MAX_TERMS : 1];
#pragma unroll
  for (int m = 0; m < (COEF ? PINN_TERM_MAX_TERMS : 1); ++m) cg[m] = 0.0;

  for (long long n = (long long)blockIdx.x * 256 + threadIdx.x; n < N; n += (long long)gridDim.x * 256) {
    float v[kSlots];
#pragma unroll
    for (int s = 0; s < kStreams; ++s) {
      const int row = stream_of_code(s, p.nt, p.nx);
      v[s] = row >= 0 ? jets[(long long)row * N + n] : 0.0f;
    }
    v[7] = x ? x[n] : 0.0f;
    v[8] = t ? t[n] : 0.0f;
    v[9] = 0.0f;
    v[10] = 0.0f;
    if (p.uses_trig) {
      v[9] = sinf(v[0]);
      v[10] = cosf(v[0]);
    }

    // r = sum_m c_m prod_f phi and d[s] = dr/d(stream code s).  The derivative of one term is summed on its own first
    // (at most four summands), then added to d: the rounding count of d[s] is that of r, whatever the program.
    float r = 0.0f;
    float d[kStreams];
#pragma unroll
    for (int s = 0; s < kStreams; ++s) d[s] = 0.0f;
    for (int m = 0; m < p.n_terms; ++m) {
      const float c = coef[m];
      const unsigned codes = p.factors[m];
      const int nf = p.n_factors[m];
      float phi[PINN_TERM_MAX_FACTORS];
#pragma unroll
      for (int f = 0; f < PINN_TERM_MAX_FACTORS; ++f) phi[f] = f < nf ? slot_value(v, (codes >> (8 * f)) & 255u) : 1.0f;
      float prod = c;
#pragma unroll
      for (int f = 0; f < PINN_TERM_MAX_FACTORS; ++f)
        if (f < nf) prod *= phi[f];
      r += prod;
      if (cot) {
        float dt[kStreams];
#pragma unroll
        for (int s = 0; s < kStreams; ++s) dt[s] = 0.0f;
#pragma unroll
        for (int f = 0; f < PINN_TERM_MAX_FACTORS; ++f) {
          if (f < nf) {
            const unsigned code = (codes >> (8 * f)) & 255u;
            if (code == PINN_TERM_X || code == PINN_TERM_T) continue;  // coordinates carry no cotangent
            float others = c;
#pragma unroll
            for (int g = 0; g < PINN_TERM_MAX_FACTORS; ++g)
              if (g != f && g < nf) others *= phi[g];
            if (code == PINN_TERM_SIN_U) slot_add(dt, 0, others * v[10]);
            else if (code == PINN_TERM_COS_U) slot_add(dt, 0, -(others * v[9]));
            else slot_add(dt, code, others);
          }
        }
#pragma unroll
        for (int s = 0; s < kStreams; ++s) d[s] += dt[s];
      }
    }

    float dl;
    const float lv = term_loss(p.loss, p.huber_delta, r, &dl);
    const float rbar = rbar_in ? rbar_in[n] : grad_scale * dl;
    if (residual_out) residual_out[n] = r;
    if (cot) {
#pragma unroll
      for (int s = 0; s < kStreams; ++s) {
        const int row = stream_of_code(s, p.nt, p.nx);
        if (row >= 0) cot[(long long)row * N + n] = rbar * d[s];
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
            if (f < nf) prod *= slot_value(v, (codes >> (8 * f)) & 255u);
          cg[m] += (double)(rbar * prod);
        }
      }
    }
  }

  if (REDUCE) {
    __shared__ double red[256];
    const int rows = COEF ? 1 + p.n_terms : 1;
#pragma unroll
    for (int k = 0; k < kTermRow; ++k) {
      if (k < rows) {
        red[threadIdx.x] = k == 0 ? loss_acc : cg[COEF ? k - 1 : 0];
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
          if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
          __syncthreads();
        }
        if (threadIdx.x == 0) partial[blockIdx.x * kTermRow + k] = red[0];
        __syncthreads();
      }
    }
  }
}

// thread k < rows: sum k of the block partials in block order, in double, added to its output and rounded once
__global__ void term_finish_kernel(const double* partial, int blocks, int n_terms, float* loss_sum_out, float* coef_grads) {
  const int k = threadIdx.x;
  if (k > n_terms) return;
  float* out = k == 0 ? loss_sum_out : (coef_grads ? coef_grads + (k - 1) : nullptr);
  if (!out) return;
  double s = 0.0;
  for (int b = 0; b < blocks; ++b) s += partial[b * kTermRow + k];
  out[0] = (float)((double)out[0] + s);
}

// the stream sets the library has units for (csrc/Makefile: SETS)
bool term_set_compiled(int nt, int nx) {
  static const int sets[][2] = {{0, 0}, {1, 0}, {1, 1}, {1, 2}, {1, 3}, {1, 4}, {2, 0}, {2, 2}};
  for (const auto& s : sets)
    if (s[0] == nt && s[1] == nx) return true;
  return false;
}

}  // namespace

extern "C" int pinn_internal_fail(int code, const char* msg);  // pinn_abi.hip: sets pinn_last_error()

static int term_launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return PINN_OK;
  char msg[256];
  snprintf(msg, sizeof(msg), "HIP error %d: %s (%s)", (int)e, hipGetErrorString(e), what);
  return pinn_internal_fail(PINN_ERR_HIP, msg);
}

extern "C" int pinn_term_residual(const PinnTermPde* pde, const float* coef_values, const float* jets, const float* x,
                                  const float* t, int64_t N, float grad_scale, const float* residual_cotangent,
                                  float* residual_out, float* loss_sum_out, float* jet_cotangents, float* coef_grads,
                                  double* scratch, void* stream) {
  char msg[160];
  if (!pde) return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_term_residual: null descriptor");
  if (pde->n_terms < 0 || pde->n_terms > PINN_TERM_MAX_TERMS) {
    snprintf(msg, sizeof(msg), "pinn_term_residual: n_terms %d outside [0, %d]", (int)pde->n_terms, PINN_TERM_MAX_TERMS);
    return pinn_internal_fail(PINN_ERR_BAD_DESC, msg);
  }
  const int nt = pde->time_order, nx = pde->space_order;
  if (!term_set_compiled(nt, nx)) {
    snprintf(msg, sizeof(msg), "pinn_term_residual: stream set (nt=%d, nx=%d) is not compiled", nt, nx);
    return pinn_internal_fail(PINN_ERR_BAD_DESC, msg);
  }
  TermProg p;
  p.n_terms = pde->n_terms;
  p.nt = nt;
  p.nx = nx;
  p.loss = pde->loss;
  p.huber_delta = pde->huber_delta;
  p.uses_trig = 0;
  bool uses_x = false, uses_t = false;
  for (int m = 0; m < PINN_TERM_MAX_TERMS; ++m) {
    p.factors[m] = 0xffffffffu;
    p.n_factors[m] = 0;
  }
  for (int m = 0; m < pde->n_terms; ++m) {
    const PinnTermPdeTerm& tm = pde->terms[m];
    if (tm.n_factors < 0 || tm.n_factors > PINN_TERM_MAX_FACTORS) {
      snprintf(msg, sizeof(msg), "pinn_term_residual: term %d has n_factors %d outside [0, %d]", m, (int)tm.n_factors,
               PINN_TERM_MAX_FACTORS);
      return pinn_internal_fail(PINN_ERR_BAD_DESC, msg);
    }
    unsigned packed = 0xffffffffu;
    for (int f = 0; f < tm.n_factors; ++f) {
      const int code = tm.factor[f];
      if (code < 0 || code >= kSlots) {
        snprintf(msg, sizeof(msg), "pinn_term_residual: term %d, factor %d: unknown factor code %d", m, f, code);
        return pinn_internal_fail(PINN_ERR_BAD_DESC, msg);
      }
      if (code < kStreams && stream_of_code(code, nt, nx) < 0) {
        snprintf(msg, sizeof(msg), "pinn_term_residual: term %d, factor %d names a stream (code %d) that the set (nt=%d, nx=%d) does not hold",
                 m, f, code, nt, nx);
        return pinn_internal_fail(PINN_ERR_BAD_DESC, msg);
      }
      if (code == PINN_TERM_X) uses_x = true;
      if (code == PINN_TERM_T) uses_t = true;
      if (code == PINN_TERM_SIN_U || code == PINN_TERM_COS_U) p.uses_trig = 1;
      packed = (packed & ~(255u << (8 * f))) | ((unsigned)code << (8 * f));
    }
    p.factors[m] = packed;
    p.n_factors[m] = tm.n_factors;
  }
  if (N < 0) return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_term_residual: N < 0");
  if (N == 0) return PINN_OK;
  if (!jets || !coef_values) return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_term_residual: null jets or coef_values");
  if ((uses_x && !x) || (uses_t && !t))
    return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_term_residual: a term names X / T but the coordinate array is null");
  const bool reduce = loss_sum_out || coef_grads;
  if (reduce && !scratch) return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_term_residual: null scratch with a loss or coefficient sum");
  if (reinterpret_cast<uintptr_t>(scratch) & 7u)
    return pinn_internal_fail(PINN_ERR_MISALIGNED, "pinn_term_residual: scratch must be 8-byte aligned");

  long long nb = ((long long)N + 255) / 256;
  const int blocks = (int)(nb > kTermBlocks ? kTermBlocks : nb);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float* xs = uses_x ? x : nullptr;
  const float* ts = uses_t ? t : nullptr;
  if (!reduce) {
    hipLaunchKernelGGL((term_residual_kernel<false, false>), dim3(blocks), dim3(256), 0, st, p, coef_values, jets, xs, ts,
                       (long long)N, grad_scale, residual_cotangent, residual_out, jet_cotangents, scratch);
    return term_launched("term_residual_kernel");
  }
  if (coef_grads)
    hipLaunchKernelGGL((term_residual_kernel<true, true>), dim3(blocks), dim3(256), 0, st, p, coef_values, jets, xs, ts,
                       (long long)N, grad_scale, residual_cotangent, residual_out, jet_cotangents, scratch);
  else
    hipLaunchKernelGGL((term_residual_kernel<true, false>), dim3(blocks), dim3(256), 0, st, p, coef_values, jets, xs, ts,
                       (long long)N, grad_scale, residual_cotangent, residual_out, jet_cotangents, scratch);
  int rc = term_launched("term_residual_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(term_finish_kernel, dim3(1), dim3(64), 0, st, scratch, blocks, (int)p.n_terms, loss_sum_out, coef_grads);
  return term_launched("term_finish_kernel");
}
