// Per-face boundary conditions (include/pinn_jet.h, "face loss terms"): pinn_face_losses, the loss-term call of a boundary /
// initial chain whose terms combine a value segment and a derivative segment of the jets,
//   d_i = alpha (A[i] - A'[i]) + beta (B[i] - B'[i]) - T_i,
// for up to PINN_FACE_MAX_TERMS terms.  Two launches:
//   1. a fixed grid of at most 64 blocks x 256 threads: the term loop is wave-uniform, the points of a term are strided over
//      the whole grid, every named cotangent float is written once, per-block per-term sums of l(d) in double,
//   2. one workgroup: the partials in block order, the means, the summary.
// No atomics: every sum has an order fixed by the term lengths and the grid, and which thread takes which point does not
// depend on the alignment of any segment (4-byte accesses throughout), so two calls are bit-identical.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/pinn_jet.h"

namespace {

constexpr int kFaceBlocks = 64;  // fixed upper bound of the grid of pass 1: the partials are summed in block order
constexpr int kMaxTerms = PINN_FACE_MAX_TERMS;
constexpr int kWaves = 4;  // 256 threads

static_assert(PINN_FACE_SCRATCH_DOUBLES >= kFaceBlocks * kMaxTerms, "scratch size");
static_assert(kMaxTerms <= 64, "one term per lane of the finish pass");

struct FaceTable {  // the host table, by value in the kernel arguments (16 + 32 * 48 bytes)
  int n_terms, loss;
  float huber_delta;
  int pad;
  PinnFaceTerm t[kMaxTerms];
};

// l(d) in double from the fp32 difference (jet_device.h::loss_term's branches)
__device__ __forceinline__ double face_loss(int kind, float delta, float d) {
  const double x = (double)d;
  if (kind == PINN_LOSS_MAE) return fabs(x);
  if (kind == PINN_LOSS_HUBER) {
    const double dd = (double)delta;
    return fabsf(d) < delta ? 0.5 * x * x : dd * (fabs(x) - 0.5 * dd);
  }
  return x * x;
}

// l'(d): exact in fp32 for all three kinds (sgn(0) = 0, Huber's quadratic branch on |d| < delta)
__device__ __forceinline__ float face_dloss(int kind, float delta, float d) {
  if (kind == PINN_LOSS_MAE) return d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
  if (kind == PINN_LOSS_HUBER) return fabsf(d) < delta ? d : (d > 0.0f ? delta : -delta);
  return 2.0f * d;
}

// Pass 1.  Block b takes points b * 256 + tid, + gridDim * 256, ... of every term.  partial[b * 32 + k] = this block's sum
// of l(d) over term k: the lanes of a wave by a fixed butterfly, the four wave sums in wave order.
__global__ __launch_bounds__(256) void face_partial_kernel(const float* __restrict__ J, float* __restrict__ cot, FaceTable p,
                                                           double* __restrict__ partial) {
  __shared__ double wsum[kMaxTerms][kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long first = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
  for (int k = 0; k < p.n_terms; ++k) {  // wave-uniform: the table is in the kernel arguments
    const int n = p.t[k].n, va = p.t[k].value, vp = p.t[k].value_pair, da = p.t[k].deriv, dp = p.t[k].deriv_pair;
    const float alpha = p.t[k].alpha, beta = p.t[k].beta, tc = p.t[k].target_const;
    const float* __restrict__ tg = p.t[k].target;
    const float s = __fdiv_rn(p.t[k].weight, (float)n);
    const float sa = __fmul_rn(s, alpha), sb = __fmul_rn(s, beta);
    double acc = 0.0;
    for (long long i = first; i < n; i += stride) {
      float d = -(tg ? tg[i] : tc);
      if (va >= 0) {
        float a = J[va + i];
        if (vp >= 0) a = __fsub_rn(a, J[vp + i]);
        d = __fmaf_rn(alpha, a, d);
      }
      if (da >= 0) {
        float b = J[da + i];
        if (dp >= 0) b = __fsub_rn(b, J[dp + i]);
        d = __fmaf_rn(beta, b, d);
      }
      acc += face_loss(p.loss, p.huber_delta, d);
      const float dl = face_dloss(p.loss, p.huber_delta, d);
      if (va >= 0) {
        const float c = __fmul_rn(sa, dl);
        cot[va + i] = c;
        if (vp >= 0) cot[vp + i] = -c;
      }
      if (da >= 0) {
        const float c = __fmul_rn(sb, dl);
        cot[da + i] = c;
        if (dp >= 0) cot[dp + i] = -c;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) wsum[k][wave] = acc;
  }
  __syncthreads();
  if ((int)threadIdx.x < p.n_terms) {
    const int k = threadIdx.x;
    partial[(long long)blockIdx.x * kMaxTerms + k] = ((wsum[k][0] + wsum[k][1]) + wsum[k][2]) + wsum[k][3];
  }
}

struct FaceMeans {  // what the finish pass needs of the table
  int n_terms;
  int n[kMaxTerms];
  float weight[kMaxTerms];
};

// Pass 2, one workgroup of 64: lane k adds term k's partials in block order; lane 0 takes the means in double, each rounded
// once, and writes {residual, boundary, initial, total}, double sums of the rounded means in term order, each rounded once.
__global__ __launch_bounds__(64) void face_finish_kernel(const double* __restrict__ partial, int blocks, FaceMeans m,
                                                         float* __restrict__ losses, const float* residual_sum,
                                                         float residual_scale, float residual_weight, int n_boundary_terms,
                                                         float* summary4) {
  __shared__ double S[kMaxTerms];
  if ((int)threadIdx.x < m.n_terms) {
    double sum = 0.0;
    for (int b0 = 0; b0 < blocks; b0 += 16) {  // 16 blocks' loads in flight at once, added in block order (an absent block adds 0.0)
      double s[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) s[j] = b0 + j < blocks ? partial[(long long)(b0 + j) * kMaxTerms + threadIdx.x] : 0.0;
#pragma unroll
      for (int j = 0; j < 16; ++j) sum += s[j];
    }
    S[threadIdx.x] = sum;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const float res = residual_sum ? __fmul_rn(residual_sum[0], residual_scale) : 0.0f;
  double bnd = 0.0, ini = 0.0, tot = (double)residual_weight * (double)res;
  for (int k = 0; k < m.n_terms; ++k) {  // uniform reads of the table
    const float l = (float)(S[k] / (double)m.n[k]);
    losses[k] = l;
    if (k < n_boundary_terms) bnd += (double)l;
    else ini += (double)l;
    tot += (double)m.weight[k] * (double)l;
  }
  if (summary4) {
    summary4[0] = res;
    summary4[1] = (float)bnd;
    summary4[2] = (float)ini;
    summary4[3] = (float)tot;
  }
}

}  // namespace

extern "C" int pinn_internal_fail(int code, const char* msg);  // pinn_abi.hip: sets pinn_last_error()

static int launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return PINN_OK;
  char msg[256];
  snprintf(msg, sizeof(msg), "HIP error %d: %s (%s)", (int)e, hipGetErrorString(e), what);
  return pinn_internal_fail(PINN_ERR_HIP, msg);
}

extern "C" int pinn_face_losses(const float* jets, float* cotangent, int64_t n_floats, int32_t n_terms, const PinnFaceTerm* terms,
                                int32_t loss, float huber_delta, float* term_losses, const float* residual_sum,
                                float residual_scale, float residual_weight, int32_t n_boundary_terms, float* summary4,
                                double* scratch, void* stream) {
  if (n_terms < 0 || n_terms > PINN_FACE_MAX_TERMS)
    return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_face_losses: n_terms outside [0, PINN_FACE_MAX_TERMS]");
  if (loss != PINN_LOSS_MSE && loss != PINN_LOSS_MAE && loss != PINN_LOSS_HUBER)
    return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_face_losses: unknown loss kind");
  if (n_floats < 0) return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_face_losses: n_floats < 0");
  if (n_terms > 0 && (!jets || !cotangent || !terms || !term_losses || !scratch))
    return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_face_losses: null argument");
  if (n_terms > 0 && (reinterpret_cast<uintptr_t>(scratch) & 7u))
    return pinn_internal_fail(PINN_ERR_MISALIGNED, "pinn_face_losses: scratch must be 8-byte aligned");
  FaceTable p;
  FaceMeans m;
  p.n_terms = m.n_terms = n_terms;
  p.loss = loss;
  p.huber_delta = huber_delta;
  p.pad = 0;
  struct Range {
    int64_t lo, hi;
  };
  Range ranges[4 * PINN_FACE_MAX_TERMS];
  int n_ranges = 0, n_max = 0;
  for (int k = 0; k < n_terms; ++k) {
    const PinnFaceTerm& t = terms[k];
    if (t.n < 1) return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_face_losses: a term needs n >= 1");
    const int32_t off[4] = {t.value, t.value_pair, t.deriv, t.deriv_pair};
    for (int j = 0; j < 4; ++j) {
      if (off[j] == -1) continue;
      if (off[j] < 0 || (int64_t)off[j] + t.n > n_floats)
        return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_face_losses: a segment leaves the buffer");
      ranges[n_ranges].lo = off[j];
      ranges[n_ranges++].hi = (int64_t)off[j] + t.n;
    }
    if ((t.value >= 0) != (t.alpha != 0.0f))
      return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_face_losses: alpha != 0 goes with a value segment, alpha == 0 with none");
    if ((t.deriv >= 0) != (t.beta != 0.0f))
      return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_face_losses: beta != 0 goes with a derivative segment, beta == 0 with none");
    if ((t.value_pair >= 0 && t.value < 0) || (t.deriv_pair >= 0 && t.deriv < 0))
      return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_face_losses: a partner segment without its primary");
    p.t[k] = t;
    m.n[k] = t.n;
    m.weight[k] = t.weight;
    n_max = std::max(n_max, (int)t.n);
  }
  std::sort(ranges, ranges + n_ranges, [](const Range& a, const Range& b) { return a.lo < b.lo; });
  for (int j = 1; j < n_ranges; ++j)
    if (ranges[j].lo < ranges[j - 1].hi) return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_face_losses: two segments overlap");
  for (int k = n_terms; k < PINN_FACE_MAX_TERMS; ++k) {
    p.t[k] = PinnFaceTerm{-1, -1, -1, -1, 0, 0.0f, 0.0f, 0.0f, 0.0f, nullptr};
    m.n[k] = 0;
    m.weight[k] = 0.0f;
  }
  if (n_terms == 0 && !summary4) return PINN_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int blocks = std::min(kFaceBlocks, (n_max + 255) / 256);
  if (n_terms > 0) {
    hipLaunchKernelGGL(face_partial_kernel, dim3(blocks), dim3(256), 0, st, jets, cotangent, p, scratch);
    const int rc = launched("face_partial_kernel");
    if (rc) return rc;
  }
  hipLaunchKernelGGL(face_finish_kernel, dim3(1), dim3(64), 0, st, scratch, blocks, m, term_losses, residual_sum, residual_scale,
                     residual_weight, n_boundary_terms, summary4);
  return launched("face_finish_kernel");
}
