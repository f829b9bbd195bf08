// Causal (time-weighted) residual loss (include/pinn_jet.h, "causal residual weights"): the middle of the chain
// pinn_residual_forward -> pinn_causal_weights -> pinn_residual_backward.  The time axis is cut into n_bins bins; the loss of a
// bin is weighted by exp(-eps * sum of the mean losses of the earlier bins), the weights detached.  Three launches:
//   1. a fixed grid of per-block, per-bin double sums of l(r) and counts,
//   2. one workgroup: the partials in block order, the serial prefix in double, the weights and the two loss sums,
//   3. the cotangents grad_scale * w_b(n) * l'(r_n), walked in quads like the smoothness kernels of train_kernels.hip.
// No atomics anywhere: every sum has an order fixed by the data and the grid, so two calls are bit-identical, and which
// thread sums which point does not depend on the alignment of the buffers.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/pinn_jet.h"

namespace {

constexpr int kCausalBlocks = 64;              // fixed grid of pass 1: the partials are summed in block order
constexpr int kMaxBins = PINN_CAUSAL_MAX_BINS;  // one LDS row per wave, one column per bin
constexpr int kWaves = 4;                      // 256 threads

static_assert(kMaxBins == 64, "one bin per lane of the finish pass");
static_assert(PINN_CAUSAL_SCRATCH_DOUBLES >= kCausalBlocks * kMaxBins * 2, "scratch size");

// b(n): one rounded fp32 operation each, never contracted into an FMA — bit-equal to torch's
// ((t - lo) * s).clamp(0, M - 1).to(int32) on fp32 tensors.  fmaxf / fminf drop a NaN, so the result is always in [0, M).
__device__ __forceinline__ int causal_bin(float t, float lo, float s, float top) {
  const float v = __fmul_rn(__fsub_rn(t, lo), s);
  return (int)fminf(fmaxf(v, 0.0f), top);
}

// l(r) in double from the fp32 residual (jet_device.h::loss_term's branches)
__device__ __forceinline__ double causal_loss(int kind, float d, float r) {
  const double x = (double)r;
  if (kind == PINN_LOSS_MAE) return fabs(x);
  if (kind == PINN_LOSS_HUBER) {
    const double a = fabs(x), dd = (double)d;
    return fabsf(r) < d ? 0.5 * x * x : dd * (a - 0.5 * dd);
  }
  return x * x;
}

// l'(r): exact in fp32 for all three kinds (sgn(0) = 0, Huber's quadratic branch on |r| < delta)
__device__ __forceinline__ float causal_dloss(int kind, float d, float r) {
  if (kind == PINN_LOSS_MAE) return r > 0.0f ? 1.0f : (r < 0.0f ? -1.0f : 0.0f);
  if (kind == PINN_LOSS_HUBER) return fabsf(r) < d ? r : (r > 0.0f ? d : -d);
  return 2.0f * r;
}

// Pass 1.  Block b takes points b * 256 + tid, + gridDim * 256, ...  Inside a wave the lanes are reduced bin by bin: the
// first unfinished lane names a bin, the lanes that hold it are summed by a fixed butterfly (the others add 0.0, which is
// exact), and lane 0 adds the total into the wave's LDS row.  One or two rounds for a time-ordered batch, at most 64; every
// branch is wave-uniform.  partial[(b * 64 + bin) * 2 + {0, 1}] = {sum l(r), count}.
__global__ __launch_bounds__(256) void causal_partial_kernel(const float* r, const float* t, long long n, int n_bins, float lo,
                                                             float s, int loss, float delta, double* partial) {
  __shared__ double wsum[kWaves][kMaxBins];
  __shared__ unsigned wcnt[kWaves][kMaxBins];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  wsum[wave][lane] = 0.0;
  wcnt[wave][lane] = 0u;
  __syncthreads();
  const float top = (float)(n_bins - 1);
  const long long stride = (long long)gridDim.x * 256;
  for (long long base = (long long)blockIdx.x * 256; base < n; base += stride) {  // block-uniform trip count
    const long long i = base + threadIdx.x;
    int b = -1;  // a lane past n matches no bin
    double l = 0.0;
    if (i < n) {
      b = causal_bin(t[i], lo, s, top);
      l = causal_loss(loss, delta, r[i]);
    }
    unsigned long long todo = __ballot(b >= 0);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int lb = __builtin_amdgcn_readlane(b, leader);
      const bool mine = b == lb;
      const unsigned long long mask = __ballot(mine);
      double v = mine ? l : 0.0;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
      if (lane == 0) {
        wsum[wave][lb] += v;
        wcnt[wave][lb] += (unsigned)__popcll(mask);
      }
      todo &= ~mask;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < n_bins) {  // the four wave rows in wave order
    const int bin = threadIdx.x;
    double sum = wsum[0][bin];
    unsigned cnt = wcnt[0][bin];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) sum += wsum[w][bin], cnt += wcnt[w][bin];
    double* out = partial + ((long long)blockIdx.x * kMaxBins + bin) * 2;
    out[0] = sum;
    out[1] = (double)cnt;
  }
}

// Pass 2, one workgroup of 64: lane i adds bin i's partials in block order and takes L_i = S_i / c_i (0 for an empty bin);
// lane 0 walks the serial prefix in double; every lane takes its w_i = (float)exp(-eps * sum_{k<i} L_k) (the exponentials side
// by side, not one after the other); lane 0 adds the two loss sums in bin order, each rounded once.
__global__ __launch_bounds__(64) void causal_finish_kernel(const double* partial, int blocks, int n_bins, const float* eps_dev,
                                                           float* bin_losses, float* bin_weights, float* loss_sum_out,
                                                           float* plain_sum_out) {
  __shared__ double S[kMaxBins], P[kMaxBins];
  __shared__ float W[kMaxBins];
  const int bin = threadIdx.x;
  double L = 0.0;
  if (bin < n_bins) {
    double sum = 0.0, cnt = 0.0;
    for (int b0 = 0; b0 < blocks; b0 += 16) {  // 16 blocks' loads in flight at once, added in block order (an absent block adds 0.0)
      double s[16], c[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const double* in = partial + ((long long)(b0 + j) * kMaxBins + bin) * 2;
        s[j] = b0 + j < blocks ? in[0] : 0.0;
        c[j] = b0 + j < blocks ? in[1] : 0.0;
      }
#pragma unroll
      for (int j = 0; j < 16; ++j) sum += s[j], cnt += c[j];
    }
    L = cnt > 0.0 ? sum / cnt : 0.0;
    S[bin] = sum;
    P[bin] = L;
  }
  __syncthreads();
  if (threadIdx.x == 0) {  // exclusive prefix, in place
    double prefix = 0.0;
    for (int i = 0; i < n_bins; ++i) {
      const double l = P[i];
      P[i] = prefix;
      prefix += l;
    }
  }
  __syncthreads();
  if (bin < n_bins) {
    const float w = (float)exp(-(double)eps_dev[0] * P[bin]);
    W[bin] = w;
    bin_weights[bin] = w;
    if (bin_losses) bin_losses[bin] = (float)L;
  }
  __syncthreads();
  if (threadIdx.x == 0 && (loss_sum_out || plain_sum_out)) {
    double weighted = 0.0, plain = 0.0;
    for (int i = 0; i < n_bins; ++i) {
      weighted += (double)W[i] * S[i];
      plain += S[i];
    }
    if (loss_sum_out) loss_sum_out[0] += (float)weighted;
    if (plain_sum_out) plain_sum_out[0] += (float)plain;
  }
}

__device__ __forceinline__ void causal_load4(const float* p, long long i, long long n, bool vec, float v[4]) {
  if (vec && i + 4 <= n) {
    const float4 q = *reinterpret_cast<const float4*>(p + i);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = i + j < n ? p[i + j] : 0.0f;
  }
}

// Pass 3.  al: bit 0 r, bit 1 t, bit 2 cot — set where 16-byte aligned.
__global__ __launch_bounds__(256) void causal_cotangent_kernel(const float* r, const float* t, long long n, int n_bins, float lo,
                                                               float s, int loss, float delta, float grad_scale,
                                                               const float* bin_weights, float* cot, int al) {
  __shared__ float gw[kMaxBins];  // grad_scale * w_i
  if ((int)threadIdx.x < n_bins) gw[threadIdx.x] = __fmul_rn(grad_scale, bin_weights[threadIdx.x]);
  __syncthreads();
  const float top = (float)(n_bins - 1);
  const long long nq = (n + 3) >> 2;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long long)gridDim.x * 256) {
    const long long i = q << 2;
    float rc[4], tc[4], c[4];
    causal_load4(r, i, n, al & 1, rc);
    causal_load4(t, i, n, al & 2, tc);
#pragma unroll
    for (int j = 0; j < 4; ++j)  // lanes past n were loaded as 0: bin in range, not stored
      c[j] = __fmul_rn(gw[causal_bin(tc[j], lo, s, top)], causal_dloss(loss, delta, rc[j]));
    if ((al & 4) && i + 4 <= n) {
      *reinterpret_cast<float4*>(cot + i) = make_float4(c[0], c[1], c[2], c[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i + j < n) cot[i + j] = c[j];
    }
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

extern "C" int pinn_causal_weights(const float* residual, const float* t, int64_t N, int32_t n_bins, double t_lo, double t_hi,
                                   const float* eps_dev, int32_t loss, float huber_delta, float grad_scale, float* cotangent,
                                   float* loss_sum_out, float* plain_sum_out, float* bin_losses, float* bin_weights,
                                   double* scratch, void* stream) {
  if (n_bins < 1 || n_bins > PINN_CAUSAL_MAX_BINS)
    return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_causal_weights: n_bins outside [1, PINN_CAUSAL_MAX_BINS]");
  if (!std::isfinite(t_lo) || !std::isfinite(t_hi) || !(t_hi > t_lo))
    return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_causal_weights: the time domain needs finite bounds with t_hi > t_lo");
  if (loss != PINN_LOSS_MSE && loss != PINN_LOSS_MAE && loss != PINN_LOSS_HUBER)
    return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_causal_weights: unknown loss kind");
  if (N < 0) return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_causal_weights: N < 0");
  if (N == 0) return PINN_OK;
  if (!residual || !t || !eps_dev || !cotangent || !bin_weights || !scratch)
    return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_causal_weights: null argument");
  if (reinterpret_cast<uintptr_t>(scratch) & 7u)
    return pinn_internal_fail(PINN_ERR_MISALIGNED, "pinn_causal_weights: scratch must be 8-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float lo = (float)t_lo, s = (float)((double)n_bins / (t_hi - t_lo));
  const long long n = (long long)N;
  int blocks = (int)((n + 255) / 256 > kCausalBlocks ? kCausalBlocks : (n + 255) / 256);
  hipLaunchKernelGGL(causal_partial_kernel, dim3(blocks), dim3(256), 0, st, residual, t, n, n_bins, lo, s, loss, huber_delta, scratch);
  int rc = launched("causal_partial_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(causal_finish_kernel, dim3(1), dim3(64), 0, st, scratch, blocks, n_bins, eps_dev, bin_losses, bin_weights,
                     loss_sum_out, plain_sum_out);
  if ((rc = launched("causal_finish_kernel"))) return rc;
  auto al = [](const float* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
  const int bits = (al(residual) ? 1 : 0) | (al(t) ? 2 : 0) | (al(cotangent) ? 4 : 0);
  const long long nq = (n + 3) >> 2;
  int cblocks = (int)((nq + 255) / 256 > 1024 ? 1024 : (nq + 255) / 256);
  hipLaunchKernelGGL(causal_cotangent_kernel, dim3(cblocks), dim3(256), 0, st, residual, t, n, n_bins, lo, s, loss, huber_delta,
                     grad_scale, bin_weights, cotangent, bits);
  return launched("causal_cotangent_kernel");
}
