// Small kernels of the captured training step (include/pinn_jet.h, "training step" section): the point-wise loss
// terms of PDEBase.compute_loss on the boundary / initial points, and gradient clipping + Adam over ONE flat
// parameter buffer.  Everything else of a step is the jet engine's residual launch; with these two the whole step is
// free of autograd and runs as a handful of launches inside a HIP graph.  With adaptive loss weights (RBW / LRW) the last
// part is pinn_adaptive_adam_step instead: weight update + weighted combination of the component gradients + clip + Adam.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/pinn_jet.h"

namespace {

struct PointTerms {
  int n_terms;
  int lo[PINN_MAX_POINT_TERMS], hi[PINN_MAX_POINT_TERMS];
  const float* target[PINN_MAX_POINT_TERMS];
  float weight[PINN_MAX_POINT_TERMS];
  int loss;
  float huber_delta;
};

__device__ __forceinline__ float loss_val(int kind, float d, float r, float* dl) {
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

// one workgroup; term k: losses[k] = mean_{n in [lo,hi)} l(u[n] - target_k[n]); cot[n] += weight_k l'(.) / (hi - lo)
__global__ __launch_bounds__(256) void point_loss_kernel(const float* u, PointTerms p, int n_total, float* losses, float* cot,
                                                         const float* residual_sum, float residual_scale, float residual_weight,
                                                         int n_boundary_terms, float* summary4) {
  __shared__ float red[256];
  const int tid = threadIdx.x;
  for (int n = tid; n < n_total; n += 256) cot[n] = 0.0f;
  __syncthreads();
  for (int k = 0; k < p.n_terms; ++k) {
    const int cnt = p.hi[k] - p.lo[k];
    const float inv = cnt > 0 ? 1.0f / (float)cnt : 0.0f;
    float acc = 0.0f;
    for (int n = p.lo[k] + tid; n < p.hi[k]; n += 256) {
      float dl;
      acc += loss_val(p.loss, p.huber_delta, u[n] - p.target[k][n - p.lo[k]], &dl);
      cot[n] += p.weight[k] * dl * inv;  // terms are processed one after another: no two threads share n within a term
    }
    red[tid] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s) red[tid] += red[tid + s];
      __syncthreads();
    }
    if (tid == 0) losses[k] = red[0] * inv;
    __syncthreads();
  }
  if (tid == 0 && summary4) {  // {residual, boundary, initial, total} of PDEBase.compute_loss (pde_base.py:1168-1235)
    const float res = residual_sum ? residual_sum[0] * residual_scale : 0.0f;
    float bnd = 0.0f, ini = 0.0f, tot = residual_weight * res;
    for (int k = 0; k < p.n_terms; ++k) {
      if (k < n_boundary_terms) bnd += losses[k];
      else ini += losses[k];
      tot += p.weight[k] * losses[k];
    }
    summary4[0] = res;
    summary4[1] = bnd;
    summary4[2] = ini;
    summary4[3] = tot;
  }
}

// The general form: jets J[stream][n] (K x n_total), term k on stream `stream[k]`, either against a target array or —
// pair[k] != 0 — as the difference of two point ranges, d_i = J[s][lo + i] - J[s][lo + pair + i] (periodic boundary
// conditions: value and d/dx at paired wall points, heat_equation.py:420-445).  cot is K x n_total, overwritten.
struct JetTerms {
  int n_terms;
  int lo[PINN_MAX_POINT_TERMS], hi[PINN_MAX_POINT_TERMS], stream[PINN_MAX_POINT_TERMS], pair[PINN_MAX_POINT_TERMS];
  const float* target[PINN_MAX_POINT_TERMS];
  float weight[PINN_MAX_POINT_TERMS];
  int loss;
  float huber_delta;
};

__global__ __launch_bounds__(256) void jet_loss_kernel(const float* J, int K, JetTerms p, int n_total, float* losses, float* cot,
                                                       const float* residual_sum, float residual_scale, float residual_weight,
                                                       int n_boundary_terms, float* summary4) {
  __shared__ float red[256];
  const int tid = threadIdx.x;
  for (int n = tid; n < K * n_total; n += 256) cot[n] = 0.0f;
  __syncthreads();
  for (int k = 0; k < p.n_terms; ++k) {
    const int cnt = p.hi[k] - p.lo[k];
    const float inv = cnt > 0 ? 1.0f / (float)cnt : 0.0f;
    const float* Js = J + (long long)p.stream[k] * n_total;
    float* cs = cot + (long long)p.stream[k] * n_total;
    float acc = 0.0f;
    for (int n = p.lo[k] + tid; n < p.hi[k]; n += 256) {
      float dl;
      const float other = p.pair[k] ? Js[n + p.pair[k]] : p.target[k][n - p.lo[k]];
      acc += loss_val(p.loss, p.huber_delta, Js[n] - other, &dl);
      const float c = p.weight[k] * dl * inv;
      cs[n] += c;  // terms run one after another and a term's two ranges are disjoint: no two threads share an address
      if (p.pair[k]) cs[n + p.pair[k]] -= c;
    }
    red[tid] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s) red[tid] += red[tid + s];
      __syncthreads();
    }
    if (tid == 0) losses[k] = red[0] * inv;
    __syncthreads();
  }
  if (tid == 0 && summary4) {
    const float res = residual_sum ? residual_sum[0] * residual_scale : 0.0f;
    float bnd = 0.0f, ini = 0.0f, tot = residual_weight * res;
    for (int k = 0; k < p.n_terms; ++k) {
      if (k < n_boundary_terms) bnd += losses[k];
      else ini += losses[k];
      tot += p.weight[k] * losses[k];
    }
    summary4[0] = res;
    summary4[1] = bnd;
    summary4[2] = ini;
    summary4[3] = tot;
  }
}

constexpr int kNormBlocks = 64;

// 1 - beta^t of Adam's bias corrections (torch forms them in double).  `1.0f - powf(beta, t)` cancels at small t
// (1 - 0.999^2 keeps 14 of its 24 bits), which put an error of about 1e-6 into every early update; expm1f does not.
__device__ __forceinline__ float bias_correction(float beta, float t) { return -expm1f(t * logf(beta)); }

// partial sums of squares in a fixed order (deterministic): block b sums elements b*256+tid, +64*256, ...
__global__ __launch_bounds__(256) void sumsq_kernel(const float* g, long long n, float* partial) {
  __shared__ float red[256];
  float acc = 0.0f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)kNormBlocks * 256) acc = fmaf(g[i], g[i], acc);
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// torch.nn.utils.clip_grad_norm_(max_norm) followed by torch.optim.Adam(lr, betas, eps, weight_decay).step()
// (pinnrl/training/trainer.py:686-698) over one flat buffer.  `step` holds the number of steps taken so far.
__global__ __launch_bounds__(256) void adam_kernel(float* p, const float* g, float* m, float* v, long long n, const float* lr,
                                                   float beta1, float beta2, float eps, float wd, float max_norm,
                                                   float* step, const float* partial, float* norm_out) {
  float tot = 0.0f;
  for (int i = 0; i < kNormBlocks; ++i) tot += partial[i];  // every thread, same order
  const float norm = sqrtf(tot);
  float coef = 1.0f;
  if (max_norm > 0.0f) {
    coef = max_norm / (norm + 1e-6f);
    coef = coef < 1.0f ? coef : 1.0f;
  }
  const float t = step[0] + 1.0f;
  const float bc1 = bias_correction(beta1, t), bc2 = bias_correction(beta2, t);
  const float step_size = lr[0] / bc1, rs2 = rsqrtf(bc2);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    float gi = g[i] * coef;
    const float pi = p[i];
    if (wd != 0.0f) gi = fmaf(wd, pi, gi);
    const float mi = fmaf(1.0f - beta1, gi - m[i], m[i]);           // torch: m.lerp_(g, 1 - beta1)
    const float vi = fmaf(beta2, v[i], (1.0f - beta2) * gi * gi);   // torch: v.mul_(beta2).addcmul_(g, g, 1 - beta2)
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) * rs2 + eps;
    p[i] = pi - step_size * (mi / denom);
  }
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x == 0 && norm_out) norm_out[0] = norm;
}

__global__ void step_inc_kernel(float* step) { step[0] += 1.0f; }

// ---- adaptive loss weights (pinnrl/components/adaptive_weights.py:35-107, pinnrl/training/trainer.py:586-684) ----------------
// The weights are detached numbers, so grad(total) = sum_c w_c grad(L_c): from the C component gradients one Gram pass gives
// every norm the step needs (LRW's per-component norms on its diagonal, the clip norm of the combined gradient as the
// quadratic form w^T G w), one workgroup runs the EMA rule, and the update pass combines, clips and applies Adam without the
// combined gradient ever going through memory.
constexpr int kMaxComp = 4, kMaxPairs = kMaxComp * (kMaxComp + 1) / 2;
// res[] (after the Gram partials in the scratch): what the update pass reads — written by the one-workgroup launch only
enum { kResW = 0, kResCoef = 4, kResStepSize = 5, kResRs2 = 6, kResFloats = 8 };

struct CompLosses {
  const float* ptr[kMaxComp];
  float scale[kMaxComp];
  float init[kMaxComp];
};

// partial[pair * kNormBlocks + block] = this block's share of <g_a, g_b>, pairs in the order (0,0) (0,1) .. (1,1) ..;
// products of two floats are exact in double, and every sum runs in a fixed order: deterministic.
// vec: rows are 16-byte aligned (base and ld): float4 loads over n / 4 vectors, the last n % 4 elements by block 0.
template <int C>
__global__ __launch_bounds__(256) void gram_kernel(const float* g, long long ld, long long n, int vec, double* partial) {
  constexpr int NP = C * (C + 1) / 2;
  __shared__ double red[256];
  double acc[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) acc[p] = 0.0;
  const long long first = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)kNormBlocks * 256;
  auto add = [&](const float* e) {
    int p = 0;
#pragma unroll
    for (int a = 0; a < C; ++a)
#pragma unroll
      for (int b = a; b < C; ++b, ++p) acc[p] = fma((double)e[a], (double)e[b], acc[p]);
  };
  if (vec) {
    const long long nv = n >> 2;
    for (long long i = first; i < nv; i += stride) {
      float4 q[C];
#pragma unroll
      for (int c = 0; c < C; ++c) q[c] = reinterpret_cast<const float4*>(g + c * ld)[i];
      float e[C];
#pragma unroll
      for (int c = 0; c < C; ++c) e[c] = q[c].x;
      add(e);
#pragma unroll
      for (int c = 0; c < C; ++c) e[c] = q[c].y;
      add(e);
#pragma unroll
      for (int c = 0; c < C; ++c) e[c] = q[c].z;
      add(e);
#pragma unroll
      for (int c = 0; c < C; ++c) e[c] = q[c].w;
      add(e);
    }
    const long long i = (nv << 2) + threadIdx.x;  // scalar tail
    if (blockIdx.x == 0 && threadIdx.x < 4 && i < n) {
      float e[C];
#pragma unroll
      for (int c = 0; c < C; ++c) e[c] = g[c * ld + i];
      add(e);
    }
  } else {
    for (long long i = first; i < n; i += stride) {
      float e[C];
#pragma unroll
      for (int c = 0; c < C; ++c) e[c] = g[c * ld + i];
      add(e);
    }
  }
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    red[threadIdx.x] = acc[p];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) partial[p * kNormBlocks + blockIdx.x] = red[0];
    __syncthreads();
  }
}

// One workgroup: the only launch that writes the weight state.  state16 = {running[4], prev_weights[4], weights[4], calls,
// has_prev, -, -}.  Also the scalars of the Adam update (as adam_kernel forms them) and the step counter's increment: the
// update pass reads res[] and never `step`, so no block of it depends on what another block writes.
__global__ __launch_bounds__(64) void adaptive_update_kernel(const double* partial, CompLosses cl, int C, int strategy, double alpha,
                                                             double aw_eps, int has_init, float* state, float* weights_out,
                                                             float* summary4, float max_norm, const float* lr, float beta1,
                                                             float beta2, float* step, float* res, float* norm_out) {
  __shared__ double G[kMaxPairs];
  const int NP = C * (C + 1) / 2;
  if ((int)threadIdx.x < NP) {
    double tot = 0.0;
    for (int b = 0; b < kNormBlocks; ++b) tot += partial[threadIdx.x * kNormBlocks + b];
    G[threadIdx.x] = tot;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double L[kMaxComp], v[kMaxComp], run[kMaxComp], w[kMaxComp];
  int diag = 0;
  for (int c = 0; c < C; ++c) {
    L[c] = (double)(cl.ptr[c][0] * cl.scale[c]);
    v[c] = strategy == 1 ? sqrt(G[diag]) : L[c];
    diag += C - c;
  }
  const bool first = state[12] == 0.0f;
  bool has_prev = state[13] != 0.0f;
  if (first) {
    for (int c = 0; c < C; ++c) {
      run[c] = v[c];
      w[c] = has_init ? (double)cl.init[c] : 1.0;
    }
  } else {
    double sum = 0.0;
    for (int c = 0; c < C; ++c) {
      run[c] = alpha * (double)state[c] + (1.0 - alpha) * v[c];
      sum += strategy == 1 ? 1.0 / (run[c] + aw_eps) : run[c];
    }
    for (int c = 0; c < C; ++c) {
      if (strategy == 1) {
        w[c] = (1.0 / (run[c] + aw_eps)) / sum;
      } else {
        w[c] = run[c] / (sum + aw_eps);
        if (has_prev) w[c] = alpha * (double)state[4 + c] + (1.0 - alpha) * w[c];
      }
    }
    if (strategy != 1) has_prev = true;
  }
  float wf[kMaxComp];
  double total = 0.0;
  for (int c = 0; c < kMaxComp; ++c) {
    wf[c] = c < C ? (float)w[c] : 0.0f;
    state[c] = c < C ? (float)run[c] : 0.0f;
    if (!first && strategy != 1) state[4 + c] = wf[c];
    state[8 + c] = wf[c];
    res[kResW + c] = wf[c];
    if (weights_out) weights_out[c] = wf[c];
    if (c < C) total += (double)wf[c] * L[c];
  }
  state[12] += 1.0f;
  state[13] = has_prev ? 1.0f : 0.0f;
  if (summary4) {
    for (int c = 0; c < 3; ++c) summary4[c] = c < C ? (float)L[c] : 0.0f;
    summary4[3] = (float)total;
  }
  // the norm clip_grad_norm_ would take of sum_c w_c g_c, as the quadratic form of the Gram matrix, in double: where two
  // component gradients nearly cancel the terms are orders of magnitude above their sum
  double q = 0.0;
  int p = 0;
  for (int a = 0; a < C; ++a)
    for (int b = a; b < C; ++b, ++p) q += (a == b ? 1.0 : 2.0) * (double)wf[a] * (double)wf[b] * G[p];
  const float norm = (float)sqrt(q > 0.0 ? q : 0.0);
  float coef = 1.0f;
  if (max_norm > 0.0f) {
    coef = max_norm / (norm + 1e-6f);
    coef = coef < 1.0f ? coef : 1.0f;
  }
  const float t = step[0] + 1.0f;
  const float bc1 = bias_correction(beta1, t), bc2 = bias_correction(beta2, t);
  res[kResCoef] = coef;
  res[kResStepSize] = lr[0] / bc1;
  res[kResRs2] = rsqrtf(bc2);
  step[0] = t;
  if (norm_out) norm_out[0] = norm;
}

struct AdamScalars {
  float w[kMaxComp], coef, step_size, rs2, beta1, beta2, eps, wd;
};

// g = sum_c w_c g_c in a fixed order, then the arithmetic of adam_kernel on one element
template <int C>
__device__ __forceinline__ void adaptive_adam_elem(const AdamScalars& s, const float* gc, float& p, float& m, float& v, float& g) {
  g = s.w[0] * gc[0];
#pragma unroll
  for (int c = 1; c < C; ++c) g = fmaf(s.w[c], gc[c], g);
  float gi = g * s.coef;
  const float pi = p;
  if (s.wd != 0.0f) gi = fmaf(s.wd, pi, gi);
  const float mi = fmaf(1.0f - s.beta1, gi - m, m);
  const float vi = fmaf(s.beta2, v, (1.0f - s.beta2) * gi * gi);
  m = mi;
  v = vi;
  const float denom = sqrtf(vi) * s.rs2 + s.eps;
  p = pi - s.step_size * (mi / denom);
}

template <int C>
__global__ __launch_bounds__(256) void adaptive_adam_kernel(float* p, const float* g, long long ld, float* m, float* v, long long n,
                                                            int vec, const float* res, float beta1, float beta2, float eps, float wd,
                                                            float* grad_out) {
  AdamScalars s;
#pragma unroll
  for (int c = 0; c < kMaxComp; ++c) s.w[c] = res[kResW + c];
  s.coef = res[kResCoef];
  s.step_size = res[kResStepSize];
  s.rs2 = res[kResRs2];
  s.beta1 = beta1, s.beta2 = beta2, s.eps = eps, s.wd = wd;
  const long long first = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
  const long long nv = vec ? n >> 2 : 0;
  for (long long i = first; i < nv; i += stride) {
    float4 q[C];
#pragma unroll
    for (int c = 0; c < C; ++c) q[c] = reinterpret_cast<const float4*>(g + c * ld)[i];
    float4 pp = reinterpret_cast<float4*>(p)[i], mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i], gg;
    float e[C];
#pragma unroll
    for (int c = 0; c < C; ++c) e[c] = q[c].x;
    adaptive_adam_elem<C>(s, e, pp.x, mm.x, vv.x, gg.x);
#pragma unroll
    for (int c = 0; c < C; ++c) e[c] = q[c].y;
    adaptive_adam_elem<C>(s, e, pp.y, mm.y, vv.y, gg.y);
#pragma unroll
    for (int c = 0; c < C; ++c) e[c] = q[c].z;
    adaptive_adam_elem<C>(s, e, pp.z, mm.z, vv.z, gg.z);
#pragma unroll
    for (int c = 0; c < C; ++c) e[c] = q[c].w;
    adaptive_adam_elem<C>(s, e, pp.w, mm.w, vv.w, gg.w);
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
    if (grad_out) reinterpret_cast<float4*>(grad_out)[i] = gg;
  }
  for (long long i = (nv << 2) + first; i < n; i += stride) {  // the scalar tail (everything when the rows are not aligned)
    float e[C], gi;
#pragma unroll
    for (int c = 0; c < C; ++c) e[c] = g[c * ld + i];
    adaptive_adam_elem<C>(s, e, p[i], m[i], v[i], gi);
    if (grad_out) grad_out[i] = gi;
  }
}

// ---- finite-difference smoothness term (pinnrl/pdes/heat_equation.py:625-650) -------------------------------------------------
// S = mean|(u(x+e,t) - u(x,t))/e| + mean|(u(x,t) - u(x-e,t))/e| over the collocation batch, shifted points clamped to the
// domain: the stencil kernel writes the 3N evaluation points [x | x+e | x-e], pinn_jet_forward (orders 0, 0) evaluates them,
// and one pass over the values gives the partial sums and the cotangents of the reverse sweep (they do not need S).
// Both kernels walk the points in quads; a quad is moved with one 16-byte access where its segment base is 16-byte aligned
// and the quad is whole, with scalar accesses otherwise (segment s starts at s * N floats).  Which thread sums which point
// does not depend on the alignment.
constexpr int kFdBlocks = 64;
static_assert(PINN_FD_SCRATCH_DOUBLES >= 2 * kFdBlocks, "scratch size");

__device__ __forceinline__ void fd_load4(const float* p, long long i, long long n, bool vec, float v[4]) {
  if (vec && i + 4 <= n) {
    const float4 q = *reinterpret_cast<const float4*>(p + i);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = i + j < n ? p[i + j] : 0.0f;
  }
}

__device__ __forceinline__ void fd_store4(float* p, long long i, long long n, bool vec, const float v[4]) {
  if (vec && i + 4 <= n) {
    *reinterpret_cast<float4*>(p + i) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i + j < n) p[i + j] = v[j];
  }
}

// al: bit 0 x, bit 1 t, bits 2..4 the three segments of x3, bits 5..7 those of t3 — set where 16-byte aligned.
// x + e and x - e are single fp32 operations on (float)eps, then torch.clamp's min(max(v, lo), hi): bit-equal to torch.
__global__ __launch_bounds__(256) void fd_stencil_kernel(const float* x, const float* t, long long n, float eps, float lo, float hi,
                                                         float* x3, float* t3, int al) {
  const long long nq = (n + 3) >> 2;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long long)gridDim.x * 256) {
    const long long i = q << 2;
    float xc[4], tc[4], xp[4], xm[4];
    fd_load4(x, i, n, al & 1, xc);
    fd_load4(t, i, n, al & 2, tc);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      xp[j] = fminf(fmaxf(xc[j] + eps, lo), hi);
      xm[j] = fminf(fmaxf(xc[j] - eps, lo), hi);
    }
    fd_store4(x3, i, n, al & 4, xc);
    fd_store4(x3 + n, i, n, al & 8, xp);
    fd_store4(x3 + 2 * n, i, n, al & 16, xm);
    fd_store4(t3, i, n, al & 32, tc);
    fd_store4(t3 + n, i, n, al & 64, tc);
    fd_store4(t3 + 2 * n, i, n, al & 128, tc);
  }
}

__device__ __forceinline__ float fd_sign(float d) { return d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f); }  // sgn(0) = 0: torch's abs backward

// u3 = [uc | up | um].  Block b sums quads b * 256 + tid, + gridDim * 256, ... in double; partial[2 b] = sum|(up - uc)/e|,
// partial[2 b + 1] = sum|(uc - um)/e|.  The differences are fp32 subtractions (their signs are the reference's signs);
// the quotient is a true division, taken in double.  cot3 = c * {s2 - s1 | s1 | -s2}, c = weight / (e N).
// al: bits 0..2 the segments of u3, bits 3..5 those of cot3.
__global__ __launch_bounds__(256) void fd_smooth_kernel(const float* u3, long long n, double eps, float c, float* cot3, double* partial,
                                                        int al) {
  __shared__ double red[256];
  const long long nq = (n + 3) >> 2;
  double a1 = 0.0, a2 = 0.0;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long long)gridDim.x * 256) {
    const long long i = q << 2;
    float uc[4], up[4], um[4], cc[4], cp[4], cm[4];
    fd_load4(u3, i, n, al & 1, uc);
    fd_load4(u3 + n, i, n, al & 2, up);
    fd_load4(u3 + 2 * n, i, n, al & 4, um);
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // lanes past n were loaded as 0: they add 0 and are not stored
      const float d1 = up[j] - uc[j], d2 = uc[j] - um[j];
      a1 += fabs((double)d1) / eps;
      a2 += fabs((double)d2) / eps;
      const float s1 = fd_sign(d1), s2 = fd_sign(d2);
      cp[j] = s1 * c;
      cc[j] = (s2 - s1) * c;
      cm[j] = -s2 * c;
    }
    fd_store4(cot3, i, n, al & 8, cc);
    fd_store4(cot3 + n, i, n, al & 16, cp);
    fd_store4(cot3 + 2 * n, i, n, al & 32, cm);
  }
  for (int k = 0; k < 2; ++k) {
    red[threadIdx.x] = k ? a2 : a1;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) partial[2 * blockIdx.x + k] = red[0];
    __syncthreads();
  }
}

// one thread: the block partials in a fixed order, S = mean + mean in double, rounded once
__global__ void fd_finish_kernel(const double* partial, int blocks, long long n, float weight, float* loss_out, float* summary4) {
  double s1 = 0.0, s2 = 0.0;
  for (int b = 0; b < blocks; ++b) {
    s1 += partial[2 * b];
    s2 += partial[2 * b + 1];
  }
  const double S = s1 / (double)n + s2 / (double)n;
  loss_out[0] = (float)S;
  if (summary4) summary4[3] = (float)((double)summary4[3] + (double)weight * S);
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

template <int C>
static void launch_adaptive(hipStream_t st, int blocks, float* params, const float* comp_grads, long long ld, float* exp_avg,
                            float* exp_avg_sq, long long n, int vec, int vec_all, double* partial, const float* res, float beta1,
                            float beta2, float eps, float wd, float* grad_out, int phase) {
  if (phase == 0)
    hipLaunchKernelGGL(gram_kernel<C>, dim3(kNormBlocks), dim3(256), 0, st, comp_grads, ld, n, vec, partial);
  else
    hipLaunchKernelGGL(adaptive_adam_kernel<C>, dim3(blocks), dim3(256), 0, st, params, comp_grads, ld, exp_avg, exp_avg_sq, n, vec_all,
                       res, beta1, beta2, eps, wd, grad_out);
}

extern "C" {

int pinn_point_losses(const float* u, int32_t n_total, int32_t n_terms, const int32_t* lo, const int32_t* hi,
                      const float* const* targets, const float* weights, int32_t loss, float huber_delta,
                      float* term_losses, float* cotangent, const float* residual_sum, float residual_scale,
                      float residual_weight, int32_t n_boundary_terms, float* summary4, void* stream) {
  if (!u || !lo || !hi || !targets || !weights || !term_losses || !cotangent) return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_point_losses: null argument");
  if (n_terms < 0 || n_terms > PINN_MAX_POINT_TERMS || n_total < 0) return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_point_losses: term count / point count out of range");
  PointTerms p;
  p.n_terms = n_terms;
  for (int k = 0; k < n_terms; ++k) {
    if (lo[k] < 0 || hi[k] < lo[k] || hi[k] > n_total || !targets[k]) return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_point_losses: bad term range or null target");
    p.lo[k] = lo[k];
    p.hi[k] = hi[k];
    p.target[k] = targets[k];
    p.weight[k] = weights[k];
  }
  p.loss = loss;
  p.huber_delta = huber_delta;
  hipLaunchKernelGGL(point_loss_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), u, p, n_total, term_losses, cotangent,
                     residual_sum, residual_scale, residual_weight, n_boundary_terms, summary4);
  return launched("point_loss_kernel");
}

int pinn_jet_losses(const float* jets, int32_t n_streams, int32_t n_total, int32_t n_terms, const int32_t* lo, const int32_t* hi,
                    const int32_t* stream_of, const int32_t* pair_offset, const float* const* targets, const float* weights,
                    int32_t loss, float huber_delta, float* term_losses, float* cotangent, const float* residual_sum,
                    float residual_scale, float residual_weight, int32_t n_boundary_terms, float* summary4, void* stream) {
  if (!jets || !lo || !hi || !stream_of || !pair_offset || !targets || !weights || !term_losses || !cotangent)
    return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_jet_losses: null argument");
  if (n_terms < 0 || n_terms > PINN_MAX_POINT_TERMS || n_total < 0 || n_streams < 1 || n_streams > PINN_MAX_STREAMS)
    return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_jet_losses: term / stream / point count out of range");
  JetTerms p;
  p.n_terms = n_terms;
  for (int k = 0; k < n_terms; ++k) {
    if (lo[k] < 0 || hi[k] < lo[k] || hi[k] > n_total || stream_of[k] < 0 || stream_of[k] >= n_streams)
      return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_jet_losses: bad term range or stream");
    if (pair_offset[k]) {  // the partner range must lie inside the jets and must not overlap the term's own range
      if (pair_offset[k] < hi[k] - lo[k] || hi[k] + pair_offset[k] > n_total)
        return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_jet_losses: paired range overlaps its partner or leaves the jets");
    } else if (!targets[k]) {
      return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_jet_losses: null target of an unpaired term");
    }
    p.lo[k] = lo[k];
    p.hi[k] = hi[k];
    p.stream[k] = stream_of[k];
    p.pair[k] = pair_offset[k];
    p.target[k] = targets[k];
    p.weight[k] = weights[k];
  }
  p.loss = loss;
  p.huber_delta = huber_delta;
  hipLaunchKernelGGL(jet_loss_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), jets, n_streams, p, n_total, term_losses,
                     cotangent, residual_sum, residual_scale, residual_weight, n_boundary_terms, summary4);
  return launched("jet_loss_kernel");
}

int pinn_adam_clip_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, const float* lr,
                        float beta1, float beta2, float eps, float weight_decay, float max_norm, float* step,
                        float* scratch64, float* grad_norm_out, void* stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || !lr || !step || !scratch64 || n <= 0)
    return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_adam_clip_step: null argument or n <= 0");
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(sumsq_kernel, dim3(kNormBlocks), dim3(256), 0, st, grads, (long long)n, scratch64);
  int rc = launched("sumsq_kernel");
  if (rc) return rc;
  int blocks = (int)((n + 255) / 256);
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(adam_kernel, dim3(blocks), dim3(256), 0, st, params, grads, exp_avg, exp_avg_sq, (long long)n, lr, beta1,
                     beta2, eps, weight_decay, max_norm, step, scratch64, grad_norm_out);
  if ((rc = launched("adam_kernel"))) return rc;
  hipLaunchKernelGGL(step_inc_kernel, dim3(1), dim3(1), 0, st, step);
  return launched("step_inc_kernel");
}

int pinn_adaptive_adam_step(float* params, const float* comp_grads, int64_t ld, int32_t n_components,
                            const float* const* comp_losses, const float* loss_scales, int32_t strategy, double alpha,
                            double aw_eps, const float* initial_weights, float* state16, float* weights4_out, float* summary4,
                            float* exp_avg, float* exp_avg_sq, int64_t n, const float* lr, float beta1, float beta2, float eps,
                            float weight_decay, float max_norm, float* step, float* scratch, float* grad_norm_out,
                            float* grad_out, void* stream) {
  if (!params || !comp_grads || !comp_losses || !state16 || !exp_avg || !exp_avg_sq || !lr || !step || !scratch || n <= 0)
    return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_adaptive_adam_step: null argument or n <= 0");
  if (n_components < 1 || n_components > kMaxComp || ld < n || (strategy != PINN_ADAPTIVE_RBW && strategy != PINN_ADAPTIVE_LRW))
    return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_adaptive_adam_step: component count, row stride or strategy out of range");
  if (reinterpret_cast<uintptr_t>(scratch) & 7u)
    return pinn_internal_fail(PINN_ERR_MISALIGNED, "pinn_adaptive_adam_step: scratch must be 8-byte aligned");
  static_assert(PINN_ADAPTIVE_SCRATCH_FLOATS >= 2 * kMaxPairs * kNormBlocks + kResFloats, "scratch size");
  CompLosses cl;
  for (int c = 0; c < kMaxComp; ++c) {
    if (c < n_components && !comp_losses[c]) return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_adaptive_adam_step: null component loss");
    cl.ptr[c] = c < n_components ? comp_losses[c] : nullptr;
    cl.scale[c] = (c < n_components && loss_scales) ? loss_scales[c] : 1.0f;
    cl.init[c] = (c < n_components && initial_weights) ? initial_weights[c] : 1.0f;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* partial = reinterpret_cast<double*>(scratch);
  float* res = scratch + 2 * kMaxPairs * kNormBlocks;
  auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
  const int vec = al(comp_grads) && ld % 4 == 0;  // the rows of the component gradients can be read 16 bytes at a time
  const int vec_all = vec && al(params) && al(exp_avg) && al(exp_avg_sq) && (!grad_out || al(grad_out));
  int blocks = (int)(((vec_all ? (n + 3) / 4 : n) + 255) / 256);
  if (blocks > 1024) blocks = 1024;
  auto phase = [&](int ph) {
#define PINN_ADAPTIVE_CASE(C)                                                                                              \
  case C:                                                                                                                  \
    launch_adaptive<C>(st, blocks, params, comp_grads, ld, exp_avg, exp_avg_sq, n, vec, vec_all, partial, res, beta1, beta2, \
                       eps, weight_decay, grad_out, ph);                                                                   \
    break;
    switch (n_components) {
      PINN_ADAPTIVE_CASE(1)
      PINN_ADAPTIVE_CASE(2)
      PINN_ADAPTIVE_CASE(3)
      PINN_ADAPTIVE_CASE(4)
    }
#undef PINN_ADAPTIVE_CASE
  };
  phase(0);
  int rc = launched("gram_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(adaptive_update_kernel, dim3(1), dim3(64), 0, st, partial, cl, n_components, strategy, alpha, aw_eps,
                     initial_weights ? 1 : 0, state16, weights4_out, summary4, max_norm, lr, beta1, beta2, step, res, grad_norm_out);
  if ((rc = launched("adaptive_update_kernel"))) return rc;
  phase(1);
  return launched("adaptive_adam_kernel");
}

int pinn_fd_stencil_points(const float* x, const float* t, int64_t N, double eps, double x_lo, double x_hi, float* x3, float* t3,
                           void* stream) {
  if (N < 0 || !(eps > 0.0) || !(x_lo <= x_hi))
    return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_fd_stencil_points: N < 0, eps <= 0 or x_lo > x_hi");
  if (N == 0) return PINN_OK;
  if (!x || !t || !x3 || !t3) return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_fd_stencil_points: null argument");
  auto al = [](const float* p, int64_t off) { return ((reinterpret_cast<uintptr_t>(p) + 4u * (uintptr_t)off) & 15u) == 0; };
  int bits = (al(x, 0) ? 1 : 0) | (al(t, 0) ? 2 : 0);
  for (int s = 0; s < 3; ++s) bits |= (al(x3, s * N) ? 4 << s : 0) | (al(t3, s * N) ? 32 << s : 0);
  const long long nq = ((long long)N + 3) >> 2;
  int blocks = (int)((nq + 255) / 256);
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(fd_stencil_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), x, t, (long long)N, (float)eps,
                     (float)x_lo, (float)x_hi, x3, t3, bits);
  return launched("fd_stencil_kernel");
}

int pinn_fd_smoothness(const float* u3, int64_t N, double eps, float weight, float* loss_out, float* cotangent3, float* summary4,
                       double* scratch, void* stream) {
  if (N <= 0 || !(eps > 0.0)) return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_fd_smoothness: N <= 0 or eps <= 0");
  if (!u3 || !loss_out || !cotangent3 || !scratch) return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_fd_smoothness: null argument");
  if (reinterpret_cast<uintptr_t>(scratch) & 7u)
    return pinn_internal_fail(PINN_ERR_MISALIGNED, "pinn_fd_smoothness: scratch must be 8-byte aligned");
  auto al = [](const float* p, int64_t off) { return ((reinterpret_cast<uintptr_t>(p) + 4u * (uintptr_t)off) & 15u) == 0; };
  int bits = 0;
  for (int s = 0; s < 3; ++s) bits |= (al(u3, s * N) ? 1 << s : 0) | (al(cotangent3, s * N) ? 8 << s : 0);
  const long long nq = ((long long)N + 3) >> 2;
  int blocks = (int)((nq + 255) / 256);
  if (blocks > kFdBlocks) blocks = kFdBlocks;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float c = (float)((double)weight / (eps * (double)N));
  hipLaunchKernelGGL(fd_smooth_kernel, dim3(blocks), dim3(256), 0, st, u3, (long long)N, eps, c, cotangent3, scratch, bits);
  int rc = launched("fd_smooth_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(fd_finish_kernel, dim3(1), dim3(1), 0, st, scratch, blocks, (long long)N, weight, loss_out, summary4);
  return launched("fd_finish_kernel");
}

}  // extern "C"
