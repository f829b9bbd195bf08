// L-BFGS over flat fp32 buffers (include/pinn_jet.h, "L-BFGS" section): the direction update of torch.optim.LBFGS.step()
// (torch/optim/lbfgs.py:396-460) as three launches, and the reductions its line search reads after every closure evaluation
// as two.  The closure itself is the launch list of the training step without its optimiser tail.
//
// The two-loop recursion runs in COEFFICIENT space: q and r are linear combinations of the basis {g, s_i, y_i}, so every
// s_i . q and y_i . r is a short dot of a row of the basis' Gram matrix with the coefficient vector.  The Gram entries of
// the ring rows persist in the state (a new pair adds one row and one column); the entries against g are formed by the
// update pass of every call.  Mathematically this is torch's vector recursion; its scalars are double and its Gram entries
// are double sums of exact fp32 products, so it loses accuracy against the direct form only under cancellation of order
// 1e7 or more.  No atomics, fixed grids, fixed summation order: bit-identical across runs.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <type_traits>

#include "../../include/pinn_jet.h"

namespace {

constexpr int kBlocks = 64;  // the fixed grid of every pass over the n elements (and the number of max|d| partials)
constexpr int kMaxHist = PINN_LBFGS_MAX_HISTORY;
constexpr int kMaxDots = 6 * kMaxHist + 8;
static_assert(PINN_LBFGS_RECORD_DOUBLES == 8 + kBlocks, "record = 8 scalars + one max|d| partial per block");

// state (doubles): {head, count, n_iter, H_diag, -, -, -, -}, ro[S], Gram[2S x 2S] with S = history_size + 1 ring slots;
// Gram index of the s row in slot a: a, of its y row: S + a.  head = slot of the oldest live pair; the live pairs are the
// slots (head + k) % S, k = 0 .. count - 1, oldest first; the spare slot (head + count) % S takes the tentative pair.
enum { kStHead = 0, kStCount = 1, kStIter = 2, kStHdiag = 3, kStRo = 8 };
// record (doubles)
enum { kRecLoss = 0, kRecGtd = 1, kRecGmax = 2, kRecGsum = 3, kRecAccepted = 4, kRecCount = 5, kRecIter = 6, kRecHdiag = 7, kRecDmax = 8 };
// partial sums of the update pass, dot j of block b at partial[j * kBlocks + b].  Live pair k (age order) has the six
// dots 6k + {sN.s_k, sN.y_k, yN.s_k, yN.y_k, g.s_k, g.y_k}; after the c live pairs come
// {sN.sN, sN.yN, yN.yN, g.sN, g.yN, g.g, max|g|, sum|g|}  (sN, yN: the tentative pair).
enum { kTailSS = 0, kTailSY = 1, kTailYY = 2, kTailGS = 3, kTailGY = 4, kTailGG = 5, kTailGmax = 6, kTailGsum = 7 };

__device__ __forceinline__ double wave_sum(double v) {  // butterfly: a fixed tree, the same bits in every lane
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

template <int V>
struct Pack {
  float v[V];
};
template <int V>
__device__ __forceinline__ Pack<V> load(const float* p, long long i) {  // V = 4: i counts 16-byte units; V = 1: elements
  Pack<V> r;
  if constexpr (V == 4) {
    const float4 q = reinterpret_cast<const float4*>(p)[i];
    r.v[0] = q.x, r.v[1] = q.y, r.v[2] = q.z, r.v[3] = q.w;
  } else {
    r.v[0] = p[i];
  }
  return r;
}
template <int V>
__device__ __forceinline__ void store(float* p, long long i, const Pack<V>& r) {
  if constexpr (V == 4) reinterpret_cast<float4*>(p)[i] = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
  else p[i] = r.v[0];
}

// Every pass walks the elements the same way: 16-byte units i = first, first + stride, .. below nv = n / 4 when the
// buffers are aligned (vec), then the remaining elements one by one.  A thread therefore meets the same elements in each of
// its loops, which is what lets the update pass read back the tentative pair it has just written.
// body(std::integral_constant<int, V>, i): V = 4 with i a unit index, V = 1 with i an element index.
template <class F>
__device__ __forceinline__ void for_elements(long long n, int vec, F&& body) {
  const long long first = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)kBlocks * 256;
  const long long nv = vec ? n >> 2 : 0;
  for (long long i = first; i < nv; i += stride) body(std::integral_constant<int, 4>{}, i);
  for (long long i = (nv << 2) + first; i < n; i += stride) body(std::integral_constant<int, 1>{}, i);
}

// head and count as the state holds them, kept inside the ring whatever the caller left in the state
__device__ __forceinline__ void ring_position(const double* state, int S, int* head, int* count) {
  const int h = (int)state[kStHead], c = (int)state[kStCount];
  *head = h < 0 ? 0 : (h >= S ? S - 1 : h);
  *count = c < 0 ? 0 : (c >= S ? S - 1 : c);
}

// Update pass: the tentative pair y = g - prev_grad, s = t_prev * d into the spare ring slot, prev_grad = g, and this
// block's share of every inner product the one-workgroup launch needs.  On the first iteration (n_iter == 0) no pair work.
__global__ __launch_bounds__(256) void lbfgs_update_kernel(const float* g, float* prev_grad, const float* d, float* ring, long long ld,
                                                           long long n, int S, int vec, float t_prev, const double* state,
                                                           double* partial) {
  __shared__ double red[kMaxDots * 4];
  int head, count;
  ring_position(state, S, &head, &count);
  const bool first_iter = state[kStIter] == 0.0;
  const int c = first_iter ? 0 : count;
  const int sp = (head + count) % S;
  float* sN = ring + (long long)sp * ld;
  float* yN = ring + (long long)(S + sp) * ld;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int T = 6 * c;

  double a[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = 0.0;
  for_elements(n, vec, [&](auto vc, long long i) {
    constexpr int V = decltype(vc)::value;
    const Pack<V> gi = load<V>(g, i);
    Pack<V> si, yi;
    if (!first_iter) {
      const Pack<V> pi = load<V>(prev_grad, i), di = load<V>(d, i);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        si.v[e] = di.v[e] * t_prev;       // torch: d.mul(t)
        yi.v[e] = gi.v[e] - pi.v[e];      // torch: flat_grad.sub(prev_flat_grad)
      }
      store<V>(sN, i, si);
      store<V>(yN, i, yi);
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e) si.v[e] = yi.v[e] = 0.0f;
    }
    store<V>(prev_grad, i, gi);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const double gd = (double)gi.v[e], sd = (double)si.v[e], yd = (double)yi.v[e];
      a[kTailSS] = fma(sd, sd, a[kTailSS]);
      a[kTailSY] = fma(sd, yd, a[kTailSY]);
      a[kTailYY] = fma(yd, yd, a[kTailYY]);
      a[kTailGS] = fma(gd, sd, a[kTailGS]);
      a[kTailGY] = fma(gd, yd, a[kTailGY]);
      a[kTailGG] = fma(gd, gd, a[kTailGG]);
      a[kTailGmax] = fmax(a[kTailGmax], fabs(gd));
      a[kTailGsum] += fabs(gd);
    }
  });
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const double w = j == kTailGmax ? wave_max(a[j]) : wave_sum(a[j]);
    if (lane == 0) red[(T + j) * 4 + wave] = w;
  }

  for (int k = 0; k < c; ++k) {  // the live pairs, oldest first
    const int sl = (head + k) % S;
    const float* sk = ring + (long long)sl * ld;
    const float* yk = ring + (long long)(S + sl) * ld;
    double b[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) b[j] = 0.0;
    for_elements(n, vec, [&](auto vc, long long i) {
    constexpr int V = decltype(vc)::value;
      const Pack<V> gi = load<V>(g, i), si = load<V>(sN, i), yi = load<V>(yN, i), ski = load<V>(sk, i), yki = load<V>(yk, i);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const double gd = (double)gi.v[e], sd = (double)si.v[e], yd = (double)yi.v[e], skd = (double)ski.v[e], ykd = (double)yki.v[e];
        b[0] = fma(sd, skd, b[0]);
        b[1] = fma(sd, ykd, b[1]);
        b[2] = fma(yd, skd, b[2]);
        b[3] = fma(yd, ykd, b[3]);
        b[4] = fma(gd, skd, b[4]);
        b[5] = fma(gd, ykd, b[5]);
      }
    });
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const double w = wave_sum(b[j]);
      if (lane == 0) red[(6 * k + j) * 4 + wave] = w;
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < T + 8; j += 256) {
    const double* r = red + j * 4;
    partial[j * kBlocks + blockIdx.x] = j == T + kTailGmax ? fmax(fmax(r[0], r[1]), fmax(r[2], r[3])) : ((r[0] + r[1]) + (r[2] + r[3]));
  }
}

// One workgroup (one wave): the only launch that writes the state.  Sums the partials in a fixed order, accepts or rejects
// the tentative pair, runs the two-loop recursion on coefficients and writes them (coef[0] on g, coef[1 + k] on s_k,
// coef[1 + count + k] on y_k, k in age order) with the record's scalars.
__global__ __launch_bounds__(64) void lbfgs_solve_kernel(const double* partial, double* state, int S, int H, double* coef, double* record) {
  __shared__ double dots[kMaxDots];
  __shared__ double cs[kMaxHist], cy[kMaxHist], al[kMaxHist], gs[kMaxHist], gy[kMaxHist], ro[kMaxHist];
  __shared__ int slot[kMaxHist];
  const int lane = threadIdx.x;
  int head, count;
  ring_position(state, S, &head, &count);
  const double n_iter = state[kStIter];
  double hdiag = state[kStHdiag];
  const bool first_iter = n_iter == 0.0;
  const int c_old = first_iter ? 0 : count, T = 6 * c_old, head_old = head;
  for (int j = lane; j < T + 8; j += 64) {
    const double* p = partial + j * kBlocks;
    double tot = 0.0;
    if (j == T + kTailGmax) {
      for (int b = 0; b < kBlocks; ++b) tot = fmax(tot, p[b]);
    } else {
      for (int b = 0; b < kBlocks; ++b) tot += p[b];
    }
    dots[j] = tot;
  }
  __syncthreads();
  double* ros = state + kStRo;
  double* G = state + kStRo + S;
  const int W = 2 * S;
  bool accepted = false;
  int sp = -1;
  if (first_iter) {  // torch: old_dirs = [], old_stps = [], ro = [], H_diag = 1
    head = 0, count = 0, hdiag = 1.0;
  } else {
    const double ys = dots[T + kTailSY], yy = dots[T + kTailYY];
    accepted = ys > 1e-10;
    if (accepted) {
      sp = (head + count) % S;
      for (int k = lane; k < c_old; k += 64) {  // the new row and column; a pair about to be evicted is written too, and never read
        const int sl = (head + k) % S;
        G[sp * W + sl] = G[sl * W + sp] = dots[6 * k + 0];
        G[sp * W + S + sl] = G[(S + sl) * W + sp] = dots[6 * k + 1];
        G[(S + sp) * W + sl] = G[sl * W + S + sp] = dots[6 * k + 2];
        G[(S + sp) * W + S + sl] = G[(S + sl) * W + S + sp] = dots[6 * k + 3];
      }
      if (lane == 0) {
        G[sp * W + sp] = dots[T + kTailSS];
        G[sp * W + S + sp] = G[(S + sp) * W + sp] = ys;
        G[(S + sp) * W + S + sp] = yy;
        ros[sp] = 1.0 / ys;
      }
      hdiag = ys / yy;
      if (count == H) head = (head + 1) % S;  // the oldest pair leaves; its slot is the next spare one
      else ++count;
    }
  }
  __syncthreads();
  for (int k = lane; k < count; k += 64) {
    const int sl = (head + k) % S;
    slot[k] = sl;
    ro[k] = ros[sl];
    cs[k] = cy[k] = 0.0;
    if (sl == sp) {
      gs[k] = dots[T + kTailGS], gy[k] = dots[T + kTailGY];
    } else {
      const int k_old = (sl - head_old + S) % S;
      gs[k] = dots[6 * k_old + 4], gy[k] = dots[6 * k_old + 5];
    }
  }
  __syncthreads();
  const double gg = dots[T + kTailGG];
  double cg = -1.0;  // q = -g
  for (int i = count - 1; i >= 0; --i) {  // newest to oldest: al_i = ro_i s_i.q, q -= al_i y_i
    const double* row = G + (long long)slot[i] * W;
    double p = 0.0;
    for (int k = lane; k < count; k += 64) p = fma(cy[k], row[S + slot[k]], fma(cs[k], row[slot[k]], p));
    p = wave_sum(p) + cg * gs[i];
    const double a = p * ro[i];
    __syncthreads();
    if (lane == 0) {
      al[i] = a;
      cy[i] -= a;
    }
    __syncthreads();
  }
  cg *= hdiag;  // r = H_diag q
  for (int k = lane; k < count; k += 64) cs[k] *= hdiag, cy[k] *= hdiag;
  __syncthreads();
  for (int i = 0; i < count; ++i) {  // oldest to newest: be_i = ro_i y_i.r, r += (al_i - be_i) s_i
    const double* row = G + (long long)(S + slot[i]) * W;
    double p = 0.0;
    for (int k = lane; k < count; k += 64) p = fma(cy[k], row[S + slot[k]], fma(cs[k], row[slot[k]], p));
    p = wave_sum(p) + cg * gy[i];
    const double be = p * ro[i];
    __syncthreads();
    if (lane == 0) cs[i] += al[i] - be;
    __syncthreads();
  }
  double p = 0.0;
  for (int k = lane; k < count; k += 64) p = fma(cy[k], gy[k], fma(cs[k], gs[k], p));
  const double gtd = wave_sum(p) + cg * gg;
  for (int k = lane; k < count; k += 64) coef[1 + k] = cs[k], coef[1 + count + k] = cy[k];
  if (lane == 0) {
    coef[0] = cg;
    state[kStHead] = (double)head;
    state[kStCount] = (double)count;
    state[kStIter] = n_iter + 1.0;
    state[kStHdiag] = hdiag;
    record[kRecLoss] = 0.0;
    record[kRecGtd] = gtd;
    record[kRecGmax] = dots[T + kTailGmax];
    record[kRecGsum] = dots[T + kTailGsum];
    record[kRecAccepted] = accepted ? 1.0 : 0.0;
    record[kRecCount] = (double)count;
    record[kRecIter] = n_iter + 1.0;
    record[kRecHdiag] = hdiag;
  }
}

// Combine pass: d[i] = coef_g g[i] + sum_k (coef_s[k] s_k[i] + coef_y[k] y_k[i]), accumulated in double in registers and
// rounded once; record[kRecDmax + block] = this block's max|d| (the maximum over the blocks is max|d|).
__global__ __launch_bounds__(256) void lbfgs_combine_kernel(const float* g, const float* ring, long long ld, long long n, int S, int vec,
                                                            const double* state, const double* coef, float* d, double* record) {
  __shared__ double c_sh[2 * kMaxHist + 1];
  __shared__ int slot[kMaxHist];
  __shared__ double red[4];
  int head, count;
  ring_position(state, S, &head, &count);
  for (int j = threadIdx.x; j < 2 * count + 1; j += 256) c_sh[j] = coef[j];
  for (int k = threadIdx.x; k < count; k += 256) slot[k] = (head + k) % S;
  __syncthreads();
  const double cg = c_sh[0];
  double m = 0.0;
  for_elements(n, vec, [&](auto vc, long long i) {
    constexpr int V = decltype(vc)::value;
    const Pack<V> gi = load<V>(g, i);
    double acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = cg * (double)gi.v[e];
    for (int k = 0; k < count; ++k) {
      const Pack<V> sk = load<V>(ring + (long long)slot[k] * ld, i), yk = load<V>(ring + (long long)(S + slot[k]) * ld, i);
      const double a = c_sh[1 + k], b = c_sh[1 + count + k];
#pragma unroll
      for (int e = 0; e < V; ++e) acc[e] = fma(b, (double)yk.v[e], fma(a, (double)sk.v[e], acc[e]));
    }
    Pack<V> di;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      di.v[e] = (float)acc[e];
      m = fmax(m, fabs((double)di.v[e]));
    }
    store<V>(d, i, di);
  });
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) record[kRecDmax + blockIdx.x] = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// The line search's reductions of one evaluated trial point: partial[0 .. 64) g.d, [64 .. 128) max|g|, [128 .. 192) sum|g|
__global__ __launch_bounds__(256) void lbfgs_eval_partial_kernel(const float* g, const float* d, long long n, int vec, double* partial) {
  __shared__ double red[3 * 4];
  double a[3] = {0.0, 0.0, 0.0};
  for_elements(n, vec, [&](auto vc, long long i) {
    constexpr int V = decltype(vc)::value;
    const Pack<V> gi = load<V>(g, i), di = load<V>(d, i);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const double gd = (double)gi.v[e];
      a[0] = fma(gd, (double)di.v[e], a[0]);
      a[1] = fmax(a[1], fabs(gd));
      a[2] += fabs(gd);
    }
  });
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double w = j == 1 ? wave_max(a[j]) : wave_sum(a[j]);
    if (lane == 0) red[j * 4 + wave] = w;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const double* r = red + threadIdx.x * 4;
    partial[threadIdx.x * kBlocks + blockIdx.x] = threadIdx.x == 1 ? fmax(fmax(r[0], r[1]), fmax(r[2], r[3])) : ((r[0] + r[1]) + (r[2] + r[3]));
  }
}

__global__ __launch_bounds__(64) void lbfgs_eval_final_kernel(const double* partial, const float* loss, double* record) {
  const int j = threadIdx.x;
  if (j < 3) {
    const double* p = partial + j * kBlocks;
    double tot = 0.0;
    if (j == 1) {
      for (int b = 0; b < kBlocks; ++b) tot = fmax(tot, p[b]);
    } else {
      for (int b = 0; b < kBlocks; ++b) tot += p[b];
    }
    record[kRecGtd + j] = tot;  // kRecGtd, kRecGmax, kRecGsum are consecutive
  } else if (j == 3) {
    record[kRecLoss] = loss ? (double)loss[0] : 0.0;
  } else if (j < PINN_LBFGS_RECORD_DOUBLES) {
    record[j] = 0.0;
  }
  if (j + 64 < PINN_LBFGS_RECORD_DOUBLES) record[j + 64] = 0.0;
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

static bool aligned(const void* p, unsigned mask) { return (reinterpret_cast<uintptr_t>(p) & mask) == 0; }

extern "C" {

size_t pinn_lbfgs_state_bytes(int32_t history_size) {
  if (history_size < 1 || history_size > kMaxHist) return 0;
  const size_t S = (size_t)history_size + 1;
  return (kStRo + S + 4 * S * S) * sizeof(double);
}

size_t pinn_lbfgs_scratch_bytes(int32_t history_size) {
  if (history_size < 1 || history_size > kMaxHist) return 0;
  // the update pass's partials (3 * kBlocks of them serve pinn_lbfgs_eval_stats), then the coefficients
  return ((size_t)(6 * history_size + 8) * kBlocks + 2 * (size_t)history_size + 2) * sizeof(double);
}

int pinn_lbfgs_direction(const float* grad, float* prev_grad, float* direction, float* ring, int64_t ld, int64_t n,
                         int32_t history_size, double t_prev, double* state, double* scratch, double* record, void* stream) {
  if (!grad || !prev_grad || !direction || !ring || !state || !scratch || !record || n <= 0)
    return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_lbfgs_direction: null argument or n <= 0");
  if (history_size < 1 || history_size > kMaxHist || ld < n)
    return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_lbfgs_direction: history_size outside [1, 64] or ld < n");
  if (!aligned(state, 7u) || !aligned(scratch, 7u) || !aligned(record, 7u))
    return pinn_internal_fail(PINN_ERR_MISALIGNED, "pinn_lbfgs_direction: state, scratch and record must be 8-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int S = history_size + 1;
  const int vec = aligned(grad, 15u) && aligned(prev_grad, 15u) && aligned(direction, 15u) && aligned(ring, 15u) && ld % 4 == 0;
  double* coef = scratch + (size_t)(6 * history_size + 8) * kBlocks;
  hipLaunchKernelGGL(lbfgs_update_kernel, dim3(kBlocks), dim3(256), 0, st, grad, prev_grad, direction, ring, (long long)ld, (long long)n,
                     S, vec, (float)t_prev, state, scratch);
  int rc = launched("lbfgs_update_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(lbfgs_solve_kernel, dim3(1), dim3(64), 0, st, scratch, state, S, (int)history_size, coef, record);
  if ((rc = launched("lbfgs_solve_kernel"))) return rc;
  hipLaunchKernelGGL(lbfgs_combine_kernel, dim3(kBlocks), dim3(256), 0, st, grad, ring, (long long)ld, (long long)n, S, vec, state, coef,
                     direction, record);
  return launched("lbfgs_combine_kernel");
}

int pinn_lbfgs_eval_stats(const float* grad, const float* direction, int64_t n, const float* loss, double* scratch, double* record,
                          void* stream) {
  if (!grad || !direction || !scratch || !record || n <= 0)
    return pinn_internal_fail(PINN_ERR_BAD_DESC, "pinn_lbfgs_eval_stats: null argument or n <= 0");
  if (!aligned(scratch, 7u) || !aligned(record, 7u))
    return pinn_internal_fail(PINN_ERR_MISALIGNED, "pinn_lbfgs_eval_stats: scratch and record must be 8-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int vec = aligned(grad, 15u) && aligned(direction, 15u);
  hipLaunchKernelGGL(lbfgs_eval_partial_kernel, dim3(kBlocks), dim3(256), 0, st, grad, direction, (long long)n, vec, scratch);
  int rc = launched("lbfgs_eval_partial_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(lbfgs_eval_final_kernel, dim3(1), dim3(64), 0, st, scratch, loss, record);
  return launched("lbfgs_eval_final_kernel");
}

}  // extern "C"
