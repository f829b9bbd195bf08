// Fused forward + reverse tile-major kernel on 16-point units: eight waves per workgroup, v_mfma_f32_16x16x4_f32,
// tape held in LDS.  It serves reverse launches of the store-flush class of jet_kernel_wide.h
// (plain MLPs whose MFMA layers all keep their weight gradients in registers: 1 <= n_layers <= kPersist) at image
// height 128, and the forward-only launches of the same networks (BWD = false), so that both give bit-identical
// per-point results; every other call keeps the 32-point kernel.
//
//   * One 512-thread workgroup per CU, two waves per SIMD.  Wave w owns feature rows 16w .. 16w+15 of every layer:
//     forward z = W a, reverse abar = W^T zbar (its input-feature rows) and dW += zbar a^T (its output rows), so the
//     persistent weight-gradient tiles are split eight ways (80 VGPRs for the headline network instead of 160).
//   * Workgroup b takes 16-point units b, b + grid, ... of ceil(N / 16): the grid stays min(CUs, ceil(N / 32)), so
//     every workgroup does about two units per 32-point tile of the older kernel, and the last round is half as long.
//   * Activation images are [stream][point][feature] with a row of kUP = 132 floats.  In the forward and abar GEMMs
//     lane group g = lane >> 4 takes features 16b + 4g + m at MFMA step m = 0..3, so one ds_read_b128 of four
//     consecutive features feeds four 16x16x4 MFMAs, and a producer lane, which holds rows 4g .. 4g+3 of its
//     accumulator for point lane & 15, writes them back with one ds_write_b128.  The 4-float row pad (instead of an
//     XOR swizzle) keeps every LDS access base register + immediate offset; it leaves one 2-way bank conflict in
//     one of the four lane groups of a b128 read.  The dW GEMM sums over points and reads both operands with
//     conflict-free ds_read_b32.
//   * The pre-activation records that the reverse sweep replays (layers 0 .. n_layers - 2) stay in two LDS images,
//     and the last layer's record is parked in the wave's own columns of the idle a_{l-1} image: no tape in global
//     memory, no workspace besides the store-flush slab.
//   * Barriers.  The forward sweep ping-pongs between the images X and A2 (one barrier per layer boundary); the
//     encoding goes to the image that makes the last layer read X, so the reverse sweep always has zbar in X and
//     a_{l-1} in A2.  The coordinates of the workgroup's next unit are stored into the other half of a double buffer
//     during the current unit, so a unit starts with one barrier.  In the reverse sweep the two waves of a SIMD
//     (w and w + 4) run a layer's two GEMMs in opposite order, so that the activation adjoint of each (VALU) runs
//     beside a GEMM of the other.  Ten barriers per unit for three MFMA layers behind Fourier features.
//   * Reverse launches of the merged units (K = 3) have LDS for a fifth image S and keep what the forward sweep wrote:
//     static image roles, the last layer's record in S, every zbar stored over the record it was computed from, so a
//     reverse layer is one barrier and two GEMMs, without the put and the replay (KEEP in the kernel; eight barriers per
//     unit for the network above; DESIGN.md §4.1 has the table of who reads and writes which image when).
//   * Registers.  The reverse kernel sits at the 256-VGPR limit of two waves per SIMD, and what the optimizer hoists
//     out of the unit loop is spilled.  So running sums that one phase alone touches (dw_out per lane, loss, db_out)
//     and the PDE coefficients live in LDS, and addresses used once per unit or once per kernel are formed from an
//     opaque copy of the thread index where they are used (u16_opaque).
//   * No atomics: per-lane partial sums (db, dw_out, db_out, loss) and the weight-gradient tiles are written once per
//     workgroup into row blockIdx.x of the slab, and units run in a fixed order, so results are bitwise
//     reproducible from run to run.
#pragma once
#include "jet_kernel_wide.h"

namespace pinn {

// workgroup barrier; the diagnostic build books the time up to it on phase idx and the wait itself on ST_BARRIER
#define U16_BARRIER(idx)     \
  do {                       \
    PINN_STAMP(idx);         \
    __syncthreads();         \
    PINN_STAMP(ST_BARRIER);  \
  } while (0)

constexpr int kU = 16;          // points per unit
constexpr int kUP = 132;        // LDS row of an image: 128 features + 4 floats of pad
constexpr int kUThreads = 512;  // 8 waves
constexpr int kUWaves = 8;
constexpr int kUH = 128;        // image height (features)
constexpr int kUImgS = kU * kUP;  // floats per stream of an image

// The shape the fixed-shape units (FIXED in the kernel) are compiled for: the default network of the package, fixed for a
// whole training run.  jet_u16_fixed_shape() compares a NetDev with it.
struct U16FixedShape {
  int din, enc_out, layers, in0, width;
};
constexpr U16FixedShape kUFixed = {2, 64, 3, 64, 128};

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// a value the optimizer cannot trace back to its source: what is derived from it is computed where it is used
__device__ __forceinline__ int u16_opaque(int v) {
  asm volatile("" : "+v"(v));
  return v;
}

// pre-activation jets of encoding feature j at point n of the unit (xin: [c][kU])
template <int NT, int NX>
__device__ __forceinline__ void u16_enc_preact(const float* ep, int din, const float* xin, int j, int n, float* z) {
  constexpr int K = 1 + NT + NX;
#pragma unroll
  for (int s = 0; s < K; ++s) z[s] = 0.0f;
  float v = ep[kMaxDin * kUH + j];
  float wt = 0.0f;
#pragma unroll
  for (int c = 0; c < kMaxDin; ++c) {
    const float w = ep[c * kUH + j];  // zero beyond din
    v = fmaf(xin[c * kU + n], w, v);
    wt = c == din - 1 ? w : wt;
  }
  z[0] = v;
  if constexpr (NT >= 1) z[1] = wt;
  if constexpr (NX >= 1) z[1 + NT] = ep[j];
}

// encoding into an image dst[s][n][f]; thread -> (point tid & 15, feature tid >> 4 + 32 i)
// MRG: the merged stream set [value, w, d/dx] (jet_device.h), cc its coefficient c; NT = NX = 1 then
// FIXED: the fixed-shape units (kUFixed): Fourier features, 64 of them, of two coordinates
template <int ACT, int NT, int NX, bool MRG = false, bool FIXED = false>
__device__ __forceinline__ void u16_encode(const NetDev& net, const float* ep, const float* xin, float* dst, int tid, float cc = 0.0f) {
  constexpr int K = 1 + NT + NX;
  const int n = tid & 15;
  const int din = FIXED ? kUFixed.din : net.din;
  float* row = dst + n * kUP;
  if (FIXED || net.enc == ENC_FOURIER) {
    const int M = FIXED ? kUFixed.enc_out >> 1 : net.enc_out >> 1;
#pragma unroll 1
    for (int m = tid >> 4; m < M; m += kUThreads / kU) {
      float z[K], ys[K], yc[K];
      u16_enc_preact<NT, NX>(ep, din, xin, m, n, z);
      float sn, cs;
      fast_sincosf(z[0], &sn, &cs);
      const float fs[6] = {sn, cs, -sn, -cs, sn, cs};
      const float fc[6] = {cs, -sn, -cs, sn, cs, -sn};
      ys[0] = sn;
      yc[0] = cs;
      if constexpr (MRG) {
        merged_fwd(fs, cc, z, ys);
        merged_fwd(fc, cc, z, yc);
      } else {
        dir_fwd<NT>(fs, z + 1, ys + 1);
        dir_fwd<NX>(fs, z + 1 + NT, ys + 1 + NT);
        dir_fwd<NT>(fc, z + 1, yc + 1);
        dir_fwd<NX>(fc, z + 1 + NT, yc + 1 + NT);
      }
#pragma unroll
      for (int s = 0; s < K; ++s) {
        row[s * kUImgS + m] = ys[s];
        row[s * kUImgS + M + m] = yc[s];
      }
    }
  } else {
    const int H = net.enc_out;
#pragma unroll 1
    for (int f = tid >> 4; f < H; f += kUThreads / kU) {
      float z[K], y[K];
      u16_enc_preact<NT, NX>(ep, din, xin, f, n, z);
      if constexpr (MRG) act_fwd_merged<ACT>(net.enc_param, cc, z, y);
      else act_fwd<ACT, NT, NX>(net.enc_param, z, y);
#pragma unroll
      for (int s = 0; s < K; ++s) row[s * kUImgS + f] = y[s];
    }
  }
}

// Weight operand of block b (16 k): rows form (z = W a) one 16-byte load of W[16w + c][16b + 4g .. +3]; columns form
// (abar = W^T zbar) four loads W[16b + 4g + m][16w + c].  W is wave-uniform (scalar base), the lane part is a 32-bit
// byte offset (u16_rows_off / u16_cols_off): no per-lane 64-bit addresses, which the optimizer hoists out of the unit
// loop and then spills.
__device__ __forceinline__ unsigned u16_rows_off(int row0, int ld, int c, int g) {
  return static_cast<unsigned>((row0 + c) * ld + 4 * g) * 4u;
}
__device__ __forceinline__ unsigned u16_cols_off(int col0, int ld, int c, int g) {
  return static_cast<unsigned>(4 * g * ld + col0 + c) * 4u;
}
template <bool COLS>
__device__ __forceinline__ f32x4 u16_wload(const float* W, int ld, unsigned off, int b) {
  if constexpr (COLS) {
    f32x4 v;
#pragma unroll
    for (int m = 0; m < 4; ++m) v[m] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(W + (long long)(16 * b + m) * ld) + off);
    return v;
  } else {
    return *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(W + 16 * b) + off);
  }
}

// acc[s] += W-slice . X[s][c][:] over depth 16 NB; xl = X + c kUP + 4g.  Weights are requested two blocks ahead of
// their MFMAs (blocks 0 and 1 by the caller, a phase earlier), image operands one block ahead.
template <int K, int NB, bool COLS>
__device__ __forceinline__ void u16_gemm_n(f32x4 (&acc)[K], const float* W, int ld, unsigned off, f32x4 w0, f32x4 w1, const float* xl) {
  f32x4 wq[3];
  wq[0] = w0;
  wq[1] = w1;
  f32x4 bc[K], bn[K];
#pragma unroll
  for (int s = 0; s < K; ++s) bc[s] = *reinterpret_cast<const f32x4*>(xl + s * kUImgS);
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    if (b + 2 < NB) wq[(b + 2) % 3] = u16_wload<COLS>(W, ld, off, b + 2);
    if (b + 1 < NB) {
#pragma unroll
      for (int s = 0; s < K; ++s) bn[s] = *reinterpret_cast<const f32x4*>(xl + s * kUImgS + 16 * (b + 1));
    }
    // keep the operand requests of block b+1 ahead of the MFMAs of block b
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int s = 0; s < K; ++s) acc[s] = mfma16(wq[b % 3][m], bc[s][m], acc[s]);
    __builtin_amdgcn_sched_barrier(0);
    if (b + 1 < NB) {
#pragma unroll
      for (int s = 0; s < K; ++s) bc[s] = bn[s];
    }
  }
}

// depth = 16 nb (nb wave-uniform)
template <int K, bool COLS>
__device__ __forceinline__ void u16_gemm(f32x4 (&acc)[K], const float* W, int ld, unsigned off, f32x4 w0, f32x4 w1, int nb, const float* xl) {
  switch (nb) {
    case 8: u16_gemm_n<K, 8, COLS>(acc, W, ld, off, w0, w1, xl); return;
    case 4: u16_gemm_n<K, 4, COLS>(acc, W, ld, off, w0, w1, xl); return;
    default: break;
  }
#pragma unroll 1
  for (int b = 0; b < nb; ++b) {
    const f32x4 w = b == 0 ? w0 : b == 1 ? w1 : u16_wload<COLS>(W, ld, off, b);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int s = 0; s < K; ++s) acc[s] = mfma16(w[m], xl[s * kUImgS + 16 * b + m], acc[s]);
  }
}

// pt[OFF + t] += sum_s Z_s[own rows][points] A_s[16t + j][points]^T, t < NA.  Point order: lane group g takes point
// 4g + m at step m; zl = Z + 4g kUP + 16w + c, al = A + 4g kUP + c (ds_read_b32, conflict-free)
template <int K, int NA, int OFF, int NPT>
__device__ __forceinline__ void u16_outer_n(f32x4 (&pt)[NPT], const float* zl, const float* al) {
  float zc, zn, ac[NA], an[NA];
  zc = zl[0];
#pragma unroll
  for (int t = 0; t < NA; ++t) ac[t] = al[16 * t];
#pragma unroll
  for (int st = 0; st < 4 * K; ++st) {  // step = (stream s, point m)
    if (st + 1 < 4 * K) {
      const int s = (st + 1) >> 2, m = (st + 1) & 3;
      zn = zl[s * kUImgS + m * kUP];
#pragma unroll
      for (int t = 0; t < NA; ++t) an[t] = al[s * kUImgS + m * kUP + 16 * t];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < NA; ++t) pt[OFF + t] = mfma16(zc, ac[t], pt[OFF + t]);
    __builtin_amdgcn_sched_barrier(0);
    if (st + 1 < 4 * K) {
      zc = zn;
#pragma unroll
      for (int t = 0; t < NA; ++t) ac[t] = an[t];
    }
  }
}

// na = in_dim / 16 (wave-uniform).  A narrower layer than NMAX runs the NMAX form when na is not NMAX / 2: the
// extra tiles read image columns beyond in_dim and are never flushed.
template <int K, int OFF, int NMAX, int NPT>
__device__ __forceinline__ void u16_outer(f32x4 (&pt)[NPT], int na, const float* zl, const float* al) {
  if constexpr (NMAX >= 8) {
    if (na * 2 == NMAX) { u16_outer_n<K, NMAX / 2, OFF, NPT>(pt, zl, al); return; }
  }
  u16_outer_n<K, NMAX, OFF, NPT>(pt, zl, al);
}

// ---- the packed round (the kernel's last round): a 16-column operand group holds 4 points x 4 streams
// instead of 16 points x 1 stream.  Column c of group j is (stream c >> 2, point 4j + (c & 3)); the images keep their
// [stream][point][feature] layout, rows 0 .. 4G-1 in use.  G (1..3) is wave-uniform; every j < G test below is a scalar
// branch around a block of MFMAs, so accumulator indices stay compile-time. ----
#ifndef PINN_U16_PACK
#define PINN_U16_PACK 1  // 0: the unit is compiled without the packed round (csrc/Makefile: it would need scratch)
#endif
constexpr int kUPackMax = 3;  // groups of a packed round; four groups are an ordinary unit

// acc[j] += W-slice . column (stream, point 4j + q) over depth 16 NB; xl = X + stream kUImgS + q kUP + 4g.  Blocks, steps
// and weight prefetch distance of u16_gemm_n: every column sums in the order it has in a full unit.
template <int NB, bool COLS>
__device__ __forceinline__ void u16p_gemm_n(f32x4 (&acc)[kUPackMax], int G, const float* W, int ld, unsigned off, f32x4 w0, f32x4 w1, const float* xl) {
  f32x4 wq[3];
  wq[0] = w0;
  wq[1] = w1;
  f32x4 bc[kUPackMax], bn[kUPackMax];
#pragma unroll
  for (int j = 0; j < kUPackMax; ++j) {
    bc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    bn[j] = bc[j];
    if (j < G) bc[j] = *reinterpret_cast<const f32x4*>(xl + 4 * j * kUP);
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    if (b + 2 < NB) wq[(b + 2) % 3] = u16_wload<COLS>(W, ld, off, b + 2);
    if (b + 1 < NB) {
#pragma unroll
      for (int j = 0; j < kUPackMax; ++j)
        if (j < G) bn[j] = *reinterpret_cast<const f32x4*>(xl + 4 * j * kUP + 16 * (b + 1));
    }
#pragma unroll
    for (int j = 0; j < kUPackMax; ++j) {
      if (j < G) {
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[j] = mfma16(wq[b % 3][m], bc[j][m], acc[j]);
      }
    }
    if (b + 1 < NB) {
#pragma unroll
      for (int j = 0; j < kUPackMax; ++j) bc[j] = bn[j];
    }
  }
}

template <bool COLS>
__device__ __forceinline__ void u16p_gemm(f32x4 (&acc)[kUPackMax], int G, const float* W, int ld, unsigned off, f32x4 w0, f32x4 w1, int nb, const float* xl) {
  switch (nb) {
    case 8: u16p_gemm_n<8, COLS>(acc, G, W, ld, off, w0, w1, xl); return;
    case 4: u16p_gemm_n<4, COLS>(acc, G, W, ld, off, w0, w1, xl); return;
    default: break;
  }
#pragma unroll 1
  for (int b = 0; b < nb; ++b) {
    const f32x4 w = b == 0 ? w0 : b == 1 ? w1 : u16_wload<COLS>(W, ld, off, b);
#pragma unroll
    for (int j = 0; j < kUPackMax; ++j) {
      if (j < G) {
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[j] = mfma16(w[m], xl[4 * j * kUP + 16 * b + m], acc[j]);
      }
    }
  }
}

// u16_outer_n on the packed round: the MFMA k index is (stream, point of the group).  Per group K steps, step = stream;
// lane group g supplies point 4j + g: zl = Z + g kUP + 16w + c, al = A + g kUP + c
template <int K, int NA, int OFF, int NPT>
__device__ __forceinline__ void u16p_outer_n(f32x4 (&pt)[NPT], int G, const float* zl, const float* al) {
#pragma unroll
  for (int j = 0; j < kUPackMax; ++j) {
    if (j < G) {
      float zc, zn = 0.0f, ac[NA], an[NA];
      zc = zl[4 * j * kUP];
#pragma unroll
      for (int t = 0; t < NA; ++t) {
        ac[t] = al[4 * j * kUP + 16 * t];
        an[t] = 0.0f;
      }
#pragma unroll
      for (int s = 0; s < K; ++s) {
        if (s + 1 < K) {
          zn = zl[(s + 1) * kUImgS + 4 * j * kUP];
#pragma unroll
          for (int t = 0; t < NA; ++t) an[t] = al[(s + 1) * kUImgS + 4 * j * kUP + 16 * t];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < NA; ++t) pt[OFF + t] = mfma16(zc, ac[t], pt[OFF + t]);
        __builtin_amdgcn_sched_barrier(0);
        if (s + 1 < K) {
          zc = zn;
#pragma unroll
          for (int t = 0; t < NA; ++t) ac[t] = an[t];
        }
      }
    }
  }
}

template <int K, int OFF, int NMAX, int NPT>
__device__ __forceinline__ void u16p_outer(f32x4 (&pt)[NPT], int G, int na, const float* zl, const float* al) {
  if constexpr (NMAX >= 8) {
    if (na * 2 == NMAX) { u16p_outer_n<K, NMAX / 2, OFF, NPT>(pt, G, zl, al); return; }
  }
  u16p_outer_n<K, NMAX, OFF, NPT>(pt, G, zl, al);
}

// the writes of this wave's lanes to LDS are ordered before the reads that follow (rows of the wave's own)
__device__ __forceinline__ void u16_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// forward activation jets of the accumulator (rows 16w + 4g + r, point c); rec gets the tape record
template <int ACT, int NT, int NX, bool MRG = false>
__device__ __forceinline__ void u16_ew_forward(f32x4 (&v)[1 + NT + NX], float w, f32x4 (&rec)[1 + NT + NX], float cc = 0.0f) {
  constexpr int K = 1 + NT + NX;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float z[K], y[K];
#pragma unroll
    for (int s = 0; s < K; ++s) z[s] = v[s][r];
    if constexpr (MRG) act_fwd_merged<ACT>(w, cc, z, y);
    else act_fwd<ACT, NT, NX>(w, z, y);
    rec[0][r] = ActTape<ACT>::value_is_output ? y[0] : z[0];
#pragma unroll
    for (int s = 1; s < K; ++s) rec[s][r] = z[s];
#pragma unroll
    for (int s = 0; s < K; ++s) v[s][r] = y[s];
  }
}

template <int K>
__device__ __forceinline__ void u16_put(float* il, const f32x4 (&v)[K]) {  // il = image + c kUP + 16w + 4g
#pragma unroll
  for (int s = 0; s < K; ++s) *reinterpret_cast<f32x4*>(il + s * kUImgS) = v[s];
}
template <int K>
__device__ __forceinline__ void u16_get(const float* il, f32x4 (&v)[K]) {
#pragma unroll
  for (int s = 0; s < K; ++s) v[s] = *reinterpret_cast<const f32x4*>(il + s * kUImgS);
}

// activation adjoint of the accumulator rows with record rec; MRG: returns the rows' coefficient partials (else 0)
template <int ACT, int NT, int NX, bool MRG = false>
__device__ __forceinline__ float u16_ew_backward(f32x4 (&ab)[1 + NT + NX], float w, const f32x4 (&rec)[1 + NT + NX], float cc = 0.0f) {
  constexpr int K = 1 + NT + NX;
  float part = 0.0f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float z[K], abv[K], zb[K];
#pragma unroll
    for (int s = 0; s < K; ++s) {
      z[s] = rec[s][r];
      abv[s] = ab[s][r];
    }
    if constexpr (MRG) part += act_bwd_tape_merged<ACT>(w, cc, z, abv, zb);
    else act_bwd_tape<ACT, NT, NX>(w, z, abv, zb);
#pragma unroll
    for (int s = 0; s < K; ++s) ab[s][r] = zb[s];
  }
  return part;
}

// replay of activation jets from a tape record, either stream set
template <int ACT, int NT, int NX, bool MRG>
__device__ __forceinline__ void u16_act_replay(float w, float cc, const float* z, float* y) {
  if constexpr (MRG) act_fwd_tape_merged<ACT>(w, cc, z, y);
  else act_fwd_tape<ACT, NT, NX>(w, z, y);
}

// sum over the 64 lanes of a wave of lanes with (lane & 15) == 0 .. 15 folded: every lane gets the sum over its
// 16-lane row (row16_sum) — used for per-feature sums over the points of a unit
__device__ __forceinline__ f32x4 row16_sum4(f32x4 v) {
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = row16_sum(v[r]);
  return v;
}

// Layer l of the fixed shape: compile-time sizes, W and act_param from the kernel's resident copies (fixed-shape units
// only; the gradient pointers are read from the descriptor where the flush uses them).  scalar_sizes: the packed round's
// form, where l is a run-time value and the sizes are scalar registers, so that the round is compiled in the shape it has
// in the generic units (its element-wise code must contract its multiply-adds as theirs does, see the round) and only
// the descriptor reads are gone.
struct U16FixedLayers {  // by value, member by member: an array indexed with the packed round's run-time l would live in scratch
  const float *W0, *W1, *W2;
  float ap0, ap1, ap2;
};
__device__ __forceinline__ LayerDev u16_fixed_layer(const U16FixedLayers f, int l, bool scalar_sizes = false) {
  LayerDev u = {};
  u.W = l == 0 ? f.W0 : l == 1 ? f.W1 : f.W2;
  int in_dim = l == 0 ? kUFixed.in0 : kUFixed.width, out_dim = kUFixed.width;
  if (scalar_sizes) asm("" : "+s"(in_dim), "+s"(out_dim));
  u.in_dim = in_dim;
  u.out_dim = out_dim;
  // The row stride goes through an empty asm: as a constant it is folded into per-lane 64-bit addresses of the column
  // form's loads (u16_wload), which are hoisted out of the unit loop and spilled; as a scalar it stays in the loads'
  // scalar base, as in the generic units.
  int ld = u.in_dim;
  asm("" : "+s"(ld));
  u.ld = ld;
  u.act_param = l == 0 ? f.ap0 : l == 1 ? f.ap1 : f.ap2;
  return u;
}
// The macros below are for the body of jet_kernel_u16 alone (undefined again behind it).  They capture its names net, fix,
// fnull and FIXED.
// the layer descriptor as the kernel body uses it (FIXED is a constant: one arm is compiled)
#define U16_LAYER(l) (FIXED ? u16_fixed_layer(fix, (l)) : uniform_layer(net.layer[(l)]))
#define U16_LAYER_P(l) (FIXED ? u16_fixed_layer(fix, (l), true) : uniform_layer(net.layer[(l)]))  // the packed round's
// whether layer l forms a weight / a bias gradient: the fixed-shape units ask the resident word fnull
#define U16_HAS_DW(l, Ly) (FIXED ? ((fnull >> (l)) & 1u) == 0u : (Ly).dW != nullptr)
#define U16_HAS_DB(l, Ly) (FIXED ? ((fnull >> (4 + (l))) & 1u) == 0u : (Ly).db != nullptr)
// trip count of a layer loop: the fixed-shape units unroll it, the others keep the loop
#define U16_LAYER_UNROLL FIXED ? kPersist : 1

// NA0: 16-feature k-tiles of the first MFMA layer's weight-gradient accumulators (4: at most 64 input features)
// BWD = false: the forward-only launch of the same networks.  It runs the forward code of the reverse launch unchanged,
// so a forward-only call and a fused call give bit-identical per-point results.
// COEF = true (reverse launches only, jet_u16c_* units): inverse problems.  The PDE coefficients come from the device
// array a.pde.coef_dev, read once at kernel start, and the writer lanes also sum rbar dr/dc_0, rbar dr/dc_1; the two
// sums go to a.pde.dcoef in this workgroup's slab row (the padding of the loss-sum slot).  The reverse kernel has no
// VGPR to spare, so neither the coefficients nor the two running sums live in registers across the unit loop: both
// sit in the 4-float row pad of the stream-0 rows of image X, which no GEMM, put or encode touches —
// X[n][128], X[n][129]: the sums of writer lane n (COEF only); X[k][130], k < 4: coefficient c_k (every variant: the
// by-value coefficients are staged there too, so that products of them are formed in the epilogue and not held in
// VGPRs across the unit loop).
//
// MRG = true (jet_u16m_* / jet_u16mc_* units, NT = NX = 1): the merged stream set [value, w, d/dx] of jet_device.h on
// the Burgers residual, K = 3.  Its coefficient c = -c_0 is read from the row pad where it is used.  The merged COEF
// form sums dL/dc per lane in pcl (every activation element's partial, and at layer 0 the Fourier features' through one
// more single-stream abar GEMM) and stores -sum as the cotangent of c_0 in the slab row's slot.
//
// FIXED = true (jet_u16mf_* / jet_u16mfc_* units, merged set only): the shape of the network is compiled in (kUFixed:
// 64 Fourier features of two coordinates, three MFMA layers 64 -> 128 -> 128 -> 128 with ld == in_dim, head 128 -> 1).
// The layer loops of the unit loop are unrolled with a compile-time layer, so widths, image roles, GEMM depths and tile
// offsets are constants and no layer descriptor is read inside the unit loop: the three W pointers, the activation
// parameters and one word that says which gradient pointers are null are read once and stay in scalar registers (the row
// stride too: u16_fixed_layer says why it is not a literal).  The packed round keeps its loops and takes the same
// resident values.  The arithmetic and its order are those of the generic merged unit, which the same descriptor takes
// with PINN_FLAG_GENERIC_UNITS.
template <int ACT, int NT, int NX, bool BWD, int NA0, bool COEF = false, bool MRG = false, bool FIXED = false>
__global__ __launch_bounds__(kUThreads, 1) void jet_kernel_u16(const KernelArgs a) {
  static_assert(!MRG || (NT == 1 && NX == 1), "the merged set is laid out as the (1,1) set");
  static_assert(!FIXED || (MRG && NA0 == kUFixed.in0 / 16), "the fixed shape is a merged unit's");
  constexpr int K = 1 + NT + NX;
  constexpr int NKT = kUH / 16;
  constexpr int NPT = NA0 + (kPersist - 1) * NKT;
  static_assert(kPersist == 3, "the layer -> tile-offset table below is written for three persistent layers");
  constexpr int img = K * kUImgS;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const NetDev& net = a.net;
  float* X = smem;                    // forward activations (ping-pong with A2); zbar in the reverse sweep
  float* A2 = X + img;                // forward activations; the last layer's parked record; reverse sweep: a_{l-1}
  float* REC = A2 + img;              // records of layers 0, 1 (replayed in the reverse sweep)
  // Reverse launches of the merged units keep a fifth image S: the last layer's record is parked there, X and A2 keep
  // the forward activations, and every zbar_l is stored over the record it was computed from (S, REC[l]).
  constexpr bool KEEP = MRG && BWD;
  [[maybe_unused]] float* S = REC + 2 * img;
  float* UP = REC + (KEEP ? 3 : 2) * img;  // kUWaves * K * kU: per-wave partial sums of the output layer
  float* xin2 = UP + kUWaves * K * kU;  // 2 * kMaxDin * kU: coordinates of this unit and of the workgroup's next one
  float* wb = xin2 + 2 * kMaxDin * kU;     // (1 + n_layers) * 128: w_out, then the hidden-layer biases
  float* ep = wb + (1 + kPersist) * kUH;  // (kMaxDin + 1) * 128: encoding parameters
  float* pl = ep + (kMaxDin + 1) * kUH;   // (kPersist + kMaxDin + 1) * 128: per-feature db of the MFMA layers, then the
                                          // first-Linear gradient partials (thread tid < 128 owns feature tid)
  float* pdwl = pl + (kPersist + kMaxDin + 1) * kUH;  // kUThreads * 4: per-lane partial dw_out (reverse launches; no
                                                      // VGPRs to spare for a running sum that B0 alone touches)
  float* psl = pdwl + 4 * kUThreads;  // 2 * kU: running loss and db_out sums of the writer lanes (tid < kU), same reason
  float* xint = psl + 2 * kU;         // kMaxDin * kU: coordinates of the packed round's points (fetched at kernel start)
  [[maybe_unused]] float* pcl = xint + kMaxDin * kU;  // kUThreads: per-lane dL/dc sums (merged COEF units only: not allocated otherwise)
  auto mcoef = [&]() -> float {  // c of the merged set (visible after the unit loop's first barrier)
    if constexpr (MRG) return -X[kUH + 2];
    else return 0.0f;
  };
  auto cadd = [&](float part, bool own) {  // lane-private slot
    if constexpr (MRG && COEF) {
      if (own) pcl[u16_opaque(threadIdx.x)] += part;
    }
  };

  PINN_STAMP_DECL
  const int tid = threadIdx.x;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int g = lane >> 4, c = lane & 15;
  const int din = FIXED ? kUFixed.din : net.din;
  const int nl = FIXED ? kUFixed.layers : net.n_layers;
  // The unit loop's points: a.N, or the whole rounds only when a packed round follows (every unit of the loop is then
  // full).  The loop knows no other point count: one more scalar held across it costs the reverse kernel scratch.
#if PINN_U16_PACK
  const long long NL = a.u16_loop_points;
#else
  const long long NL = a.N;
#endif
  const long long nunits = (NL + kU - 1) / kU;
  const int frow = 16 * wv + 4 * g;  // first of this lane's four accumulator rows
  const int ioff = c * kUP + frow;   // this lane's 16-byte word of an image (point c, rows frow .. frow+3)

  for (int k = tid; k < kUH; k += kUThreads) {
    wb[k] = k < net.h_last ? net.w_out[k] : 0.0f;
    for (int l = 0; l < nl; ++l) wb[(1 + l) * kUH + k] = k < net.layer[l].out_dim ? net.layer[l].b[k] : 0.0f;
  }
  stage_enc_params<kUH>(net, ep, tid);
#pragma unroll
  for (int i = 0; i < kPersist + kMaxDin + 1; ++i)
    if (tid < kUH) pl[i * kUH + tid] = 0.0f;
  const float b_out0 = net.b_out[0];
  static_assert(!COEF || BWD, "coefficient cotangents belong to the reverse launch");
  if constexpr (COEF) {
    if (tid < kU) {
      X[tid * kUP + kUH] = 0.0f;
      X[tid * kUP + kUH + 1] = 0.0f;
    }
  }
  // the coefficients of every launch sit in the row pad (below): values formed from them are then formed in the
  // epilogue, where registers are free, instead of being held (and spilled) across the unit loop
  if (tid < 4) {  // visible after the unit loop's first barrier
    const float cv = tid == 0 ? a.pde.c0 : tid == 1 ? a.pde.c1 : tid == 2 ? a.pde.c2 : a.pde.c3;
    X[tid * kUP + kUH + 2] = COEF ? a.pde.coef_dev[tid] : cv;
  }

  f32x4 pt[NPT];
#pragma unroll
  for (int t = 0; t < NPT; ++t) pt[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  if constexpr (BWD) *reinterpret_cast<f32x4*>(pdwl + 4 * tid) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};  // lane-private
  if (tid < 2 * kU) psl[tid] = 0.0f;  // lane-private from here on: slot tid and slot kU + tid of lane tid < kU
  if constexpr (MRG && COEF) pcl[tid] = 0.0f;

  float xr[kMaxDin] = {0.0f, 0.0f, 0.0f, 0.0f};
  // Merged units: one value per lane of wave 0 instead, coordinate tid >> 4 of point tid & 15 (kMaxDin kU = 64 lanes), and
  // a fetch is one unconditional load with no wait behind it.  The address is selected arithmetically between x and t; a
  // lane without a coordinate (past din, or a point past the end) loads t[0].  xv holds the raw word: whether it counts
  // is decided again at its store (mput), so that nothing uses the loaded register before then.  x may be null when
  // din == 1: no lane selects it then.  Lane indices come from an opaque copy of tid: nothing is held across the unit loop.
  [[maybe_unused]] float xv = 0.0f;
  static_assert(kMaxDin * kU == 64, "the merged units' coordinate lanes are wave 0");
  auto mfetch = [&](long long p, bool ok) {  // wave 0; p, ok: the lane's point and whether it exists
    const int cc = u16_opaque(tid) >> 4;
    const bool live = ok && cc < din;
    const bool space = live && cc < din - 1;
    unsigned long long bx = reinterpret_cast<unsigned long long>(a.x), bt = reinterpret_cast<unsigned long long>(a.t);
    // both pointers in scalar registers: left to itself the optimizer selects between the two kernel-argument slots per
    // lane and reads the pointer with a vector load, a second round trip ahead of the coordinate's
    asm volatile("" : "+s"(bx), "+s"(bt));
    // index p (din - 1) + cc into x, p into t, 0 for a lane without a coordinate: one multiply-add, no branch
    const long long idx = p * (space ? din - 1 : live ? 1 : 0) + (space ? cc : 0);
    // (a global pointer: formed from an integer it would otherwise be a flat one, whose load also counts in lgkmcnt)
    using gfloat = const float __attribute__((address_space(1)));
    xv = *(gfloat*)(bt + (space ? bx - bt : 0ull) + 4ull * static_cast<unsigned long long>(idx));
  };
  auto mput = [&](float* dst, bool ok) {  // dst[cc kU + point]
    const int to = u16_opaque(tid);
    dst[to] = ok && (to >> 4) < din ? xv : 0.0f;
  };
  auto unit_point = [&](long long u, bool& ok) -> long long {
    const long long p = u * kU + (u16_opaque(tid) & 15);
    ok = u < nunits && p < NL;
    return p;
  };
  auto at_point = [&](long long p0, int npts, bool& ok) -> long long {
    const int n = u16_opaque(tid) & 15;
    ok = n < npts && p0 + n < a.N;
    return p0 + n;
  };
  // u: the unit whose coordinates are requested; merged units store those of unit us (requested earlier)
  auto fetch_coords = [&](long long u) {
    if constexpr (MRG) {
      if (wv == 0) {
        bool ok;
        const long long p = unit_point(u, ok);
        mfetch(p, ok);
      }
    } else if (tid < kU) {
      const long long p = u * kU + tid;
      const bool ok = u < nunits && p < NL;
#pragma unroll
      for (int cc = 0; cc < kMaxDin; ++cc) {
        if (cc < din - 1) xr[cc] = ok ? a.x[p * (din - 1) + cc] : 0.0f;
        if (cc == din - 1) xr[cc] = ok ? a.t[p] : 0.0f;
      }
    }
  };
  auto fetch_coords_at = [&](long long p0, int npts) {  // points p0 .. p0 + npts - 1 (npts <= kU)
    if constexpr (MRG) {
      if (wv == 0) {
        bool ok;
        const long long p = at_point(p0, npts, ok);
        mfetch(p, ok);
      }
    } else if (tid < kU) {
      const long long p = p0 + tid;
      const bool ok = tid < npts && p < a.N;
#pragma unroll
      for (int cc = 0; cc < kMaxDin; ++cc) {
        if (cc < din - 1) xr[cc] = ok ? a.x[p * (din - 1) + cc] : 0.0f;
        if (cc == din - 1) xr[cc] = ok ? a.t[p] : 0.0f;
      }
    }
  };
  auto put_xr = [&](float* dst) {  // the other units: what the last fetch left in xr
    if (tid < kU) {
#pragma unroll
      for (int cc = 0; cc < kMaxDin; ++cc) dst[cc * kU + tid] = xr[cc];
    }
  };
  auto put_coords = [&](float* dst, [[maybe_unused]] long long us) {  // of unit us
    if constexpr (MRG) {
      if (wv == 0) {
        bool ok;
        unit_point(us, ok);
        mput(dst, ok);
      }
    } else {
      put_xr(dst);
    }
  };
  auto put_coords_at = [&](float* dst, [[maybe_unused]] long long p0, [[maybe_unused]] int npts) {  // of fetch_coords_at
    if constexpr (MRG) {
      if (wv == 0) {
        bool ok;
        at_point(p0, npts, ok);
        mput(dst, ok);
      }
    } else {
      put_xr(dst);
    }
  };
#if PINN_U16_PACK
  if (a.u16_tail_groups > 0) {  // the packed round's coordinates: visible long before the round's first barrier
    const long long tp0 = a.u16_loop_points + 4LL * a.u16_tail_groups * blockIdx.x;
    fetch_coords_at(tp0, 4 * a.u16_tail_groups);
    put_coords_at(xint, tp0, 4 * a.u16_tail_groups);
  }
#endif
  fetch_coords(blockIdx.x);
  put_coords(xin2, blockIdx.x);
  // Merged units: xv holds the coordinates of the workgroup's next unit from here on.  Unit u stores them behind its
  // first GEMM (as every unit does) and requests those of the unit after next behind its LAST forward GEMM.  vmcnt counts
  // in order, so the first vmcnt wait behind a request waits for the cold load as well, whatever it was written for.
  // Behind the last forward GEMM no weight request follows in the forward sweep; in the compiled kernel the first such
  // wait is one the compiler places behind the output layer's barrier (it guards registers of earlier weight requests),
  // so the load has the last layer's jets, the output layer and that barrier to land.  That is not quite enough: about
  // 350 cycles per unit stay exposed on wave 0, against 2 000 at the unit top (profiles/r10_wave0_chains.md).
  if constexpr (MRG) fetch_coords(blockIdx.x + gridDim.x);
  // Fixed-shape units: what the unit loop and the packed round need of the layer table, read here once.  The values go
  // through an empty asm so that they are kept in scalar registers instead of being read again at every use.
  [[maybe_unused]] U16FixedLayers fix = {};
  [[maybe_unused]] unsigned fnull = 0u;  // bit l: layer l has no dW, bit 4 + l: no db
  if constexpr (FIXED) {
    auto resident_w = [&](int l) -> const float* {
      unsigned long long wp = reinterpret_cast<unsigned long long>(net.layer[l].W);
      asm("" : "+s"(wp));
      using gfloat = const float __attribute__((address_space(1)));
      return (const float*)(gfloat*)wp;
    };
    auto resident_ap = [&](int l) -> float {
      unsigned ap = __float_as_uint(net.layer[l].act_param);
      asm("" : "+s"(ap));
      return __uint_as_float(ap);
    };
    fix = {resident_w(0), resident_w(1), resident_w(2), resident_ap(0), resident_ap(1), resident_ap(2)};
#pragma unroll
    for (int l = 0; l < kPersist; ++l) fnull |= (net.layer[l].dW ? 0u : 1u << l) | (net.layer[l].db ? 0u : 16u << l);
    asm("" : "+s"(fnull));
  }
  int xpar = 0;

  for (long long u = blockIdx.x; u < nunits; u += gridDim.x) {
    const long long p0 = u * kU;
    // previous unit's readers of X / A2 / UP are done; this unit's coordinates (stored during the previous unit, into
    // the half of xin2 that unit did not read) are visible
    U16_BARRIER(ST_BWD_FLUSH);
    const float* xin = xin2 + xpar * (kMaxDin * kU);
    float* xin_next = xin2 + (xpar ^ 1) * (kMaxDin * kU);
    xpar ^= 1;
    if constexpr (!MRG) fetch_coords(u + gridDim.x);
    f32x4 w0, w1;  // first two weight blocks of the next GEMM, requested a phase ahead
    {
      const LayerDev L0 = U16_LAYER(0);
      const unsigned off = u16_rows_off(16 * wv < L0.out_dim ? 16 * wv : 0, L0.ld, c, g);
      w0 = u16_wload<false>(L0.W, L0.ld, off, 0);
      w1 = u16_wload<false>(L0.W, L0.ld, off, L0.in_dim > 16 ? 1 : 0);
    }
    PINN_STAMP(ST_STAGE);
    // The forward sweep ping-pongs between X and A2: layer l reads one image and puts its activations into the other,
    // so a layer boundary is one barrier.  The encoding goes where the parity of n_layers makes the LAST layer read X:
    // its record is then parked in A2 and the reverse sweep finds zbar -> X, a_{l-1} -> A2 for every n_layers.
    // The merged units have static roles instead: the encoding in X, a_l in A2 for even l and in X for odd l, the last
    // layer's record in S; their reverse sweep reads the activations where the forward sweep left them.
    float* src = (MRG || (nl & 1)) ? X : A2;
    float* dst = (MRG || (nl & 1)) ? A2 : X;
    u16_encode<ACT, NT, NX, MRG, FIXED>(net, ep, xin, src, u16_opaque(tid), mcoef());  // opaque: addresses formed here, not held over the loop
    U16_BARRIER(ST_ENCODE);

    // ---- hidden layers ----
    f32x4 acc[K];
#pragma unroll U16_LAYER_UNROLL
    for (int l = 0; l < nl; ++l) {
      const LayerDev Ly = U16_LAYER(l);
      const bool on = FIXED || 16 * wv < Ly.out_dim;
      const bool last = l + 1 == nl;
#pragma unroll
      for (int s = 0; s < K; ++s) acc[s] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      if (on) {
        u16_gemm<K, false>(acc, Ly.W, Ly.ld, u16_rows_off(16 * wv, Ly.ld, c, g), w0, w1, Ly.in_dim >> 4, src + c * kUP + 4 * g);
        acc[0] += *reinterpret_cast<const f32x4*>(wb + (1 + l) * kUH + frow);
      }
      if (l == 0) {
        // the loads had the encoding and a GEMM to land (merged units: a whole unit); last read two barriers ago
        put_coords(xin_next, u + gridDim.x);
      }
      if constexpr (MRG) {
        if (last) fetch_coords(u + 2 * gridDim.x);  // behind the store above: xv is free
      }
      PINN_STAMP(ST_FWD_GEMM);
      if (!last) {
        {
          const LayerDev Ln = U16_LAYER(l + 1);
          const unsigned off = u16_rows_off(16 * wv < Ln.out_dim ? 16 * wv : 0, Ln.ld, c, g);
          w0 = u16_wload<false>(Ln.W, Ln.ld, off, 0);  // latency hides under the jets
          w1 = u16_wload<false>(Ln.W, Ln.ld, off, Ln.in_dim > 16 ? 1 : 0);
        }
        if (on) {  // the record goes to this wave's own columns: nobody else reads them in the forward sweep
          f32x4 rec[K];
          u16_ew_forward<ACT, NT, NX, MRG>(acc, Ly.act_param, rec, mcoef());
          if constexpr (BWD) u16_put<K>(REC + l * img + ioff, rec);
        }
        // dst was last read a barrier ago (by the GEMMs of layer l-1, or by the previous unit's reverse sweep)
        if (on) u16_put<K>(dst + ioff, acc);
        U16_BARRIER(ST_FWD_EW);
        float* const t = src;
        src = dst;
        dst = t;
      } else if (on) {  // last hidden layer: activations stay in acc, the record is parked in this wave's columns of A2
        f32x4 rec[K];   // (merged units: of S)
        u16_ew_forward<ACT, NT, NX, MRG>(acc, Ly.act_param, rec, mcoef());
        if constexpr (BWD) u16_put<K>((KEEP ? S : A2) + ioff, rec);
      }
    }
    PINN_STAMP(ST_FWD_EW);

    // ---- output layer (H_last -> 1): lane partials -> wave partials in LDS -> every lane sums ----
    {
      const f32x4 w4 = *reinterpret_cast<const f32x4*>(wb + frow);
      float po[K];
#pragma unroll
      for (int s = 0; s < K; ++s) {
        po[s] = fmaf(w4[0], acc[s][0], fmaf(w4[1], acc[s][1], fmaf(w4[2], acc[s][2], w4[3] * acc[s][3])));
        po[s] += __shfl_xor(po[s], 16);
        po[s] += __shfl_xor(po[s], 32);
      }
      if (g == 0) {
#pragma unroll
        for (int s = 0; s < K; ++s) UP[(wv * K + s) * kU + c] = po[s];
      }
    }
    U16_BARRIER(ST_OUT);

    // ---- epilogue, evaluated by every lane for its point c (32 lanes per point, same values) ----
    float ub[K];
    {
      const long long p = p0 + c;
      const bool ok = p < NL;
      const bool writer = tid < kU;
      float j[K];
#pragma unroll
      for (int s = 0; s < K; ++s) {
        float v = s == 0 ? b_out0 : 0.0f;
#pragma unroll
        for (int w = 0; w < kUWaves; ++w) v += UP[(w * K + s) * kU + c];
        j[s] = v;
      }
      if (!FIXED && a.mode == MODE_JETS) {
#pragma unroll
        for (int s = 0; s < K; ++s) {
          if (writer && ok && a.jets_out[s]) a.jets_out[s][p] = j[s];
          ub[s] = (BWD && ok && a.jets_bar[s]) ? a.jets_bar[s][p] : 0.0f;
        }
      } else {
        float d[K];
        PdeDev pde = a.pde;
        pde.c0 = X[0 * kUP + kUH + 2];
        pde.c1 = X[1 * kUP + kUH + 2];
        pde.c2 = X[2 * kUP + kUH + 2];
        pde.c3 = X[3 * kUP + kUH + 2];
        float r;
        if constexpr (MRG) r = pde_residual_merged(j, d);
        else r = pde_residual<NT, NX>(pde, j, xin[c], d);
        float dl;
        float lt = loss_term(pde, r, &dl);
        if (!ok) {
          lt = 0.0f;
          dl = 0.0f;
        }
        if (writer && ok && a.residual_out) a.residual_out[p] = r;
        if (writer) psl[c] += lt;
        const float rb = !BWD ? 0.0f : a.res_bar ? (ok ? a.res_bar[p] : 0.0f) : a.grad_scale * dl;
#pragma unroll
        for (int s = 0; s < K; ++s) ub[s] = rb * d[s];
        if constexpr (COEF && !MRG) {
          float dc0, dc1;
          pde_coef_grads<NT, NX>(pde, j, xin[c], dc0, dc1);
          if (writer) {  // lane-private LDS slots (tid < kU: c == tid)
            X[c * kUP + kUH] += rb * dc0;
            X[c * kUP + kUH + 1] += rb * dc1;
          }
        }
      }
    }

    PINN_STAMP(ST_EPI);
    if constexpr (!BWD) continue;
    // ---- B0: output layer.  dw_out partials stay per lane; abar = w_out (x) ub, then the last layer's adjoint ----
    if (tid < kU) psl[kU + c] += ub[0];
    f32x4 ab[K];
    {
      const LayerDev Lz = U16_LAYER(nl - 1);
      const f32x4 w4 = *reinterpret_cast<const f32x4*>(wb + frow);
#pragma unroll
      for (int s = 0; s < K; ++s) ab[s] = w4 * ub[s];
      if (16 * wv < Lz.out_dim) {
        f32x4 rec[K];
        u16_get<K>((KEEP ? S : A2) + ioff, rec);
        float* const pdwp = pdwl + 4 * u16_opaque(tid);
        f32x4 pdw = *reinterpret_cast<const f32x4*>(pdwp);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float z[K], y[K];
#pragma unroll
          for (int s = 0; s < K; ++s) z[s] = rec[s][r];
          if constexpr (KEEP) {  // the last layer's activations are still in acc
#pragma unroll
            for (int s = 0; s < K; ++s) y[s] = acc[s][r];
          } else {
            u16_act_replay<ACT, NT, NX, MRG>(Lz.act_param, mcoef(), z, y);
          }
          float gg = 0.0f;
#pragma unroll
          for (int s = 0; s < K; ++s) gg = fmaf(ub[s], y[s], gg);
          pdw[r] += gg;
        }
        *reinterpret_cast<f32x4*>(pdwp) = pdw;
        cadd(u16_ew_backward<ACT, NT, NX, MRG>(ab, Lz.act_param, rec, mcoef()), true);
        // zbar of the last layer goes over the record it came from: that word is this lane's alone
        if constexpr (KEEP) u16_put<K>(S + ioff, ab);
      }
    }
    PINN_STAMP(ST_B0);

#pragma unroll U16_LAYER_UNROLL
    for (int l = nl - 1; l >= 0; --l) {
      const LayerDev Ly = U16_LAYER(l);
      const bool on = FIXED || 16 * wv < Ly.out_dim;
      const bool need_abar = l > 0 || (!FIXED && net.enc == ENC_LINEAR);
      const bool kon = 16 * wv < Ly.in_dim;  // this wave owns input-feature rows of the layer
      // the GEMMs of layer l+1 have finished reading X (zbar) and A2; with a single MFMA layer the barrier keeps
      // u16_encode (all columns of A2, below) from overwriting another wave's parked record before its B0 has read it
      if constexpr (!KEEP) {
        if (l + 1 < nl || nl == 1) U16_BARRIER(ST_BWD_EW);
        if (on) u16_put<K>(X + ioff, ab);
      }
      // The layer's operands: zbar_l in ZB, a_{l-1} in AP.  Merged units: zbar_l lies over the record of layer l (B0 and
      // the adjoint behind layer l+1's abar GEMM stored it there) and a_{l-1} where the forward sweep put it, so the
      // layer needs no put, no replay and one barrier (DESIGN.md §4.1 lists every interval's readers and writers).
      const float* const ZB = !KEEP ? X : l + 1 == nl ? S : REC + l * img;
      const float* const AP = !KEEP || (l & 1) ? A2 : X;
      float pw = 0.0f;  // act_param of layer l-1
      if constexpr (KEEP) {
        if (l > 0) pw = U16_LAYER(l - 1).act_param;
      } else if (l > 0) {
        const LayerDev P = U16_LAYER(l - 1);
        pw = P.act_param;
        if (kon) {  // replay a_{l-1} from its record into this wave's columns of A2
          f32x4 rec[K], y[K];
          u16_get<K>(REC + (l - 1) * img + ioff, rec);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float z[K], yy[K];
#pragma unroll
            for (int s = 0; s < K; ++s) z[s] = rec[s][r];
            u16_act_replay<ACT, NT, NX, MRG>(pw, mcoef(), z, yy);
#pragma unroll
            for (int s = 0; s < K; ++s) y[s][r] = yy[s];
          }
          u16_put<K>(A2 + ioff, y);
        }
      } else {
        u16_encode<ACT, NT, NX, MRG, FIXED>(net, ep, xin, A2, u16_opaque(tid), mcoef());
      }
      const unsigned coff = u16_cols_off(kon ? 16 * wv : 0, Ly.ld, c, g);
      if (need_abar) {  // requests hide under the barrier
        w0 = u16_wload<true>(Ly.W, Ly.ld, coff, 0);
        w1 = u16_wload<true>(Ly.W, Ly.ld, coff, 1);
      }
      U16_BARRIER(ST_BWD_PUT);
      if (U16_HAS_DB(l, Ly) && tid < Ly.out_dim) {
        float gsum = 0.0f;
#pragma unroll
        for (int n = 0; n < kU; ++n) gsum += ZB[n * kUP + tid];
        pl[l * kUH + tid] += gsum;
      }
      PINN_STAMP(ST_BWD_DB);
      // The two GEMMs of the layer read only LDS and weights and do not depend on each other, and the activation
      // adjoint of layer l-1 needs only abar and the wave's own record columns.  The SIMD partners (waves w and w + 4)
      // take them in opposite order, so that each one's adjoint (VALU) runs beside a GEMM of the other:
      //   waves 0-3: abar, adjoint, dW        waves 4-7: dW, abar, adjoint
      // No accumulator changes its summation order.
      const bool dw_first = wv >= 4;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        // dW (persistent tiles): first for waves 4-7, last for waves 0-3
        if ((half == 0) == dw_first && on && U16_HAS_DW(l, Ly)) {
          const float* zl = ZB + 4 * g * kUP + 16 * wv + c;
          const float* al = AP + 4 * g * kUP + c;
          const int na = Ly.in_dim >> 4;
          if (l == 0) u16_outer<K, 0, NA0, NPT>(pt, na, zl, al);
          else if (l == 1) u16_outer<K, NA0, NKT, NPT>(pt, na, zl, al);
          else u16_outer<K, NA0 + NKT, NKT, NPT>(pt, na, zl, al);
        }
        if ((half == 0) == dw_first) PINN_STAMP(ST_BWD_STREAM);
        if (half == 1) break;
        // abar_{l-1} = W^T zbar for all streams
        if (need_abar) {
#pragma unroll
          for (int s = 0; s < K; ++s) ab[s] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
          if (kon) u16_gemm<K, true>(ab, Ly.W, Ly.ld, coff, w0, w1, Ly.out_dim >> 4, ZB + c * kUP + 4 * g);
        }
        PINN_STAMP(ST_BWD_DX);
        // activation adjoint of layer l-1; the record is read here, not ahead of a GEMM
        if (l > 0 && kon) {
          f32x4 rec[K];
          u16_get<K>(REC + (l - 1) * img + ioff, rec);
          cadd(u16_ew_backward<ACT, NT, NX, MRG>(ab, pw, rec, mcoef()), true);
          if constexpr (KEEP) u16_put<K>(REC + (l - 1) * img + ioff, ab);  // zbar_{l-1} over its record: this lane's word
        }
        PINN_STAMP(ST_BWD_EW);
      }
      if constexpr (KEEP) {
        // Three MFMA layers: a_1 has taken the encoding's place in X.  dW_2 was X's last reader (a barrier ago), dW_0
        // reads the encoding behind the next barrier: it is formed again here, beside the partner wave's GEMMs.
        if (l == 1 && nl > 2) {
          u16_encode<ACT, NT, NX, MRG, FIXED>(net, ep, xin, X, u16_opaque(tid), mcoef());
          PINN_STAMP(ST_ENCODE);
        }
      }
      if constexpr (MRG && COEF) {
        // Fourier features depend on c through their w stream: dL/dc += sum_j abar_w,j e_j with e_j = -b_x^2 (value
        // feature j).  abar_w = W0^T zbar_w is one single-stream GEMM; the value features are stream 0 of the encoding.
        if (l == 0 && (FIXED || net.enc == ENC_FOURIER) && kon) {
          f32x4 aw[1] = {f32x4{0.0f, 0.0f, 0.0f, 0.0f}};
          {  // a rolled loop: the unrolled, prefetching form of u16_gemm_n costs this unit scratch
            const float* xl = ZB + kUImgS + c * kUP + 4 * g;
            const int nb = Ly.out_dim >> 4;
#pragma unroll 1
            for (int b = 0; b < nb; ++b) {
              const f32x4 w = u16_wload<true>(Ly.W, Ly.ld, coff, b);
              const f32x4 xv = *reinterpret_cast<const f32x4*>(xl + 16 * b);
#pragma unroll
              for (int m = 0; m < 4; ++m) aw[0] = mfma16(w[m], xv[m], aw[0]);
            }
          }
          const int M = FIXED ? kUFixed.enc_out >> 1 : net.enc_out >> 1;
          const f32x4 val = *reinterpret_cast<const f32x4*>(AP + ioff);
          float part = 0.0f;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int jf = frow + r;
            part = fmaf(aw[0][r], fourier_coef_partial_merged(ep[jf < M ? jf : jf - M], val[r]), part);
          }
          cadd(part, true);
        }
      }
    }

    // ---- encoding backward (first Linear of feedforward / SIREN) ----
    if (!FIXED && net.enc == ENC_LINEAR && (net.d_encW || (MRG && COEF))) {
      const int H = net.enc_out;
      // merged COEF units run the adjoint for its coefficient partials even without a first-Linear gradient to form
      const bool enc_sums = !(MRG && COEF) || net.d_encW != nullptr;
      U16_BARRIER(ST_ENC_BWD);
      if (16 * wv < H) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float z[K], abv[K], zb[K];
          u16_enc_preact<NT, NX>(ep, din, xin, frow + r, c, z);
#pragma unroll
          for (int s = 0; s < K; ++s) abv[s] = ab[s][r];
          if constexpr (MRG) cadd(act_bwd_merged<ACT>(net.enc_param, mcoef(), z, abv, zb), true);
          else act_bwd<ACT, NT, NX>(net.enc_param, z, abv, zb);
#pragma unroll
          for (int s = 0; s < K; ++s) ab[s][r] = zb[s];
        }
        if (enc_sums) u16_put<K>(X + ioff, ab);
      }
      U16_BARRIER(ST_ENC_BWD);
      const int te = u16_opaque(tid);  // keeps the pl addresses below out of the unit loop's live registers
      if (enc_sums && te < H) {
        float gb = 0.0f, gt = 0.0f, gx = 0.0f;
        float gw[kMaxDin] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
        for (int n = 0; n < kU; ++n) {
          const float vv = X[n * kUP + te];
          gb += vv;
#pragma unroll
          for (int cc = 0; cc < kMaxDin; ++cc)
            if (cc < din) gw[cc] = fmaf(vv, xin[cc * kU + n], gw[cc]);
          if constexpr (NT >= 1) gt += X[1 * kUImgS + n * kUP + te];
          if constexpr (NX >= 1) gx += X[(1 + NT) * kUImgS + n * kUP + te];
        }
#pragma unroll
        for (int cc = 0; cc < kMaxDin; ++cc) pl[(kPersist + cc) * kUH + te] += gw[cc] + (cc == din - 1 ? gt : 0.0f) + (cc == 0 ? gx : 0.0f);
        pl[(kPersist + kMaxDin) * kUH + te] += gb;
      }
      PINN_STAMP(ST_ENC_BWD);
    }
  }

#if PINN_U16_PACK
  // ---- the packed round: G = a.u16_tail_groups groups of 4 points x K streams (top of the file), on the points whose
  // coordinates were fetched into xint at kernel start.  The phases, images and barriers of a unit; the GEMMs work on
  // (stream, point) columns and the element-wise phases on points, so between the two a wave passes its accumulators
  // through its own columns of an image: lane (g, c) stores rows 16w + 4g .. + 3 of column c and loads them back for point
  // 4j + (c & 3), all streams.  The four lanes c >> 2 = 0 .. 3 of a point then run the unit's element-wise code on
  // the same values and store the same words.  Nothing here is live across the unit loop besides pt[] and the
  // running sums in LDS: addresses come from an opaque copy of the thread index.
  // The fixed-shape units keep the round's layer loops rolled, with the sizes in scalar registers (U16_LAYER_P): unrolled
  // with compile-time sizes the compiler contracted the round's jets differently, and some of its points rounded to
  // other bits than in the generic units (the unit loop's did not).  The round is a quarter unit once per launch.
  if (a.u16_tail_groups > 0) {
    const int G = a.u16_tail_groups;
    const int tp = u16_opaque(tid);
    const int gp = (tp & 63) >> 4, cp = tp & 15;
    const int sp = cp >> 2, qp = cp & 3;       // stream and point-in-group of this lane's MFMA column
    const int frowp = 16 * wv + 4 * gp;
    const int boff = (sp < K ? sp : 0) * kUImgS + qp * kUP + 4 * gp;  // B operand of group 0, block 0 (K < 4: idle columns repeat stream 0)
    const int woff = sp * kUImgS + qp * kUP + frowp;                  // this lane's accumulator word of group 0
    const int eoff = qp * kUP + frowp;                                // element-wise word of group 0 (point qp, rows frowp .. + 3)
    const bool wcol = sp < K;
    const bool writer = tp < 4;  // owns point 4j + tp of every group
    const long long tail_p0 = a.u16_loop_points + 4LL * G * blockIdx.x;
    auto acc_put = [&](float* im, const f32x4 (&pa)[kUPackMax]) {
#pragma unroll
      for (int j = 0; j < kUPackMax; ++j)
        if (j < G && wcol) *reinterpret_cast<f32x4*>(im + woff + 4 * j * kUP) = pa[j];
      u16_wave_sync();
    };

    // the last unit's readers of X / A2 / UP are done; the round's coordinates are visible
    U16_BARRIER(ST_BWD_FLUSH);
    const float* xin = xint;
    f32x4 w0, w1;
    {
      const LayerDev L0 = U16_LAYER_P(0);
      const unsigned off = u16_rows_off(16 * wv < L0.out_dim ? 16 * wv : 0, L0.ld, cp, gp);
      w0 = u16_wload<false>(L0.W, L0.ld, off, 0);
      w1 = u16_wload<false>(L0.W, L0.ld, off, L0.in_dim > 16 ? 1 : 0);
    }
    PINN_STAMP(ST_STAGE);
    float* src = (nl & 1) ? X : A2;
    float* dst = (nl & 1) ? A2 : X;
    u16_encode<ACT, NT, NX, MRG, FIXED>(net, ep, xin, src, tp, mcoef());
    U16_BARRIER(ST_ENCODE);

    // ---- hidden layers; the last one leaves its output-layer partials in UP ----
#pragma unroll 1
    for (int l = 0; l < nl; ++l) {
      const LayerDev Ly = U16_LAYER_P(l);
      const bool on = 16 * wv < Ly.out_dim;
      const bool last = l + 1 == nl;
      f32x4 pa[kUPackMax];
#pragma unroll
      for (int j = 0; j < kUPackMax; ++j) pa[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      if (on) u16p_gemm<false>(pa, G, Ly.W, Ly.ld, u16_rows_off(16 * wv, Ly.ld, cp, gp), w0, w1, Ly.in_dim >> 4, src + boff);
      PINN_STAMP(ST_FWD_GEMM);
      if (!last) {
        const LayerDev Ln = U16_LAYER_P(l + 1);
        const unsigned off = u16_rows_off(16 * wv < Ln.out_dim ? 16 * wv : 0, Ln.ld, cp, gp);
        w0 = u16_wload<false>(Ln.W, Ln.ld, off, 0);
        w1 = u16_wload<false>(Ln.W, Ln.ld, off, Ln.in_dim > 16 ? 1 : 0);
      }
      // dst (the last layer: A2) was last read a barrier ago; its columns 16w .. 16w+15 are this wave's until the next one
      if (on) acc_put(dst, pa);
      const f32x4 bias = *reinterpret_cast<const f32x4*>(wb + (1 + l) * kUH + frowp);
      const f32x4 w4 = *reinterpret_cast<const f32x4*>(wb + frowp);
#pragma unroll
      for (int j = 0; j < kUPackMax; ++j) {
        if (j < G) {
          // The two branches repeat the unit's: the jets of a layer stand in the code once with the record and image
          // stores behind them and once with the record store and the output layer behind them, so the compiler pairs
          // and contracts their arithmetic as it does there, and a point's jets round as in a unit.
          f32x4 v[K];
#pragma unroll
          for (int s = 0; s < K; ++s) v[s] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
          if (!last) {
            if (on) {
              u16_get<K>(dst + eoff + 4 * j * kUP, v);
              v[0] += bias;
              f32x4 rec[K];
              u16_ew_forward<ACT, NT, NX, MRG>(v, Ly.act_param, rec, mcoef());
              if constexpr (BWD) u16_put<K>(REC + l * img + eoff + 4 * j * kUP, rec);
              u16_put<K>(dst + eoff + 4 * j * kUP, v);
            }
          } else if (on) {
            u16_get<K>(dst + eoff + 4 * j * kUP, v);
            v[0] += bias;
            f32x4 rec[K];
            u16_ew_forward<ACT, NT, NX, MRG>(v, Ly.act_param, rec, mcoef());
            if constexpr (BWD) u16_put<K>(A2 + eoff + 4 * j * kUP, rec);  // parked record
          }
          if (last) {  // output layer (H_last -> 1): the unit's reduction order
            float po[K];
#pragma unroll
            for (int s = 0; s < K; ++s) {
              po[s] = fmaf(w4[0], v[s][0], fmaf(w4[1], v[s][1], fmaf(w4[2], v[s][2], w4[3] * v[s][3])));
              po[s] += __shfl_xor(po[s], 16);
              po[s] += __shfl_xor(po[s], 32);
            }
            if (gp == 0 && sp == 0) {
#pragma unroll
              for (int s = 0; s < K; ++s) UP[(wv * K + s) * kU + 4 * j + qp] = po[s];
            }
          }
        }
      }
      if (!last) {
        U16_BARRIER(ST_FWD_EW);
        float* const t = src;
        src = dst;
        dst = t;
      }
    }
    U16_BARRIER(ST_OUT);

    // ---- epilogue and B0, group by group: by every lane for point 4 jg + qp.  One loop, not unrolled: the epilogue
    // stands in the code once, followed by B0 or by nothing, as it does in a unit.  The adjoint of a group waits for
    // the next barrier in this wave's own columns of an image nobody else reads (park), not in registers: first where
    // the parked record was ----
    [[maybe_unused]] const float* park = A2;
#pragma unroll 1
    for (int jg = 0; jg < G; ++jg) {
      float ub[K];
      const int pp = 4 * jg + qp;
      {
        const long long p = tail_p0 + pp;
        const bool ok = p < a.N;
        float j[K];
#pragma unroll
        for (int s = 0; s < K; ++s) {
          float v = s == 0 ? b_out0 : 0.0f;
#pragma unroll
          for (int w = 0; w < kUWaves; ++w) v += UP[(w * K + s) * kU + pp];
          j[s] = v;
        }
        if (!FIXED && a.mode == MODE_JETS) {
#pragma unroll
          for (int s = 0; s < K; ++s) {
            if (writer && ok && a.jets_out[s]) a.jets_out[s][p] = j[s];
            ub[s] = (BWD && ok && a.jets_bar[s]) ? a.jets_bar[s][p] : 0.0f;
          }
        } else {
          float d[K];
          PdeDev pde = a.pde;
          pde.c0 = X[0 * kUP + kUH + 2];
          pde.c1 = X[1 * kUP + kUH + 2];
          pde.c2 = X[2 * kUP + kUH + 2];
          pde.c3 = X[3 * kUP + kUH + 2];
          float r;
          if constexpr (MRG) r = pde_residual_merged(j, d);
          else r = pde_residual<NT, NX>(pde, j, xin[pp], d);
          float dl;
          float lt = loss_term(pde, r, &dl);
          if (!ok) {
            lt = 0.0f;
            dl = 0.0f;
          }
          if (writer && ok && a.residual_out) a.residual_out[p] = r;
          if (writer) psl[pp] += lt;
          const float rb = !BWD ? 0.0f : a.res_bar ? (ok ? a.res_bar[p] : 0.0f) : a.grad_scale * dl;
#pragma unroll
          for (int s = 0; s < K; ++s) ub[s] = rb * d[s];
          if constexpr (COEF && !MRG) {
            float dc0, dc1;
            pde_coef_grads<NT, NX>(pde, j, xin[pp], dc0, dc1);
            if (writer) {
              X[pp * kUP + kUH] += rb * dc0;
              X[pp * kUP + kUH + 1] += rb * dc1;
            }
          }
        }
      }
      PINN_STAMP(ST_EPI);
      if constexpr (!BWD) continue;
      // ---- B0 ----
      if (writer) psl[kU + pp] += ub[0];
      f32x4 ab[K];
      {
        const LayerDev Lz = U16_LAYER_P(nl - 1);
        const f32x4 w4 = *reinterpret_cast<const f32x4*>(wb + frowp);
#pragma unroll
        for (int s = 0; s < K; ++s) ab[s] = w4 * ub[s];
        if (16 * wv < Lz.out_dim) {
          f32x4 rec[K];
          float* const rp = A2 + eoff + 4 * jg * kUP;
          u16_get<K>(rp, rec);
          if (sp == 0) {  // one of the point's four lanes adds its dw_out terms
            float* const pdwp = pdwl + 4 * tp;
            f32x4 pdw = *reinterpret_cast<const f32x4*>(pdwp);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              float z[K], y[K];
#pragma unroll
              for (int s = 0; s < K; ++s) z[s] = rec[s][r];
              u16_act_replay<ACT, NT, NX, MRG>(Lz.act_param, mcoef(), z, y);
              float gg = 0.0f;
#pragma unroll
              for (int s = 0; s < K; ++s) gg = fmaf(ub[s], y[s], gg);
              pdw[r] += gg;
            }
            *reinterpret_cast<f32x4*>(pdwp) = pdw;
          }
          cadd(u16_ew_backward<ACT, NT, NX, MRG>(ab, Lz.act_param, rec, mcoef()), sp == 0);
          u16_put<K>(rp, ab);
        }
      }
      PINN_STAMP(ST_B0);
    }

    if constexpr (BWD) {
#pragma unroll 1
      for (int l = nl - 1; l >= 0; --l) {
        const LayerDev Ly = U16_LAYER_P(l);
        const bool on = 16 * wv < Ly.out_dim;
        const bool need_abar = l > 0 || (!FIXED && net.enc == ENC_LINEAR);
        const bool kon = 16 * wv < Ly.in_dim;
        // zbar_l goes from where it was parked into this wave's columns of X.  The last layer's (the first here) was
        // parked in A2 and X's columns have been free since the output layer's barrier, so it moves BEFORE the barrier
        // below: with a single MFMA layer that barrier is all that keeps u16_encode (every column of A2, below) of a wave
        // that is ahead from overwriting the parked adjoint of a wave that is behind.  The other layers' X is read by
        // the GEMMs of layer l+1 up to the barrier, so theirs moves after it.
        auto unpark = [&]() {
#pragma unroll
          for (int j = 0; j < kUPackMax; ++j) {
            if (j < G && on) {
              f32x4 zb[K];
              u16_get<K>(park + eoff + 4 * j * kUP, zb);
              u16_put<K>(X + eoff + 4 * j * kUP, zb);
            }
          }
        };
        const bool top = l + 1 == nl;
        if (top) unpark();
        if (!top || nl == 1) U16_BARRIER(ST_BWD_EW);
        if (!top) unpark();
        float pw = 0.0f;
        u16_wave_sync();  // this wave's parked words are read before its replay below overwrites them (top layer: A2)
        if (l > 0) {
          const LayerDev P = U16_LAYER_P(l - 1);
          pw = P.act_param;
          if (kon) {  // replay a_{l-1} into this wave's columns of A2
#pragma unroll
            for (int j = 0; j < kUPackMax; ++j) {
              if (j < G) {
                f32x4 rec[K], y[K];
                u16_get<K>(REC + (l - 1) * img + eoff + 4 * j * kUP, rec);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  float z[K], yy[K];
#pragma unroll
                  for (int s = 0; s < K; ++s) z[s] = rec[s][r];
                  u16_act_replay<ACT, NT, NX, MRG>(pw, mcoef(), z, yy);
#pragma unroll
                  for (int s = 0; s < K; ++s) y[s][r] = yy[s];
                }
                u16_put<K>(A2 + eoff + 4 * j * kUP, y);
              }
            }
          }
        } else {
          u16_encode<ACT, NT, NX, MRG, FIXED>(net, ep, xin, A2, tp, mcoef());
        }
        const unsigned coff = u16_cols_off(kon ? 16 * wv : 0, Ly.ld, cp, gp);
        if (need_abar) {
          w0 = u16_wload<true>(Ly.W, Ly.ld, coff, 0);
          w1 = u16_wload<true>(Ly.W, Ly.ld, coff, 1);
        }
        U16_BARRIER(ST_BWD_PUT);
        if (U16_HAS_DB(l, Ly) && tp < Ly.out_dim) {
          float gsum = 0.0f;
          for (int n = 0; n < 4 * G; ++n) gsum += X[n * kUP + tp];
          pl[l * kUH + tp] += gsum;
        }
        PINN_STAMP(ST_BWD_DB);
        // abar_{l-1} = W^T zbar, then the activation adjoint of layer l-1.  The accumulators go through the wave's own
        // columns of the record image of layer l-1 (l = 0: of layer 0), which nothing reads any more: the replay above
        // was its last reader but for the adjoint below, which takes the record into registers first.
        if (need_abar) {
          f32x4 pa[kUPackMax];
#pragma unroll
          for (int j = 0; j < kUPackMax; ++j) pa[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
          if (kon) u16p_gemm<true>(pa, G, Ly.W, Ly.ld, coff, w0, w1, Ly.out_dim >> 4, X + boff);
          PINN_STAMP(ST_BWD_DX);
          float* const xch = REC + (l > 0 ? l - 1 : 0) * img;
#pragma unroll
          for (int j = 0; j < kUPackMax; ++j) {
            if (j < G) {
              // l = 0 (first Linear as the encoding): abar stays where the accumulators put it; the encoding backward
              // reads it there after a workgroup barrier
              f32x4 rec[K];
              if (l > 0) {
                if (kon) u16_get<K>(xch + eoff + 4 * j * kUP, rec);
                u16_wave_sync();
              }
              if (kon && wcol) *reinterpret_cast<f32x4*>(xch + woff + 4 * j * kUP) = pa[j];
              if (l > 0) {
                u16_wave_sync();
                if (kon) {
                  f32x4 ab[K];
                  u16_get<K>(xch + eoff + 4 * j * kUP, ab);
                  cadd(u16_ew_backward<ACT, NT, NX, MRG>(ab, pw, rec, mcoef()), sp == 0);
                  u16_put<K>(xch + eoff + 4 * j * kUP, ab);
                }
              }
            }
          }
          park = xch;
          PINN_STAMP(ST_BWD_EW);
        }
        if (on && U16_HAS_DW(l, Ly)) {
          const float* zl = X + gp * kUP + 16 * wv + cp;
          const float* al = A2 + gp * kUP + cp;
          const int na = Ly.in_dim >> 4;
          if (l == 0) u16p_outer<K, 0, NA0, NPT>(pt, G, na, zl, al);
          else if (l == 1) u16p_outer<K, NA0, NKT, NPT>(pt, G, na, zl, al);
          else u16p_outer<K, NA0 + NKT, NKT, NPT>(pt, G, na, zl, al);
        }
        PINN_STAMP(ST_BWD_STREAM);
        if constexpr (MRG && COEF) {  // the Fourier features' coefficient partial, as in a unit: the lanes of the w columns
          if (l == 0 && (FIXED || net.enc == ENC_FOURIER) && kon) {
            f32x4 pa[kUPackMax];
#pragma unroll
            for (int j = 0; j < kUPackMax; ++j) pa[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            u16p_gemm<true>(pa, G, Ly.W, Ly.ld, coff, u16_wload<true>(Ly.W, Ly.ld, coff, 0), u16_wload<true>(Ly.W, Ly.ld, coff, 1),
                            Ly.out_dim >> 4, X + boff);
            const int M = FIXED ? kUFixed.enc_out >> 1 : net.enc_out >> 1;
            float part = 0.0f;
#pragma unroll
            for (int j = 0; j < kUPackMax; ++j) {
              if (j < G) {
                const f32x4 val = *reinterpret_cast<const f32x4*>(A2 + eoff + 4 * j * kUP);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  const int jf = frowp + r;
                  part = fmaf(pa[j][r], fourier_coef_partial_merged(ep[jf < M ? jf : jf - M], val[r]), part);
                }
              }
            }
            cadd(part, sp == 1);
          }
        }
      }

      // ---- encoding backward (first Linear of feedforward / SIREN) ----
      if (!FIXED && net.enc == ENC_LINEAR && (net.d_encW || (MRG && COEF))) {
        const int H = net.enc_out;
        const bool enc_sums = !(MRG && COEF) || net.d_encW != nullptr;
        U16_BARRIER(ST_ENC_BWD);
        if (16 * wv < H) {
#pragma unroll
          for (int j = 0; j < kUPackMax; ++j) {
            if (j < G) {
              f32x4 ab[K];
              u16_get<K>(park + eoff + 4 * j * kUP, ab);  // abar of the encoding's outputs, left there by layer 0
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                float z[K], abv[K], zb[K];
                u16_enc_preact<NT, NX>(ep, din, xin, frowp + r, 4 * j + qp, z);
#pragma unroll
                for (int s = 0; s < K; ++s) abv[s] = ab[s][r];
                if constexpr (MRG) cadd(act_bwd_merged<ACT>(net.enc_param, mcoef(), z, abv, zb), sp == 0);
                else act_bwd<ACT, NT, NX>(net.enc_param, z, abv, zb);
#pragma unroll
                for (int s = 0; s < K; ++s) ab[s][r] = zb[s];
              }
              if (enc_sums) u16_put<K>(X + eoff + 4 * j * kUP, ab);
            }
          }
        }
        U16_BARRIER(ST_ENC_BWD);
        if (enc_sums && tp < H) {
          float gb = 0.0f, gt = 0.0f, gx = 0.0f;
          float gw[kMaxDin] = {0.0f, 0.0f, 0.0f, 0.0f};
          for (int n = 0; n < 4 * G; ++n) {
            const float vv = X[n * kUP + tp];
            gb += vv;
#pragma unroll
            for (int cc = 0; cc < kMaxDin; ++cc)
              if (cc < din) gw[cc] = fmaf(vv, xin[cc * kU + n], gw[cc]);
            if constexpr (NT >= 1) gt += X[1 * kUImgS + n * kUP + tp];
            if constexpr (NX >= 1) gx += X[(1 + NT) * kUImgS + n * kUP + tp];
          }
#pragma unroll
          for (int cc = 0; cc < kMaxDin; ++cc) pl[(kPersist + cc) * kUH + tp] += gw[cc] + (cc == din - 1 ? gt : 0.0f) + (cc == 0 ? gx : 0.0f);
          pl[(kPersist + kMaxDin) * kUH + tp] += gb;
        }
        PINN_STAMP(ST_ENC_BWD);
      }
    }
    __syncthreads();  // the round's writers of the running sums (psl, the COEF slots) are not the flush's readers
  }
#endif

  // ---- one flush per workgroup: reverse launches store into row blockIdx.x of the slab (a.flush_store: every address
  // written once); a forward-only launch adds its loss sum as the 32-point kernel does ----
  // The flush addresses are derived from an opaque copy of the thread index: computed from tid itself they are
  // hoisted above the unit loop, where the kernel has no VGPR to spare, and spilled.
  const int tf = u16_opaque(tid);
  const int cf = tf & 15, frowf = 16 * wv + 4 * ((tf & 63) >> 4);
  const long long doff = det_row_offset(a);
  if (a.mode == MODE_PDE && a.loss_sum && wv == 0) {
    float sacc = tf < kU ? psl[tf] : 0.0f;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) sacc += __shfl_xor(sacc, o);
    if (tf == 0) grad_put(a.loss_sum, sacc, doff, a.flush_store != 0);
  }
#ifdef PINN_STAMPS
  auto write_stamps = [&]() {  // [grid][8 waves][kNumStamps]
    if (a.stamps && (tf & 63) == 0) {
      st_acc[ST_TOTAL] = pinn_now() - st_begin;
      for (int i = 0; i < kNumStamps; ++i) a.stamps[((long long)blockIdx.x * kUWaves + wv) * kNumStamps + i] = st_acc[i];
    }
  };
  if constexpr (!BWD) write_stamps();
#endif
  if constexpr (!BWD) return;
  if constexpr (COEF && MRG) {  // dL/dc_0 = -dL/dc: lanes -> waves -> the slab row's slot; c_1 has no cotangent
    float sc = pcl[tf];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sc += __shfl_xor(sc, o);
    if ((tf & 63) == 0) UP[wv] = sc;
    __syncthreads();
    if (a.mode == MODE_PDE && a.pde.dcoef && tf == 0) {
      float st = 0.0f;
#pragma unroll
      for (int w = 0; w < kUWaves; ++w) st += UP[w];
      a.pde.dcoef[doff] = -st;
      a.pde.dcoef[doff + 1] = 0.0f;
    }
  } else if constexpr (COEF) {
    if (a.mode == MODE_PDE && a.pde.dcoef && wv == 0) {
      float s0 = tf < kU ? X[tf * kUP + kUH] : 0.0f, s1 = tf < kU ? X[tf * kUP + kUH + 1] : 0.0f;
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {
        s0 += __shfl_xor(s0, o);
        s1 += __shfl_xor(s1, o);
      }
      if (tf == 0) {
        a.pde.dcoef[doff] = s0;
        a.pde.dcoef[doff + 1] = s1;
      }
    }
  }
  if (net.db_out && wv == 0) {
    float gsum = tf < kU ? psl[kU + tf] : 0.0f;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) gsum += __shfl_xor(gsum, o);
    if (tf == 0) net.db_out[doff] = gsum;
  }
  if (!FIXED && net.enc == ENC_LINEAR && net.d_encW && tf < net.enc_out) {
#pragma unroll
    for (int cc = 0; cc < kMaxDin; ++cc)
      if (cc < din) net.d_encW[doff + tf * din + cc] = pl[(kPersist + cc) * kUH + tf];
    if (net.d_encb) net.d_encb[doff + tf] = pl[(kPersist + kMaxDin) * kUH + tf];
  }
  const f32x4 pdw = row16_sum4(*reinterpret_cast<const f32x4*>(pdwl + 4 * tf));
  if (net.dw_out && cf == 0 && frowf < net.h_last) *reinterpret_cast<f32x4*>(net.dw_out + doff + frowf) = pdw;
#pragma unroll
  for (int p = 0; p < kPersist; ++p) {
    if (p < nl) {
      LayerDev Lp = U16_LAYER(p);
      if constexpr (FIXED) {  // the gradient pointers are read here, where they are used
        Lp.dW = uniform_ptr(net.layer[p].dW);
        Lp.db = uniform_ptr(net.layer[p].db);
      }
      if (Lp.db && tf < Lp.out_dim) Lp.db[doff + tf] = pl[p * kUH + tf];
      if (16 * wv >= Lp.out_dim) continue;
      if (Lp.dW) {
        const int na = Lp.in_dim >> 4;
        const int off = p == 0 ? 0 : p == 1 ? NA0 : NA0 + NKT;
        float* base = Lp.dW + doff + (long long)frowf * Lp.ld + cf;
#pragma unroll
        for (int t = 0; t < NPT; ++t) {
          if (t >= off && t - off < na && (p != 0 || t < NA0) && (p != 1 || t < NA0 + NKT)) {
#pragma unroll
            for (int r = 0; r < 4; ++r) base[(long long)r * Lp.ld + 16 * (t - off)] = pt[t][r];
          }
        }
      }
    }
  }
#ifdef PINN_STAMPS
  PINN_STAMP(ST_BWD_FLUSH);
  write_stamps();
#endif
}

#undef U16_LAYER
#undef U16_LAYER_P
#undef U16_HAS_DW
#undef U16_HAS_DB
#undef U16_LAYER_UNROLL

// The launch plan (host).  With grid workgroups, R = N / (16 grid) full rounds of 16-point units and M = N - 16 grid R
// points left, G = ceil(M / (4 grid)) <= 4 four-point groups per workgroup hold them.  G = 1..3 (and a unit compiled with
// the packed round): every workgroup runs its R units and then one packed round of G groups, workgroup b on the (at most
// 4 G) points from first_tail + 4 G b on.  G = 0: nothing is left.  G = 4: the last round is ordinary units.
struct U16Plan {
  long long rounds;      // R
  long long first_tail;  // 16 grid R
  int groups;            // G
};
inline U16Plan jet_u16_tail_plan(long long N, int grid, bool packed) {
  U16Plan p;
  const long long per_round = (long long)kU * grid;
  p.rounds = N / per_round;
  p.first_tail = p.rounds * per_round;
  const long long M = N - p.first_tail;
  p.groups = (int)((M + 4LL * grid - 1) / (4LL * grid));
  if (!packed && p.groups > 0) p.groups = 4;
  return p;
}
// the plan as the kernel reads it
inline void jet_u16_set_plan(KernelArgs& a, int grid, bool packed) {
  const U16Plan p = jet_u16_tail_plan(a.N, grid, packed);
  const bool pack = p.groups >= 1 && p.groups <= kUPackMax;
  a.u16_loop_points = pack ? p.first_tail : a.N;
  a.u16_tail_groups = pack ? p.groups : 0;
}

inline size_t jet_u16_lds_bytes(int K) {
  return sizeof(float) * ((size_t)4 * K * kUImgS + kUWaves * K * kU + 2 * kMaxDin * kU + (1 + kPersist) * kUH +
                          (kMaxDin + 1) * kUH + (kPersist + kMaxDin + 1) * kUH + 4 * kUThreads + 2 * kU + kMaxDin * kU);
}
// the merged units: K = 3; reverse launches have the fifth image S behind the record images; the COEF form has its
// per-lane dL/dc sums (pcl) behind everything else
constexpr size_t jet_u16m_lds_bytes(bool coef, bool bwd) {
  return sizeof(float) * ((size_t)(bwd ? 5 : 4) * 3 * kUImgS + kUWaves * 3 * kU + 2 * kMaxDin * kU + (1 + kPersist) * kUH +
                          (kMaxDin + 1) * kUH + (kPersist + kMaxDin + 1) * kUH + 4 * kUThreads + 2 * kU + kMaxDin * kU +
                          (coef ? kUThreads : 0));
}
static_assert(jet_u16m_lds_bytes(true, true) <= 160 * 1024 && jet_u16m_lds_bytes(false, true) == 146048 &&
                  jet_u16m_lds_bytes(false, false) == 120704,
              "the merged units' five images and running sums fit the CU's LDS");


// The 16-point kernel can run the reverse launch of this network, and then runs its forward-only launches too (the
// stream set / unit / flush checks are the caller's).  Only the variant
// with four first-layer dW tiles (first MFMA layer reads at most 64 features, e.g. 64 Fourier features) is compiled:
// with eight, the persistent tiles take 96 VGPRs and the kernel spills.
inline bool jet_u16_fits(const NetDev& n, int K) {
  if (K > 4 || n.n_layers < 1 || n.n_layers > kPersist || jet_wide_hmax(n.hmax) != 128) return false;
  if (n.layer[0].in_dim > 64) return false;
  for (int l = 0; l < n.n_layers; ++l)
    if (n.layer[l].in_dim % 16 || n.layer[l].out_dim % 16 || n.layer[l].in_dim > kUH || n.layer[l].out_dim > kUH) return false;
  return jet_u16_lds_bytes(K) <= 160 * 1024;
}

template <int ACT, int NT, int NX>
hipError_t launch_jet_u16_act(const KernelArgs& a, bool bwd, int grid, hipStream_t stream) {
  constexpr int K = 1 + NT + NX;
  auto kern = bwd ? jet_kernel_u16<ACT, NT, NX, true, 4> : jet_kernel_u16<ACT, NT, NX, false, 4>;
  hipError_t e = allow_full_lds(reinterpret_cast<const void*>(kern));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kUThreads), jet_u16_lds_bytes(K), stream, a);
  return hipGetLastError();
}

// the COEF variant (reverse launch only): jet_u16c_* units
template <int ACT, int NT, int NX>
hipError_t launch_jet_u16_coef(const KernelArgs& a, int grid, hipStream_t stream) {
  constexpr int K = 1 + NT + NX;
  auto kern = jet_kernel_u16<ACT, NT, NX, true, 4, true>;
  hipError_t e = allow_full_lds(reinterpret_cast<const void*>(kern));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kUThreads), jet_u16_lds_bytes(K), stream, a);
  return hipGetLastError();
}

// The network has the shape the fixed-shape units are compiled for (kUFixed); every other network that fits the 16-point
// kernel keeps the generic units: other widths, two or one MFMA layers, another feature count, a first-Linear encoding,
// a layer that is a column-chunk view (ld != in_dim).
inline bool jet_u16_fixed_shape(const NetDev& n) {
  if (n.enc != ENC_FOURIER || n.din != kUFixed.din || n.enc_out != kUFixed.enc_out || n.n_layers != kUFixed.layers) return false;
  if (n.h_last != kUFixed.width) return false;
  for (int l = 0; l < kUFixed.layers; ++l) {
    const int in = l == 0 ? kUFixed.in0 : kUFixed.width;
    if (n.layer[l].in_dim != in || n.layer[l].out_dim != kUFixed.width || n.layer[l].ld != in) return false;
  }
  return true;
}

// the merged units (MRG = true): forward-only / reverse, and the COEF reverse launch; FIXED: the fixed-shape units
template <int ACT, bool FIXED = false>
hipError_t launch_jet_u16m_act(const KernelArgs& a, bool bwd, int grid, hipStream_t stream) {
  auto kern = bwd ? jet_kernel_u16<ACT, 1, 1, true, 4, false, true, FIXED> : jet_kernel_u16<ACT, 1, 1, false, 4, false, true, FIXED>;
  hipError_t e = allow_full_lds(reinterpret_cast<const void*>(kern));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kUThreads), jet_u16m_lds_bytes(false, bwd), stream, a);
  return hipGetLastError();
}
template <int ACT, bool FIXED = false>
hipError_t launch_jet_u16m_coef(const KernelArgs& a, int grid, hipStream_t stream) {
  auto kern = jet_kernel_u16<ACT, 1, 1, true, 4, true, true, FIXED>;
  hipError_t e = allow_full_lds(reinterpret_cast<const void*>(kern));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kUThreads), jet_u16m_lds_bytes(true, true), stream, a);
  return hipGetLastError();
}

}  // namespace pinn
