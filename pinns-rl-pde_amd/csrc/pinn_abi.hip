// C ABI of the jet engine (include/pinn_jet.h): descriptor validation, engine choice, pointer plumbing.
// No device memory is allocated or retained here; every launch goes to the caller's stream.
//
// Two engines sit behind the same entry points:
//   * the fused tile-major "wide" kernel (jet_kernel_wide.h): plain MLP family (feedforward without LayerNorm,
//     fourier, siren), hidden widths multiples of 32 up to 128, all K streams of a tile resident in LDS — the
//     headline Burgers / fourier 4x128 configuration;
//   * the layer-major engine (lm_*.h): everything else — LayerNorm architectures (ResNet, attention, feedforward with
//     layer_norm), the autoencoder (always: use_wide admits the plain MLP family only), widths up to 1024 that need not
//     be multiples of 32, any derivative order the ABI admits.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "jet_kernel_u16.h"
#include "lm_engine.h"

namespace pinn {
#define PINN_DECL(nt, nx) hipError_t launch_jetw_##nt##_##nx(const KernelArgs&, bool, int, hipStream_t);
PINN_DECL(0, 0)
PINN_DECL(1, 0)
PINN_DECL(1, 1)
PINN_DECL(1, 2)
PINN_DECL(1, 3)
PINN_DECL(1, 4)
PINN_DECL(2, 0)
PINN_DECL(2, 2)
#undef PINN_DECL
#define PINN_DECLU1(nt, nx, a) hipError_t launch_jetu_##nt##_##nx##_a##a(const KernelArgs&, bool, int, hipStream_t);
#ifdef PINN_DEV /* make dev: one stream set, tanh */
#define PINN_DECLU(nt, nx) PINN_DECLU1(nt, nx, 0)
#else
#define PINN_DECLU(nt, nx) PINN_DECLU1(nt, nx, 0) PINN_DECLU1(nt, nx, 1) PINN_DECLU1(nt, nx, 2) PINN_DECLU1(nt, nx, 3) PINN_DECLU1(nt, nx, 4)
#endif
PINN_DECLU(0, 0)
PINN_DECLU(1, 0)
PINN_DECLU(1, 1)
PINN_DECLU(1, 2)
PINN_DECLU(2, 0)
#undef PINN_DECLU
#undef PINN_DECLU1
#ifndef PINN_DEV /* inverse problems: COEF units (jet_widec_*, jet_u16c_*), reverse launches only */
#define PINN_DECLC1(p, nt, nx, a) hipError_t launch_jet##p##_##nt##_##nx##_a##a(const KernelArgs&, int, hipStream_t);
#define PINN_DECLC(p, nt, nx) PINN_DECLC1(p, nt, nx, 0) PINN_DECLC1(p, nt, nx, 1) PINN_DECLC1(p, nt, nx, 2) PINN_DECLC1(p, nt, nx, 3) PINN_DECLC1(p, nt, nx, 4)
PINN_DECLC(wc, 1, 1)
PINN_DECLC(wc, 1, 2)
PINN_DECLC(wc, 1, 4)
PINN_DECLC(wc, 2, 0)
PINN_DECLC(wc, 2, 2)
PINN_DECLC(uc, 1, 1)
PINN_DECLC(uc, 1, 2)
PINN_DECLC(uc, 2, 0)
#undef PINN_DECLC
#undef PINN_DECLC1
#endif

/* merged stream set (Burgers on three streams): jet_u16m_<family>, jet_u16mc_<family>; with the network's shape compiled
   in: jet_u16mf_<family>, jet_u16mfc_<family> */
#if !defined(PINN_DEV)
#define PINN_DECLM(a) hipError_t launch_jetum_a##a(const KernelArgs&, bool, int, hipStream_t); hipError_t launch_jetumc_a##a(const KernelArgs&, int, hipStream_t);
#define PINN_DECLF(a) hipError_t launch_jetumf_a##a(const KernelArgs&, bool, int, hipStream_t); hipError_t launch_jetumfc_a##a(const KernelArgs&, int, hipStream_t);
PINN_DECLM(0) PINN_DECLM(1) PINN_DECLM(2) PINN_DECLM(3) PINN_DECLM(4)
PINN_DECLF(0) PINN_DECLF(2) PINN_DECLF(4) /* csrc/Makefile: FACTS */
#undef PINN_DECLM
#undef PINN_DECLF
#elif defined(PINN_DEV_MERGED)
hipError_t launch_jetum_a0(const KernelArgs&, bool, int, hipStream_t);
hipError_t launch_jetumf_a0(const KernelArgs&, bool, int, hipStream_t);
#endif

#ifdef PINN_STAMPS
static unsigned long long* g_stamps = nullptr;  // diagnostic builds only: device buffer for in-kernel phase timing
#endif

static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
}  // namespace pinn

// the training-step entry points (train_kernels.hip) leave their messages in the same thread-local string
extern "C" int pinn_internal_fail(int code, const char* msg) { return pinn::fail(code, "%s", msg); }

namespace pinn {

static int num_cus() {
  static int cached = 0;
  if (cached) return cached;
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) == hipSuccess &&
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) {
    cached = cus;
    return cus;
  }
  (void)hipGetLastError();
  return 256;  // MI355X; used only for sizing when no device is visible (CPU-side workspace queries)
}


// PINN_KERNEL=lm routes every architecture through the layer-major engine (tests run both engines on the MLP
// family).  Read once per process: the ABI itself carries no mutable state.
static bool force_lm() {
  static const bool v = [] {
    const char* e = getenv("PINN_KERNEL");
    return e && !strcmp(e, "lm");
  }();
  return v;
}

static float act_param_of(int act, float user) {
  switch (act) {
    case PINN_ACT_SIN: return user;
    case PINN_ACT_RELU: return 0.0f;
    case PINN_ACT_LEAKY_RELU: return 0.01f;  // nn.LeakyReLU() default slope
    case PINN_ACT_IDENTITY: return 1.0f;
    default: return 0.0f;
  }
}

// Wide-kernel layer program of the plain-MLP family, or false when the descriptor is outside what that kernel runs
// (the caller then takes the layer-major engine).  `w` / `g` may be null (sizing queries); when given they hold
// `num_tensors` entries, already validated against the descriptor.
static bool build_wide(const PinnNetDesc* d, const float* const* w, float* const* g, NetDev* out, int* misaligned = nullptr) {
  if (d->arch != PINN_ARCH_FOURIER && d->arch != PINN_ARCH_FEEDFORWARD && d->arch != PINN_ARCH_SIREN) return false;
  if (d->flags & (PINN_FLAG_LAYER_NORM | PINN_FLAG_LAYER_MAJOR)) return false;
  NetDev n;
  memset(&n, 0, sizeof(n));
  n.din = d->input_dim;
  const int act = d->arch == PINN_ARCH_SIREN ? PINN_ACT_SIN : d->activation;
  const float par = act_param_of(act, d->act_param);
  static float sixteen_aligned[4] __attribute__((aligned(16)));
  auto W = [&](int i) -> const float* { return w ? w[i] : sixteen_aligned; };
  auto G = [&](int i) -> float* { return g ? g[i] : nullptr; };
  int first_mfma, wbase;
  if (d->arch == PINN_ARCH_FOURIER) {
    if (d->mapping_size <= 0 || (2 * d->mapping_size) % 8) return false;
    n.enc = ENC_FOURIER;
    n.enc_out = 2 * d->mapping_size;
    n.encW = W(0);
    first_mfma = 0;
    wbase = 1;
  } else {
    n.enc = ENC_LINEAR;
    n.enc_out = d->widths[0];
    n.encW = W(0);
    n.encb = W(1);
    n.d_encW = G(0);
    n.d_encb = G(1);
    n.enc_act = act;
    n.enc_param = par;
    first_mfma = 1;
    wbase = 0;
    if (n.enc_out % 32) return false;
  }
  int prev = n.enc_out, hmax = (n.enc_out + 31) / 32 * 32;
  n.n_layers = 0;
  for (int i = first_mfma; i < d->num_linear - 1; ++i) {
    const int wd = d->widths[i];
    if (wd % 32 || wd <= 0 || wd > 128 || prev % 8) return false;
    LayerDev& L = n.layer[n.n_layers++];
    L.W = W(wbase + 2 * i);
    L.b = W(wbase + 2 * i + 1);
    L.dW = G(wbase + 2 * i);
    L.db = G(wbase + 2 * i + 1);
    L.in_dim = prev;
    L.ld = prev;
    L.out_dim = wd;
    L.act = act;
    L.act_param = par;
    if (reinterpret_cast<uintptr_t>(L.W) & 15) {  // 16-byte weight loads
      if (misaligned) *misaligned = wbase + 2 * i;
      return false;
    }
    prev = wd;
    if (wd > hmax) hmax = wd;
  }
  const int io = d->num_linear - 1;
  n.w_out = W(wbase + 2 * io);
  n.b_out = W(wbase + 2 * io + 1);
  n.dw_out = G(wbase + 2 * io);
  n.db_out = G(wbase + 2 * io + 1);
  n.h_last = prev;
  if (prev % 32 || hmax > 128) return false;
  n.hmax = hmax;
  *out = n;
  return true;
}

static bool wide_store_flush_on() {  // PINN_WIDE_STORE_FLUSH=0: the two-level atomic flush everywhere (experiments), read once
  static const bool v = [] {
    const char* e = getenv("PINN_WIDE_STORE_FLUSH");
    return !(e && atoi(e) == 0);
  }();
  return v;
}

// ---- deterministic mode of the fused kernel -------------------------------------------------------------------------
// Every gradient / loss pointer of the NetDev is redirected into row 0 of a [grid][stride] slab in the workspace;
// workgroup b adds into row b with plain (non-atomic) adds, and this kernel then sums the rows of every element in
// workgroup order and adds the total to the caller's tensor: two launches on the same inputs give identical bits.
constexpr int kFlushRows = 8;  // shared slab rows of the default (non-deterministic) two-level flush

struct DetTable {
  int n;
  float* user[2 * PINN_MAX_LINEAR + 8];
  unsigned off[2 * PINN_MAX_LINEAR + 8], cnt[2 * PINN_MAX_LINEAR + 8];
  unsigned lead[2 * PINN_MAX_LINEAR + 8];  // floats at the start of the slot that belong to another target (the coefficient
                                           // sums sit in the padding of the loss-sum slot); off stays 16-byte aligned
  unsigned stride;
};

__global__ void wide_det_reduce(const DetTable tab, const float* slab, int rows) {
  const unsigned it = blockIdx.y;
  for (unsigned e = blockIdx.x * blockDim.x + threadIdx.x; e < tab.cnt[it]; e += gridDim.x * blockDim.x) {
    float s = 0.0f;
    for (int b = 0; b < rows; ++b) s += slab[(size_t)b * tab.stride + tab.off[it] + tab.lead[it] + e];
    tab.user[it][e] += s;
  }
}

// Store flush (KernelArgs::flush_store): every workgroup has WRITTEN its row; user[e] += sum over rows in row order.
// A block sums 128 consecutive elements (32 threads x 16 bytes) over 8 interleaved row groups and combines them through
// LDS in a fixed order: 42 MB of rows at ~4 TB/s instead of 256 dependent loads per thread.
__global__ __launch_bounds__(256) void wide_rows_reduce(const DetTable tab, const float* slab, int rows) {
  __shared__ float part[8][128];
  const unsigned it = blockIdx.y;
  const unsigned lead = tab.lead[it], end = lead + tab.cnt[it];
  const unsigned cnt4 = (end + 3u) & ~3u;  // rows are padded to 4 floats per target (det_slot)
  const int el = threadIdx.x & 31, rg = threadIdx.x >> 5;
  for (unsigned e0 = blockIdx.x * 128u; e0 < cnt4; e0 += gridDim.x * 128u) {
    const unsigned e = e0 + 4u * el;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    if (e < cnt4) {
      const float* src = slab + tab.off[it] + e;
#pragma unroll 8
      for (int b = rg; b < rows; b += 8) {
        const float4 v = *reinterpret_cast<const float4*>(src + (size_t)b * tab.stride);
        s0 += v.x; s1 += v.y; s2 += v.z; s3 += v.w;
      }
    }
    part[rg][4 * el + 0] = s0;
    part[rg][4 * el + 1] = s1;
    part[rg][4 * el + 2] = s2;
    part[rg][4 * el + 3] = s3;
    __syncthreads();
    if (threadIdx.x < 128 && e0 + threadIdx.x >= lead && e0 + threadIdx.x < end) {
      float t = 0.0f;
#pragma unroll
      for (int g = 0; g < 8; ++g) t += part[g][threadIdx.x];
      tab.user[it][e0 + threadIdx.x - lead] += t;
    }
    __syncthreads();
  }
}

// How a launch of the fused kernel reduces its weight gradients (and loss sum).  Reverse launches of networks whose MFMA
// layers all keep their weight-gradient tiles in registers (n_layers <= kPersist: nothing is flushed inside the tile
// loop) take the STORE flush, in both modes; otherwise PINN_FLAG_DETERMINISTIC takes one slab row per workgroup, and
// a reverse launch of more than kFlushRows workgroups the TWO-LEVEL flush; everything else adds with direct atomics.
enum WideFlush { FLUSH_DIRECT = 0, FLUSH_STORE = 1, FLUSH_TWO_LEVEL = 2, FLUSH_DET_SLAB = 3 };

static WideFlush wide_flush(const PinnNetDesc* d, const NetDev& n, int grid, bool bwd) {
  if (bwd && n.n_layers <= kPersist && wide_store_flush_on()) return FLUSH_STORE;
  if (d->flags & PINN_FLAG_DETERMINISTIC) return FLUSH_DET_SLAB;
  if (bwd && grid > kFlushRows) return FLUSH_TWO_LEVEL;
  return FLUSH_DIRECT;
}

// slab rows a flush needs in the workspace (0: none)
static int wide_slab_rows(WideFlush f, int grid) {
  return f == FLUSH_DIRECT ? 0 : f == FLUSH_TWO_LEVEL ? kFlushRows : grid;
}

// redirect one accumulation target into the slab; returns the slab pointer (row 0)
static float* det_slot(DetTable& t, float* slab, float* user, unsigned count) {
  if (!user) return nullptr;
  const int i = t.n++;
  t.user[i] = user;
  t.off[i] = t.stride;
  t.cnt[i] = count;
  t.stride += (count + 3u) & ~3u;
  return slab + t.off[i];
}

// all targets of a NetDev (and the loss sum) -> slab; `slab` may be null for sizing (only t.stride is then meaningful)
static void det_redirect(NetDev& n, float*& loss_sum, float*& dcoef, float* slab, DetTable& t) {
  memset(&t, 0, sizeof(t));
  static float dummy;
  float* base = slab ? slab : &dummy;
  auto slot = [&](float*& p, unsigned count, bool sizing_always) {
    if (slab) p = det_slot(t, base, p, count);
    else if (p || sizing_always) t.stride += (count + 3u) & ~3u;
  };
  // sizing queries have no pointers: count every target the descriptor can have
  const bool sizing = slab == nullptr;
  if (n.enc == ENC_LINEAR) {
    slot(n.d_encW, (unsigned)(n.enc_out * n.din), sizing);
    slot(n.d_encb, (unsigned)n.enc_out, sizing);
  }
  for (int l = 0; l < n.n_layers; ++l) {
    slot(n.layer[l].dW, (unsigned)(n.layer[l].out_dim * n.layer[l].ld), sizing);
    slot(n.layer[l].db, (unsigned)n.layer[l].out_dim, sizing);
  }
  slot(n.dw_out, (unsigned)n.h_last, sizing);
  slot(n.db_out, 1u, sizing);
  const unsigned loss_off = t.stride;  // the loss-sum slot is 1 float padded to 4: floats 1, 2 hold the coefficient sums
  slot(loss_sum, 1u, sizing);
  if (slab && dcoef) {
    const int i = t.n++;
    t.user[i] = dcoef;
    t.off[i] = loss_off;
    t.lead[i] = 1;
    t.cnt[i] = 2;
    dcoef = slab + loss_off + 1;
  }
  if (t.stride == 0) t.stride = 4;
}

static int check_orders(int nt, int nx) {
  if (nt < 0 || nt > 2) return fail(PINN_ERR_BAD_ORDER, "Temporal derivative order %d is not supported. Maximum order is 2.", nt);
  if (nx < 0 || nx > 4) return fail(PINN_ERR_BAD_ORDER, "Spatial derivative order %d is not supported. Maximum order is 4.", nx);
  return PINN_OK;
}

static bool stream_set_compiled(int nt, int nx) {
  static const int sets[][2] = {{0, 0}, {1, 0}, {1, 1}, {1, 2}, {1, 3}, {1, 4}, {2, 0}, {2, 2}};
  for (auto& s : sets)
    if (s[0] == nt && s[1] == nx) return true;
  return false;
}

// PINN_FLAG_SPACE_AXIS of a descriptor: the column of x its space streams differentiate along (0: the first, as ever)
static int space_axis_of(const PinnNetDesc* d) { return (d->flags & PINN_FLAG_SPACE_AXIS_MASK) >> 8; }

// PINN_FLAG_SPACE_DIRECTION bits of a descriptor (0: no direction; lm_engine.hip::build_program validates them)
static int space_dir_bits(const PinnNetDesc* d) { return d->flags & PINN_FLAG_SPACE_DIRECTION_MASK; }

// A non-zero axis runs the layer-major engine, which also has units for the space-only sets (0, 1) .. (0, 4): the launches
// of a further space axis (csrc/Makefile: ASETS).  With axis 0 they stay refused like any other uncompiled set.  A
// direction launch runs there too and admits those four sets alone.
static bool stream_set_admitted(const PinnNetDesc* d, int nt, int nx) {
  const bool space_only = nt == 0 && nx >= 1 && nx <= 4;
  if (space_dir_bits(d) != 0) {  // a descriptor the engine refuses (an invalid direction): lm_check reports that, not the set
    char lerr[8];
    return lm::lm_check(d, lerr, sizeof(lerr)) != PINN_OK || space_only;
  }
  if (stream_set_compiled(nt, nx)) return true;
  return space_axis_of(d) != 0 && space_only;
}

// the compiled PDE kinds keep the reference's >= 2-D behaviour (every spatial derivative zero): no axis for them
static int refuse_axis(const PinnNetDesc* d, const char* entry) {
  if (d && space_axis_of(d) != 0)
    return fail(PINN_ERR_UNSUPPORTED, "%s: PINN_FLAG_SPACE_AXIS(%d) is set, and the compiled PDE kinds differentiate along the first "
                "space axis only (derivatives along further axes: pinn_jet_forward + pinn_term_residual_axes)", entry, space_axis_of(d));
  if (d && space_dir_bits(d) != 0)
    return fail(PINN_ERR_UNSUPPORTED, "%s: PINN_FLAG_SPACE_DIRECTION is set, and the compiled PDE kinds differentiate along the first "
                "space axis only (mixed derivatives: pinn_jet_forward + pinn_term_residual_mixed)", entry);
  return PINN_OK;
}

static hipError_t dispatch_wide(int nt, int nx, const KernelArgs& a, bool bwd, int grid, hipStream_t st) {
#define PINN_CASE2(NT_, NX_) \
  if (nt == NT_ && nx == NX_) return launch_jetw_##NT_##_##NX_(a, bwd, grid, st);
#define PINN_CASE(NT_, NX_) PINN_CASE2(NT_, NX_)
#ifdef PINN_DEV /* make dev: one stream set */
  PINN_CASE(PINN_DEV_NT, PINN_DEV_NX)
#else
  PINN_CASE(0, 0) PINN_CASE(1, 0) PINN_CASE(1, 1) PINN_CASE(1, 2) PINN_CASE(1, 3) PINN_CASE(1, 4) PINN_CASE(2, 0) PINN_CASE(2, 2)
#endif
#undef PINN_CASE
#undef PINN_CASE2
  return hipErrorInvalidValue;
}

// the wide kernel runs this problem: program built, all K streams fit the LDS, engine not overridden
static bool use_wide(const PinnNetDesc* d, const float* const* w, float* const* g, int K, bool bwd, NetDev* n, int* misaligned = nullptr) {
  if (force_lm()) return false;
  if (space_axis_of(d) != 0 || space_dir_bits(d) != 0) return false;  // the tile-major kernels seed their space streams from column 0 only
  if (!build_wide(d, w, g, n, misaligned)) return false;
  return jet_wide_fits(K, n->hmax, bwd, n->n_layers);
}

// The 16-point kernel (jet_kernel_u16.h) runs the reverse launches of the store-flush class at image height 128, K <= 4,
// of a stream set whose unit of this activation family was built without scratch, PINN_FLAG_WIDE_TILE32 not set.  The
// forward-only launches of such a descriptor take it too: per-point results then do not depend on whether the call
// has a reverse sweep (bit for bit).
static bool u16_set_compiled(int nt, int nx) {
#ifdef PINN_DEV
  return nt == PINN_DEV_NT && nx == PINN_DEV_NX;
#else
  static const int sets[][2] = {{0, 0}, {1, 0}, {1, 1}, {1, 2}, {2, 0}};
  for (auto& s : sets)
    if (s[0] == nt && s[1] == nx) return true;
  return false;
#endif
}

// stream sets of the COEF units (inverse problems): the PDEs that have a coefficient
static bool widec_set_compiled(int nt, int nx) {
#ifdef PINN_DEV
  return false;
#else
  static const int sets[][2] = {{1, 1}, {1, 2}, {1, 4}, {2, 0}, {2, 2}};
  for (auto& s : sets)
    if (s[0] == nt && s[1] == nx) return true;
  return false;
#endif
}
static bool u16c_set_compiled(int nt, int nx) {
#ifdef PINN_DEV
  return false;
#else
  return (nt == 1 && (nx == 1 || nx == 2)) || (nt == 2 && nx == 0);
#endif
}

// coef: the jet_u16c_* unit of a pinn_residual_loss_grad_inverse call instead of the jet_u16_* one
static bool use_u16(const PinnNetDesc* d, const NetDev& n, int nt, int nx, bool bwd, bool coef = false) {
  (void)bwd;
  if ((d->flags & PINN_FLAG_WIDE_TILE32) || !(coef ? u16c_set_compiled(nt, nx) : u16_set_compiled(nt, nx))) return false;
  if (wide_flush(d, n, 0, true) != FLUSH_STORE || !jet_u16_fits(n, 1 + nt + nx)) return false;
  const int fam = jet_wide_act_family(n);
#ifdef PINN_DEV
  if (fam != PINN_ACT_TANH) return false;
#endif
  char unit[64];  // pinn_build_info() lists the u16 units that need scratch or the default MFMA form: not routed
  snprintf(unit, sizeof(unit), coef ? "jet_u16c_%d_%d_%d:" : "jet_u16_%d_%d_%d:", nt, nx, fam);
  return strstr(pinn_build_info(), unit) == nullptr;
}

// The unit of this launch carries the packed round (jet_kernel_u16.h).  A unit that would need scratch with it is built
// without (csrc/Makefile) and listed in pinn_build_info() as "nopack jet_u16..."; its last round stays ordinary units.
static bool u16_unit_packed(const NetDev& n, int nt, int nx, bool coef) {
  char unit[64];
  snprintf(unit, sizeof(unit), coef ? "nopack jet_u16c_%d_%d_%d " : "nopack jet_u16_%d_%d_%d ", nt, nx, jet_wide_act_family(n));
  return strstr(pinn_build_info(), unit) == nullptr;
}

// The merged units (jet_kernel_u16.h, MRG) run the residual-mode calls of 1-D Burgers on the stream set (1,2) with three
// streams instead of four.  The answer is a function of the descriptor, the PDE and the build alone, the same for
// forward-only, fused, res_bar and inverse calls, so their per-point residuals stay bit-identical: both four-stream u16
// units (plain and COEF) must take the descriptor, and both merged units of the family must be routable (the dev build
// has no COEF units at all and asks for the one it has).  PINN_FLAG_PLAIN_STREAMS keeps the four-stream units.
static bool use_merged(const PinnNetDesc* d, const NetDev& n, const PinnPdeDesc* pde, int nt, int nx, int mode) {
  if (mode != MODE_PDE || !pde || pde->kind != PINN_PDE_BURGERS || pde->dimension != 1 || nt != 1 || nx != 2) return false;
  if (d->flags & PINN_FLAG_PLAIN_STREAMS) return false;
  const int fam = jet_wide_act_family(n);
#if defined(PINN_DEV) && !defined(PINN_DEV_MERGED)
  return false;
#elif defined(PINN_DEV)
  return fam == PINN_ACT_TANH && use_u16(d, n, nt, nx, true, false);
#else
  if (!use_u16(d, n, nt, nx, true, false) || !use_u16(d, n, nt, nx, true, true)) return false;
  char unit[64];
  snprintf(unit, sizeof(unit), "jet_u16m_%d:", fam);
  if (strstr(pinn_build_info(), unit)) return false;
  snprintf(unit, sizeof(unit), "jet_u16mc_%d:", fam);
  return strstr(pinn_build_info(), unit) == nullptr;
#endif
}

static bool u16m_unit_packed(const NetDev& n, bool coef) {
  char unit[64];
  snprintf(unit, sizeof(unit), coef ? "nopack jet_u16mc_%d " : "nopack jet_u16m_%d ", jet_wide_act_family(n));
  return strstr(pinn_build_info(), unit) == nullptr;
}

// The fixed-shape merged units (jet_kernel_u16.h, FIXED) take a descriptor that takes the merged units and has the shape
// they are compiled for (jet_u16_fixed_shape).  They give the generic merged units' bits, and like use_merged the answer is
// the same for forward-only, fused, res_bar and inverse calls: both fixed units of the family must be routable, and each
// must carry the packed round exactly if its generic sibling does (the round sums in another order than ordinary units).
// PINN_FLAG_GENERIC_UNITS keeps the generic merged units.  `merged` is use_merged's answer for the same call.
static bool use_fixed_shape(const PinnNetDesc* d, const NetDev& n, bool merged) {
  if (!merged || (d->flags & PINN_FLAG_GENERIC_UNITS) || !jet_u16_fixed_shape(n)) return false;
  const int fam = jet_wide_act_family(n);
  if (fam == PINN_ACT_SIN || fam == PINN_ACT_SIGMOID) return false;  // no fixed units are built for these (csrc/Makefile: FACTS)
  const char* info = pinn_build_info();
  char unit[64];
#if defined(PINN_DEV)
  const int forms = 1;  // the dev build has no COEF units
#else
  const int forms = 2;
#endif
  for (int coef = 0; coef < forms; ++coef) {
    snprintf(unit, sizeof(unit), coef ? "jet_u16mfc_%d:" : "jet_u16mf_%d:", fam);
    if (strstr(info, unit)) return false;
    snprintf(unit, sizeof(unit), coef ? "nopack jet_u16mfc_%d " : "nopack jet_u16mf_%d ", fam);
    if ((strstr(info, unit) == nullptr) != u16m_unit_packed(n, coef != 0)) return false;
  }
  return true;
}

static hipError_t dispatch_u16m(bool coef, bool fixed, const KernelArgs& a, bool bwd, int grid, hipStream_t st) {
  [[maybe_unused]] const int fam = jet_wide_act_family(a);
#if !defined(PINN_DEV)
#define PINN_FCASE(A_) \
  if (fam == A_ && fixed) return coef ? launch_jetumfc_a##A_(a, grid, st) : launch_jetumf_a##A_(a, bwd, grid, st);
#define PINN_MCASE(A_) \
  if (fam == A_) return coef ? launch_jetumc_a##A_(a, grid, st) : launch_jetum_a##A_(a, bwd, grid, st);
  PINN_FCASE(0) PINN_FCASE(2) PINN_FCASE(4)
  PINN_MCASE(0) PINN_MCASE(1) PINN_MCASE(2) PINN_MCASE(3) PINN_MCASE(4)
#undef PINN_MCASE
#undef PINN_FCASE
#elif defined(PINN_DEV_MERGED)
  if (!coef && fam == 0) return fixed ? launch_jetumf_a0(a, bwd, grid, st) : launch_jetum_a0(a, bwd, grid, st);
#endif
  return hipErrorInvalidValue;
}

// reverse launch of a COEF unit: the 16-point kernel (u16) or the 32-point one
static hipError_t dispatch_coef(bool u16, int nt, int nx, const KernelArgs& a, int grid, hipStream_t st) {
#ifndef PINN_DEV
  const int fam = jet_wide_act_family(a);
#define PINN_CCASE1(P_, NT_, NX_, A_) \
  if (nt == NT_ && nx == NX_ && fam == A_) return launch_jet##P_##_##NT_##_##NX_##_a##A_(a, grid, st);
#define PINN_CCASE(P_, NT_, NX_) PINN_CCASE1(P_, NT_, NX_, 0) PINN_CCASE1(P_, NT_, NX_, 1) PINN_CCASE1(P_, NT_, NX_, 2) PINN_CCASE1(P_, NT_, NX_, 3) PINN_CCASE1(P_, NT_, NX_, 4)
  if (u16) {
    PINN_CCASE(uc, 1, 1) PINN_CCASE(uc, 1, 2) PINN_CCASE(uc, 2, 0)
  } else {
    PINN_CCASE(wc, 1, 1) PINN_CCASE(wc, 1, 2) PINN_CCASE(wc, 1, 4) PINN_CCASE(wc, 2, 0) PINN_CCASE(wc, 2, 2)
  }
#undef PINN_CCASE
#undef PINN_CCASE1
#endif
  return hipErrorInvalidValue;
}

static hipError_t dispatch_u16(int nt, int nx, const KernelArgs& a, bool bwd, int grid, hipStream_t st) {
  const int fam = jet_wide_act_family(a);
#define PINN_UCASE1(NT_, NX_, A_) \
  if (nt == NT_ && nx == NX_ && fam == A_) return launch_jetu_##NT_##_##NX_##_a##A_(a, bwd, grid, st);
#ifdef PINN_DEV
#define PINN_UCASE(NT_, NX_) PINN_UCASE1(NT_, NX_, 0)
  PINN_UCASE(PINN_DEV_NT, PINN_DEV_NX)
#else
#define PINN_UCASE(NT_, NX_) PINN_UCASE1(NT_, NX_, 0) PINN_UCASE1(NT_, NX_, 1) PINN_UCASE1(NT_, NX_, 2) PINN_UCASE1(NT_, NX_, 3) PINN_UCASE1(NT_, NX_, 4)
  PINN_UCASE(0, 0) PINN_UCASE(1, 0) PINN_UCASE(1, 1) PINN_UCASE(1, 2) PINN_UCASE(2, 0)
#endif
#undef PINN_UCASE
#undef PINN_UCASE1
  return hipErrorInvalidValue;
}

// floats of the global tape a launch of the fused kernel uses: the 32-point kernel's reverse sweep re-reads its
// records from the workspace, the 16-point kernel keeps them in LDS and puts the flush slab at the workspace's start
static size_t wide_tape_floats(const PinnNetDesc* d, const NetDev& n, int nt, int nx, bool bwd, int grid, bool coef = false) {
  if (!bwd || use_u16(d, n, nt, nx, bwd, coef)) return 0;
  return (size_t)jet_tape_floats_per_wg(1 + nt + nx, n.n_layers, 1) * grid;
}

static int wide_grid(const NetDev& n, int K, long long N, bool bwd) {
  (void)n;
  (void)K;
  (void)bwd;
  const long long ntiles = (N + kT - 1) / kT;
  long long g = num_cus();
  if (g > ntiles) g = ntiles;
  return (int)(g < 1 ? 1 : g);
}

static int validate_table(const PinnNetDesc* net, const void* table, int num_tensors, const char* what) {
  if (!net) return fail(PINN_ERR_BAD_DESC, "null descriptor");
  const int want = lm::lm_expected_tensors(net);
  if (want < 0) return fail(PINN_ERR_UNSUPPORTED, "architecture id %d has no kernel", net->arch);
  if (!table) return fail(PINN_ERR_BAD_DESC, "%s table is null", what);
  if (num_tensors != want)
    return fail(PINN_ERR_BAD_DESC, "%s table has %d entries; the state_dict of this architecture has %d", what, num_tensors, want);
  return PINN_OK;
}

static int run(const PinnNetDesc* net, const float* const* weights, float* const* grads, int num_tensors,
               const PinnPdeDesc* pde, const float* x, const float* t, int64_t N, int nt, int nx, int mode,
               float grad_scale, float* const* jets_out, const float* const* jets_bar, float* residual_out,
               float* loss_sum, void* workspace, size_t ws_bytes, bool bwd, void* stream, const float* res_bar = nullptr,
               float* coef_grads = nullptr, float* x_grad = nullptr, float* t_grad = nullptr, bool lm_only = false,
               const float* coef_dev = nullptr) {
  int rc = validate_table(net, weights, num_tensors, "weights");
  if (rc) return rc;
  if (bwd && grads && (rc = validate_table(net, grads, num_tensors, "weight_grads"))) return rc;  // null only where the entry point allows it
  if (N <= 0) return PINN_OK;
  if (!x && net->input_dim > 1) return fail(PINN_ERR_BAD_DESC, "x is null");
  if (!t) return fail(PINN_ERR_BAD_DESC, "t is null");
  if ((rc = check_orders(nt, nx))) return rc;
  if (!stream_set_admitted(net, nt, nx)) return fail(PINN_ERR_UNSUPPORTED, "stream set (nt=%d, nx=%d) is not compiled", nt, nx);
  char lerr[256] = "";
  if ((rc = lm::lm_check(net, lerr, sizeof(lerr)))) return fail(rc, "%s", lerr);
  const int K = 1 + nt + nx;
  PdeDev pd;
  memset(&pd, 0, sizeof(pd));
  if (pde) {
    pd.kind = pde->kind;
    pd.dimension = pde->dimension;
    pd.loss = pde->loss;
    pd.c0 = pde->coef[0];
    pd.c1 = pde->coef[1];
    pd.c2 = pde->coef[2];
    pd.c3 = pde->coef[3];
    pd.huber_delta = pde->huber_delta;
    pd.dcoef = bwd ? coef_grads : nullptr;
    pd.coef_dev = coef_dev;
  }
  const bool inverse = coef_dev != nullptr;  // pinn_residual_loss_grad_inverse: COEF units, coefficients from the device
  KernelArgs a;
  memset(&a, 0, sizeof(a));
  int misaligned = -1;
  // Coefficient cotangents (inverse problems) are a reduction of the layer-major engine's head kernel only: in the fused
  // tile-major kernel the extra per-tile code cost the headline configuration scratch (SGPR spills to memory) even with the
  // feature off, so such calls take the layer-major engine — which the caller selects (PINN_FLAG_LAYER_MAJOR) so that
  // pinn_workspace_bytes sizes the workspace for it.
  if (!inverse && coef_grads && !(net->flags & PINN_FLAG_LAYER_MAJOR) && !force_lm() && use_wide(net, nullptr, nullptr, K, bwd, &a.net))
    return fail(PINN_ERR_UNSUPPORTED, "coefficient gradients run on the layer-major engine: set PINN_FLAG_LAYER_MAJOR in the "
                "descriptor for this call and for its pinn_workspace_bytes query");
  bool wide = !lm_only && use_wide(net, weights, grads, K, bwd, &a.net, &misaligned);
  if (!wide && misaligned >= 0)  // pinn_workspace_bytes sized this descriptor for the fused kernel: say what is wrong instead of "workspace too small"
    return fail(PINN_ERR_MISALIGNED, "weight tensor %d is not 16-byte aligned: the fused kernel of this descriptor reads hidden-layer "
                "weights with 16-byte loads (pass aligned tensors, or set PINN_FLAG_LAYER_MAJOR to take the packing engine)", misaligned);
  if (inverse && !widec_set_compiled(nt, nx)) wide = false;  // no COEF unit of this stream set: layer-major engine
  if (wide) {
    const int grid = wide_grid(a.net, K, N, bwd);
    a.pde = pd;
    a.x = x;
    a.t = t;
    a.N = N;
    a.mode = mode;
    a.grad_scale = grad_scale;
    for (int s = 0; s < K; ++s) {
      a.jets_out[s] = jets_out ? jets_out[s] : nullptr;
      a.jets_bar[s] = jets_bar ? jets_bar[s] : nullptr;
    }
    a.residual_out = residual_out;
    a.loss_sum = loss_sum;
    a.res_bar = res_bar;
#ifdef PINN_STAMPS
    a.stamps = g_stamps;
#endif
    // Default mode of a reverse launch: TWO-LEVEL flush.  Workgroup b adds (atomically) into row b mod 8 of an 8-row
    // slab and a small launch sums the rows into the caller's tensors: 32 instead of 256 workgroups contend for an
    // address.  Measured on the headline launch (kernel + memset + row sum, events around the call): direct atomics
    // 0.554 ms, 2 rows 0.553, 4 rows 0.549, 8 rows 0.543, 16 rows 0.545, 32 rows 0.550, 64 rows 0.567.
    // Networks whose MFMA layers all keep their weight-gradient tiles in registers (n_layers <= kPersist: nothing is
    // flushed inside the tile loop) take the STORE flush instead, in both modes: one slab row per workgroup, written
    // with plain stores, then wide_rows_reduce.  The last workgroups of a launch no longer spend 32 us adding 160 KB
    // at the memory-side atomic rate, and the slab needs no memset (jet_kernel_wide.h, end of the kernel).
    const WideFlush flush = wide_flush(net, a.net, grid, bwd);
    const bool store_flush = flush == FLUSH_STORE;
    const bool two_level = flush == FLUSH_TWO_LEVEL;
    const bool det = flush != FLUSH_DIRECT;
    const int slab_rows = wide_slab_rows(flush, grid);
    const bool u16 = use_u16(net, a.net, nt, nx, bwd, inverse);
    const size_t tape_floats = wide_tape_floats(net, a.net, nt, nx, bwd, grid, inverse);
    size_t need = tape_floats * sizeof(float);
    DetTable dt;
    dt.n = 0;
    if (det) {
      NetDev probe = a.net;
      float* lprobe = a.loss_sum;
      float* cprobe = a.pde.dcoef;
      det_redirect(probe, lprobe, cprobe, nullptr, dt);  // sizing pass: the same stride pinn_workspace_bytes reports
      need += (size_t)dt.stride * slab_rows * sizeof(float);
    }
    if (need > 0 && (!workspace || ws_bytes < need))
      return fail(PINN_ERR_WORKSPACE, "workspace too small: need %zu bytes, got %zu", need, ws_bytes);
    if (need > 0 && (reinterpret_cast<uintptr_t>(workspace) & 15)) return fail(PINN_ERR_MISALIGNED, "workspace is not 16-byte aligned");
    if (tape_floats > 0) {
      a.tape_stride = jet_tape_floats_per_wg(K, a.net.n_layers, 1);
      a.tape = static_cast<float*>(workspace);
    }
    float* slab = nullptr;
    if (det) {
      const unsigned stride = dt.stride;
      slab = static_cast<float*>(workspace) + tape_floats;
      det_redirect(a.net, a.loss_sum, a.pde.dcoef, slab, dt);
      dt.stride = stride;  // rows are as wide as the sizing pass said, whatever subset of targets this call has
      a.det_stride = two_level ? -(long long)stride : (long long)stride;
      a.det_mask = slab_rows - 1;
      a.flush_store = store_flush ? 1 : 0;
      if (!store_flush) {
        const hipError_t em = hipMemsetAsync(slab, 0, (size_t)stride * slab_rows * sizeof(float), static_cast<hipStream_t>(stream));
        if (em != hipSuccess) return fail(PINN_ERR_HIP, "HIP error %d: %s", (int)em, hipGetErrorString(em));
      }
    }
    const bool merged = u16 && use_merged(net, a.net, pde, nt, nx, mode);
    if (u16) jet_u16_set_plan(a, grid, merged ? u16m_unit_packed(a.net, inverse) : u16_unit_packed(a.net, nt, nx, inverse));
    const bool fixed = use_fixed_shape(net, a.net, merged);  // same plan, LDS size and results as the generic merged unit
    hipError_t e = merged  ? dispatch_u16m(inverse, fixed, a, bwd, grid, static_cast<hipStream_t>(stream))
                   : inverse ? dispatch_coef(u16, nt, nx, a, grid, static_cast<hipStream_t>(stream))
                   : u16   ? dispatch_u16(nt, nx, a, bwd, grid, static_cast<hipStream_t>(stream))
                           : dispatch_wide(nt, nx, a, bwd, grid, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(PINN_ERR_HIP, "HIP error %d: %s", (int)e, hipGetErrorString(e));
    if (det && dt.n > 0 && store_flush) {
      hipLaunchKernelGGL(wide_rows_reduce, dim3(136, dt.n), dim3(256), 0, static_cast<hipStream_t>(stream), dt, slab, slab_rows);
      e = hipGetLastError();
      if (e != hipSuccess) return fail(PINN_ERR_HIP, "HIP error %d: %s", (int)e, hipGetErrorString(e));
    } else if (det && dt.n > 0) {
      hipLaunchKernelGGL(wide_det_reduce, dim3(32, dt.n), dim3(256), 0, static_cast<hipStream_t>(stream), dt, slab, slab_rows);
      e = hipGetLastError();
      if (e != hipSuccess) return fail(PINN_ERR_HIP, "HIP error %d: %s", (int)e, hipGetErrorString(e));
    }
    return PINN_OK;
  }
  lm::CallArgs c;
  memset(&c, 0, sizeof(c));
  c.net = net;
  c.weights = weights;
  c.grads = grads;
  c.num_tensors = num_tensors;
  c.pde = pd;
  c.x = x;
  c.t = t;
  c.N = N;
  c.nt = nt;
  c.nx = nx;
  c.mode = mode;
  c.grad_scale = grad_scale;
  c.jets_out = jets_out;
  c.jets_bar = jets_bar;
  c.residual_out = residual_out;
  c.loss_sum = loss_sum;
  c.res_bar = res_bar;
  c.workspace = workspace;
  c.ws_bytes = ws_bytes;
  c.bwd = bwd;
  c.deterministic = (net->flags & PINN_FLAG_DETERMINISTIC) != 0;
  c.stream = static_cast<hipStream_t>(stream);
  c.x_grad = x_grad;
  c.t_grad = t_grad;
  rc = lm::lm_run(c, lerr, sizeof(lerr));
  if (rc) return fail(rc, "%s", lerr);
  return PINN_OK;
}

}  // namespace pinn

using namespace pinn;

extern "C" {

int pinn_abi_version(void) { return PINN_ABI_VERSION; }

const char* pinn_last_error(void) { return g_err; }

int pinn_num_tensors(const PinnNetDesc* net) {
  if (!net) return fail(PINN_ERR_BAD_DESC, "null descriptor");
  const int n = lm::lm_expected_tensors(net);
  if (n < 0) return fail(PINN_ERR_UNSUPPORTED, "architecture id %d has no kernel", net->arch);
  char lerr[256] = "";
  const int rc = lm::lm_check(net, lerr, sizeof(lerr));
  if (rc) return fail(rc, "%s", lerr);
  return n;
}

int pinn_pde_streams(const PinnPdeDesc* pde, int32_t* time_order, int32_t* space_order) {
  if (!pde || !time_order || !space_order) return fail(PINN_ERR_BAD_DESC, "null argument");
  int nt = 1, nx = 0;
  if (pde->dimension > 1 && pde->kind == PINN_PDE_CONVECTION)  // convection_equation.py:66-76 differentiates u w.r.t. a SLICE of x: torch raises
    return fail(PINN_ERR_UNSUPPORTED, "convection with dimension %d: the reference's residual raises for dimension > 1", pde->dimension);
  if (pde->dimension > 1) {
    nt = (pde->kind == PINN_PDE_WAVE || pde->kind == PINN_PDE_PENDULUM) ? 2 : 1;
  } else {
    switch (pde->kind) {
      case PINN_PDE_BURGERS: case PINN_PDE_ALLEN_CAHN: case PINN_PDE_BLACK_SCHOLES: case PINN_PDE_HEAT_LAPLACIAN: nt = 1; nx = 2; break;
      case PINN_PDE_HEAT: case PINN_PDE_CONVECTION: nt = 1; nx = 1; break;
      case PINN_PDE_KDV: nt = 1; nx = 3; break;
      case PINN_PDE_CAHN_HILLIARD: nt = 1; nx = 4; break;
      case PINN_PDE_WAVE: nt = 2; nx = 2; break;
      case PINN_PDE_PENDULUM: nt = 2; nx = 0; break;
      default: return fail(PINN_ERR_BAD_DESC, "unknown pde kind %d", pde->kind);
    }
  }
  *time_order = nt;
  *space_order = nx;
  return PINN_OK;
}

size_t pinn_workspace_bytes(const PinnNetDesc* net, int64_t N, int32_t time_order, int32_t space_order, int32_t backward) {
  if (!net || N <= 0) return 0;
  if (time_order < 0 || time_order > 2 || space_order < 0 || space_order > 4) return 0;
  char lerr[64];
  if (lm::lm_check(net, lerr, sizeof(lerr)) != PINN_OK) return 0;
  const int K = 1 + time_order + space_order;
  const bool bwd = backward != 0;
  NetDev n;
  if (backward != 2 && use_wide(net, nullptr, nullptr, K, bwd, &n)) {  // 2: pinn_jet_backward_inputs, always layer-major
    const int grid = wide_grid(n, K, N, bwd);
    // the 32-point kernel's size even where the 16-point kernel runs (it needs only the slab): a caller can switch
    // between the two with PINN_FLAG_WIDE_TILE32 on the same workspace
    size_t bytes = bwd ? (size_t)jet_tape_floats_per_wg(K, n.n_layers, 1) * sizeof(float) * grid : 0;
    const int rows = wide_slab_rows(wide_flush(net, n, grid, bwd), grid);
    if (rows > 0) {
      DetTable dt;
      float* lprobe = nullptr;
      float* cprobe = nullptr;
      det_redirect(n, lprobe, cprobe, nullptr, dt);
      bytes += (size_t)dt.stride * rows * sizeof(float);
    }
    return bytes;
  }
  return lm::lm_workspace_bytes(net, N, time_order, space_order, bwd, (net->flags & PINN_FLAG_DETERMINISTIC) != 0);
}

int pinn_kernel_for(const PinnNetDesc* net, int64_t N, int32_t time_order, int32_t space_order, int32_t backward,
                    PinnKernelInfo* out) {
  if (!net || !out) return fail(PINN_ERR_BAD_DESC, "null argument");
  if (N <= 0) return fail(PINN_ERR_BAD_DESC, "N = %lld: a call on no points launches nothing", (long long)N);
  if (backward < 0 || backward > 2) return fail(PINN_ERR_BAD_DESC, "backward = %d: 0, 1 or 2", backward);
  int rc = check_orders(time_order, space_order);
  if (rc) return rc;
  if (!stream_set_admitted(net, time_order, space_order))
    return fail(PINN_ERR_UNSUPPORTED, "stream set (nt=%d, nx=%d) is not compiled", time_order, space_order);
  char lerr[256] = "";
  if ((rc = lm::lm_check(net, lerr, sizeof(lerr)))) return fail(rc, "%s", lerr);
  PinnKernelInfo r;
  memset(&r, 0, sizeof(r));
  r.time_order = time_order;
  r.space_order = space_order;
  r.backward = backward;
  r.act_family = r.hmax = r.na0 = r.grid = r.flush = -1;
  const int K = 1 + time_order + space_order;
  const bool bwd = backward != 0;
  NetDev n;
  if (backward != 2 && use_wide(net, nullptr, nullptr, K, bwd, &n)) {  // the decisions run() makes, in the same helpers
    r.engine = 1;
    r.act_family = jet_wide_act_family(n);
    jet_wide_variant(n, bwd, &r.hmax, &r.na0);
    r.grid = wide_grid(n, K, N, bwd);
    r.flush = wide_flush(net, n, r.grid, bwd);
    char unit[64];  // pinn_build_info() lists the units built in the default MFMA form as "jet_wide_<nt>_<nx>_<family>: ..."
    snprintf(unit, sizeof(unit), "jet_wide_%d_%d_%d:", time_order, space_order, r.act_family);
    r.default_mfma_form = strstr(pinn_build_info(), unit) != nullptr;
  }
  *out = r;
  return PINN_OK;
}

int pinn_lm_plan(const PinnNetDesc* net, int64_t N, int32_t time_order, int32_t space_order, int32_t backward,
                 PinnLmNodePlan* out, int32_t max_records) {
  PinnKernelInfo r;  // the checks of pinn_kernel_for: descriptor, orders, compiled stream set
  int rc = pinn_kernel_for(net, N, time_order, space_order, backward, &r);
  if (rc) return rc;
  char lerr[256] = "";
  rc = lm::lm_plan(net, time_order, space_order, backward, out, max_records, lerr, sizeof(lerr));
  if (rc < 0) return fail(rc, "%s", lerr);
  return rc;
}

int pinn_kernel_name(const PinnNetDesc* net, int64_t N, int32_t time_order, int32_t space_order, int32_t backward,
                     char* buf, size_t len) {
  if (!buf || len == 0) return fail(PINN_ERR_BAD_DESC, "null or empty name buffer");
  PinnKernelInfo r;
  const int rc = pinn_kernel_for(net, N, time_order, space_order, backward, &r);
  if (rc) return rc;
  const char* name = "layer_major";
  if (r.engine == 1) {
    NetDev n;
    build_wide(net, nullptr, nullptr, &n);
    name = use_u16(net, n, time_order, space_order, backward == 1) ? "jet_kernel_u16" : "jet_kernel_wide";
  }
  snprintf(buf, len, "%s", name);
  return PINN_OK;
}

int pinn_residual_unit_name(const PinnNetDesc* net, const PinnPdeDesc* pde, int64_t N, char* buf, size_t len) {
  int32_t nt, nx;
  int rc = pinn_pde_streams(pde, &nt, &nx);
  if (rc) return rc;
  rc = pinn_kernel_name(net, N, nt, nx, 1, buf, len);
  if (rc || strcmp(buf, "jet_kernel_u16") != 0) return rc;
  NetDev n;
  build_wide(net, nullptr, nullptr, &n);
  const int fam = jet_wide_act_family(n);
  const bool merged = use_merged(net, n, pde, nt, nx, MODE_PDE);  // the decisions run() makes, in the same helpers
  if (use_fixed_shape(net, n, merged)) snprintf(buf, len, "jet_u16mf_%d", fam);
  else if (merged) snprintf(buf, len, "jet_u16m_%d", fam);
  else snprintf(buf, len, "jet_u16_%d_%d_%d", (int)nt, (int)nx, fam);
  return PINN_OK;
}

int pinn_unit_tail_plan(int64_t N, int32_t grid, int64_t* rounds, int32_t* groups, int64_t* first_tail_point) {
  if (N < 0 || grid < 1) return fail(PINN_ERR_BAD_DESC, "pinn_unit_tail_plan: N = %lld, grid = %d", (long long)N, (int)grid);
  const U16Plan p = jet_u16_tail_plan(N, grid, true);
  if (rounds) *rounds = p.rounds;
  if (groups) *groups = p.groups;
  if (first_tail_point) *first_tail_point = p.first_tail;
  return PINN_OK;
}

int pinn_jet_forward(const PinnNetDesc* net, const float* const* weights, int32_t num_tensors, const float* x,
                     const float* t, int64_t N, int32_t time_order, int32_t space_order, float* const* jets_out,
                     void* workspace, size_t ws_bytes, void* stream) {
  if (!jets_out) return fail(PINN_ERR_BAD_DESC, "jets_out is null");
  return run(net, weights, nullptr, num_tensors, nullptr, x, t, N, time_order, space_order, MODE_JETS, 0.0f, jets_out,
             nullptr, nullptr, nullptr, workspace, ws_bytes, false, stream);
}

int pinn_jet_backward(const PinnNetDesc* net, const float* const* weights, int32_t num_tensors, const float* x,
                      const float* t, int64_t N, int32_t time_order, int32_t space_order,
                      const float* const* jet_cotangents, float* const* weight_grads, void* workspace, size_t ws_bytes,
                      void* stream) {
  if (!jet_cotangents || !weight_grads) return fail(PINN_ERR_BAD_DESC, "null cotangents or weight_grads");
  return run(net, weights, weight_grads, num_tensors, nullptr, x, t, N, time_order, space_order, MODE_JETS, 0.0f, nullptr,
             jet_cotangents, nullptr, nullptr, workspace, ws_bytes, true, stream);
}

// The layer-major engine whatever the descriptor's flags say (the fused tile-major kernel has no input cotangents; the
// descriptor is not modified); pinn_workspace_bytes(..., backward = 2) sizes it.
int pinn_jet_backward_inputs(const PinnNetDesc* net, const float* const* weights, int32_t num_tensors, const float* x,
                             const float* t, int64_t N, int32_t time_order, int32_t space_order,
                             const float* const* jet_cotangents, float* const* weight_grads, float* x_grad, float* t_grad,
                             void* workspace, size_t ws_bytes, void* stream) {
  if (!jet_cotangents) return fail(PINN_ERR_BAD_DESC, "null cotangents");
  if (net && weight_grads) {
    const int rc = validate_table(net, weight_grads, num_tensors, "weight_grads");
    if (rc) return rc;
  }
  if (net && net->input_dim <= 1) x_grad = nullptr;  // no spatial column
  if (!weight_grads && !x_grad && !t_grad) {  // nothing requested: validate, launch nothing
    int rc = validate_table(net, weights, num_tensors, "weights");
    if (rc || N <= 0) return rc;
    if ((rc = check_orders(time_order, space_order))) return rc;
    if (!stream_set_admitted(net, time_order, space_order))
      return fail(PINN_ERR_UNSUPPORTED, "stream set (nt=%d, nx=%d) is not compiled", time_order, space_order);
    char lerr[256] = "";
    if ((rc = lm::lm_check(net, lerr, sizeof(lerr)))) return fail(rc, "%s", lerr);
    return PINN_OK;
  }
  return run(net, weights, weight_grads, num_tensors, nullptr, x, t, N, time_order, space_order, MODE_JETS, 0.0f, nullptr,
             jet_cotangents, nullptr, nullptr, workspace, ws_bytes, true, stream, nullptr, nullptr, x_grad, t_grad, true);
}

int pinn_residual_forward(const PinnNetDesc* net, const float* const* weights, int32_t num_tensors,
                          const PinnPdeDesc* pde, const float* x, const float* t, int64_t N, float* residual_out,
                          float* loss_sum_out, void* workspace, size_t ws_bytes, void* stream) {
  int32_t nt, nx;
  int rc = refuse_axis(net, "pinn_residual_forward");
  if (rc) return rc;
  rc = pinn_pde_streams(pde, &nt, &nx);
  if (rc) return rc;
  return run(net, weights, nullptr, num_tensors, pde, x, t, N, nt, nx, MODE_PDE, 0.0f, nullptr, nullptr, residual_out,
             loss_sum_out, workspace, ws_bytes, false, stream);
}

int pinn_residual_loss_grad(const PinnNetDesc* net, const float* const* weights, int32_t num_tensors,
                            const PinnPdeDesc* pde, const float* x, const float* t, int64_t N, float grad_scale,
                            float* residual_out, float* loss_sum_out, float* const* weight_grads, void* workspace,
                            size_t ws_bytes, void* stream) {
  if (!weight_grads) return fail(PINN_ERR_BAD_DESC, "weight_grads is null");
  int32_t nt, nx;
  int rc = refuse_axis(net, "pinn_residual_loss_grad");
  if (rc) return rc;
  rc = pinn_pde_streams(pde, &nt, &nx);
  if (rc) return rc;
  return run(net, weights, weight_grads, num_tensors, pde, x, t, N, nt, nx, MODE_PDE, grad_scale, nullptr, nullptr,
             residual_out, loss_sum_out, workspace, ws_bytes, true, stream);
}

int pinn_residual_loss_grad_coef(const PinnNetDesc* net, const float* const* weights, int32_t num_tensors,
                                 const PinnPdeDesc* pde, const float* x, const float* t, int64_t N, float grad_scale,
                                 float* residual_out, float* loss_sum_out, float* const* weight_grads, float* coef_grads,
                                 void* workspace, size_t ws_bytes, void* stream) {
  if (!weight_grads) return fail(PINN_ERR_BAD_DESC, "weight_grads is null");
  int32_t nt, nx;
  int rc = refuse_axis(net, "pinn_residual_loss_grad_coef");
  if (rc) return rc;
  rc = pinn_pde_streams(pde, &nt, &nx);
  if (rc) return rc;
  return run(net, weights, weight_grads, num_tensors, pde, x, t, N, nt, nx, MODE_PDE, grad_scale, nullptr, nullptr,
             residual_out, loss_sum_out, workspace, ws_bytes, true, stream, nullptr, coef_grads);
}

// 0 layer-major, 1 jet_kernel_wide, 2 jet_kernel_u16: the engine a pinn_residual_loss_grad_inverse call takes (run()'s
// decisions with the COEF units in place of the plain ones); n receives the wide program when the answer is not 0
static int inverse_route(const PinnNetDesc* net, int nt, int nx, NetDev* n) {
  if (!widec_set_compiled(nt, nx) || !use_wide(net, nullptr, nullptr, 1 + nt + nx, true, n)) return 0;
  return use_u16(net, *n, nt, nx, true, true) ? 2 : 1;
}

static int inverse_query(const PinnNetDesc* net, const PinnPdeDesc* pde, int64_t N, int32_t* nt, int32_t* nx) {
  if (!net || !pde) return fail(PINN_ERR_BAD_DESC, "null descriptor");
  if (N <= 0) return fail(PINN_ERR_BAD_DESC, "N = %lld: a call on no points launches nothing", (long long)N);
  int rc = refuse_axis(net, "pinn_residual_loss_grad_inverse");
  if (rc) return rc;
  rc = pinn_pde_streams(pde, nt, nx);
  if (rc) return rc;
  if (!stream_set_compiled(*nt, *nx)) return fail(PINN_ERR_UNSUPPORTED, "stream set (nt=%d, nx=%d) is not compiled", *nt, *nx);
  char lerr[256] = "";
  if ((rc = lm::lm_check(net, lerr, sizeof(lerr)))) return fail(rc, "%s", lerr);
  return PINN_OK;
}

int pinn_residual_loss_grad_inverse(const PinnNetDesc* net, const float* const* weights, int32_t num_tensors,
                                    const PinnPdeDesc* pde, const float* coef_values, const float* x, const float* t,
                                    int64_t N, float grad_scale, float* residual_out, float* loss_sum_out,
                                    float* const* weight_grads, float* coef_grads, void* workspace, size_t ws_bytes,
                                    void* stream) {
  if (!weight_grads) return fail(PINN_ERR_BAD_DESC, "weight_grads is null");
  if (!coef_values) return fail(PINN_ERR_BAD_DESC, "coef_values is null: the coefficients of this call live on the device");
  int32_t nt, nx;
  int rc = refuse_axis(net, "pinn_residual_loss_grad_inverse");
  if (rc) return rc;
  rc = pinn_pde_streams(pde, &nt, &nx);
  if (rc) return rc;
  PinnPdeDesc p = *pde;  // pde->coef is ignored: every value comes from coef_values at launch time
  p.coef[0] = p.coef[1] = p.coef[2] = p.coef[3] = 0.0f;
  return run(net, weights, weight_grads, num_tensors, &p, x, t, N, nt, nx, MODE_PDE, grad_scale, nullptr, nullptr,
             residual_out, loss_sum_out, workspace, ws_bytes, true, stream, nullptr, coef_grads, nullptr, nullptr, false,
             coef_values);
}

size_t pinn_inverse_workspace_bytes(const PinnNetDesc* net, const PinnPdeDesc* pde, int64_t N) {
  int32_t nt, nx;
  if (inverse_query(net, pde, N, &nt, &nx) != PINN_OK) return 0;
  NetDev n;
  if (inverse_route(net, nt, nx, &n) == 0)
    return lm::lm_workspace_bytes(net, N, nt, nx, true, (net->flags & PINN_FLAG_DETERMINISTIC) != 0);
  // as pinn_workspace_bytes(net, N, nt, nx, 1): the 32-point kernel's size even where the 16-point kernel runs
  const int K = 1 + nt + nx;
  const int grid = wide_grid(n, K, N, true);
  size_t bytes = (size_t)jet_tape_floats_per_wg(K, n.n_layers, 1) * sizeof(float) * grid;
  const int rows = wide_slab_rows(wide_flush(net, n, grid, true), grid);
  if (rows > 0) {
    DetTable dt;
    float* lprobe = nullptr;
    float* cprobe = nullptr;
    det_redirect(n, lprobe, cprobe, nullptr, dt);
    bytes += (size_t)dt.stride * rows * sizeof(float);
  }
  return bytes;
}

int pinn_inverse_kernel_name(const PinnNetDesc* net, const PinnPdeDesc* pde, int64_t N, char* buf, size_t len) {
  if (!buf || len == 0) return fail(PINN_ERR_BAD_DESC, "null or empty name buffer");
  int32_t nt, nx;
  const int rc = inverse_query(net, pde, N, &nt, &nx);
  if (rc) return rc;
  NetDev n;
  const int route = inverse_route(net, nt, nx, &n);
  snprintf(buf, len, "%s", route == 2 ? "jet_kernel_u16" : route == 1 ? "jet_kernel_wide" : "layer_major");
  return PINN_OK;
}

int pinn_residual_backward(const PinnNetDesc* net, const float* const* weights, int32_t num_tensors,
                           const PinnPdeDesc* pde, const float* x, const float* t, int64_t N,
                           const float* residual_cotangent, float* const* weight_grads, void* workspace,
                           size_t ws_bytes, void* stream) {
  if (!weight_grads || !residual_cotangent) return fail(PINN_ERR_BAD_DESC, "null cotangent or weight_grads");
  int32_t nt, nx;
  int rc = refuse_axis(net, "pinn_residual_backward");
  if (rc) return rc;
  rc = pinn_pde_streams(pde, &nt, &nx);
  if (rc) return rc;
  return run(net, weights, weight_grads, num_tensors, pde, x, t, N, nt, nx, MODE_PDE, 0.0f, nullptr, nullptr, nullptr,
             nullptr, workspace, ws_bytes, true, stream, residual_cotangent);
}

#ifdef PINN_STAMPS
/* Diagnostic builds only (make dev STAMPS=1): device buffer of grid*4*16 uint64 for the in-kernel phase timers. */
void pinn_debug_set_stamps(void* device_buffer) { g_stamps = static_cast<unsigned long long*>(device_buffer); }
#endif

}  // extern "C"
