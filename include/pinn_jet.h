/*
 * pinn_jet.h — C ABI of the MI355X (gfx950) PINN jet engine.
 *
 * The reference (pinnrl 0.3.1) has no FFI: its boundary for this path is the
 * Python object API.  Each entry point below replaces the ATen op sequence that
 * one reference call site generates; the Python host mirror binds them with
 * ctypes (see INTEGRATION.md for the stub a pinnrl maintainer would add).
 *
 *   pinn_jet_forward         <- PINNModel.forward (pinnrl/neural_networks/__init__.py:144-154)
 *                               + PDEBase.compute_derivatives (pinnrl/pdes/pde_base.py:590-794):
 *                               u and its input derivatives ("jets") in one launch.
 *   pinn_jet_backward        <- loss.backward() through that graph (pinnrl/training/trainer.py:689):
 *                               d(sum_s <cotangent_s, jet_s>)/d(theta), accumulated into weight_grads.
 *   pinn_jet_backward_inputs <- torch.autograd.grad(u, (x, t)) through the same graph (pinnrl/pdes/allen_cahn.py:50-108,
 *                               heat_equation.py:425-445, pde_base.py:640-794): the same reverse sweep, plus the
 *                               cotangents of the coordinates; weight gradients optional.
 *   pinn_residual_forward    <- XxxEquation.compute_residual (pinnrl/pdes/burgers_equation.py:40-75,
 *                               heat_equation.py:54-110, allen_cahn.py:39-111, kdv_equation.py:38-92,
 *                               cahn_hilliard.py:39-160, wave_equation.py:38-119,
 *                               convection_equation.py:43-78, black_scholes.py:44-93,
 *                               pendulum_equation.py:51-94) + PDEBase._apply_loss_fn
 *                               (pde_base.py:309-326) as a fused per-point epilogue.
 *   pinn_residual_backward   <- loss.backward() through a residual tensor (trainer.py:689, :607-626).
 *   pinn_residual_loss_grad  <- the metric's unit of work: compute_residual -> mean loss -> backward,
 *                               one launch (pde_base.py:1098-1099 + trainer.py:689).
 *
 * Conventions: fp32, contiguous.  x:(N,dim) row-major, t:(N,1); the network input is
 * cat([x,t],1) — spatial columns first, time LAST (pde_base.py:640).  All pointers are
 * device pointers owned by the caller (PyTorch); the library never allocates, frees or
 * retains device memory and launches on the stream it is given without synchronising.
 * Return value: 0 = ok, negative = PinnStatus; pinn_last_error() describes the failure
 * (thread-local).  `weights` / `weight_grads` follow the reference's state_dict order
 * for the architecture (buffers included, e.g. fourier: B, W0, b0, ..., W_out, b_out);
 * a NULL entry in weight_grads skips that tensor.
 */
#ifndef PINN_JET_H
#define PINN_JET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PINN_ABI_VERSION 2
#define PINN_MAX_LINEAR 24
#define PINN_MAX_STREAMS 7 /* value + up to 2 time + up to 4 space derivatives */

/* PinnNetDesc.flags */
#define PINN_FLAG_LAYER_NORM 1    /* feedforward, autoencoder: a LayerNorm follows every hidden Linear (feedforward.py:43-45) */
#define PINN_FLAG_DETERMINISTIC 2 /* weight gradients (and, on calls WITH a reverse sweep, the loss sum) reduced in a fixed
                                     order: two launches on the same inputs give bit-identical results (reference anchor:
                                     tests/unit_tests/test_benchmarks.py:61-64).  Both engines: per-workgroup slab rows +
                                     ordered row sum; the workspace grows by grid x parameter count floats.  Forward-only
                                     calls: the fused tile-major kernel honours the flag for the loss sum too, the
                                     layer-major engine accumulates it with float atomics (per-point outputs are
                                     bit-reproducible either way) */
#define PINN_FLAG_LAYER_MAJOR 4   /* engine hint: run the layer-major engine even where the fused tile-major kernel
                                     applies (same results to rounding; tests run both) */
#define PINN_FLAG_WIDE_TILE32 8   /* engine hint: reverse launches of the fused tile-major kernel keep the 32-point kernel
                                     where the 16-point one would run (A/B runs and tests; same results to rounding) */
#define PINN_FLAG_PLAIN_STREAMS 16 /* engine hint: every call of the descriptor keeps one stream per derivative where the
                                      16-point kernel would run 1-D Burgers on the merged set u, u_t - nu u_xx, u_x (A/B
                                      runs and tests; same results to rounding) */
#define PINN_FLAG_GENERIC_UNITS 32 /* engine hint: every call of the descriptor keeps the merged units that read the network's
                                      shape from the descriptor where the 16-point kernel would run the units with the
                                      default shape compiled in (Fourier features 2 -> 64, three layers of 128; A/B runs and
                                      tests; the same bits) */
/* Space axis of a jet launch: with axis a (1 or 2) the space streams of pinn_jet_forward, pinn_jet_backward and
   pinn_jet_backward_inputs are d^k/dx_a^k, seeded from column a of x instead of column 0; the stream order stays
   [u, d/dt.., d/dx_a..].  The weight gradient and the input cotangents (every column, mixed terms included) stay exact.
   A non-zero axis always takes the layer-major engine (pinn_kernel_for / pinn_kernel_name report it, pinn_workspace_bytes
   sizes for it) and also admits the stream sets (0, 1) .. (0, 4), which have layer-major units only: with axis 0 those four
   sets are refused like any other uncompiled set.  axis >= input_dim - 1: PINN_ERR_BAD_DESC.  The pinn_residual_* entry
   points (the compiled PDE kinds, whose >= 2-D behaviour is the reference's) refuse a non-zero axis with
   PINN_ERR_UNSUPPORTED.  Axis bits zero: nothing changes. */
#define PINN_FLAG_SPACE_AXIS(a) ((a) << 8)
#define PINN_FLAG_SPACE_AXIS_MASK 0x300
/* Space direction of a jet launch: two bits per space axis (0 -> 0, 1 -> +1, 2 -> -1; 3 is PINN_ERR_BAD_DESC).  With the
   direction d the space streams of pinn_jet_forward, pinn_jet_backward and pinn_jet_backward_inputs are
   (sum_c d_c d/dx_c)^k u; the stream order stays [u, d/ds, d2/ds2, ..].  Mixed derivatives are fixed linear combinations of
   such streams (pinn_term_residual_mixed).  A direction launch always takes the layer-major engine (pinn_kernel_for /
   pinn_kernel_name report it; pinn_workspace_bytes sizes it as an axis launch: one N x (input_dim - 1) copy of the
   coordinates and one more on reverse calls) and admits the space-only sets (0, 1) .. (0, 4) and no other.  A non-zero
   AXIS admits (0, 3) and (0, 4) as well.  Valid: at least two non-zero entries, the first of them +1 (the negated direction
   adds nothing), none on an axis >= input_dim - 1, axis bits zero; anything else is PINN_ERR_BAD_DESC, reported by every
   query and entry point before a table entry is read.  The pinn_residual_* entry points refuse direction bits with
   PINN_ERR_UNSUPPORTED.  Direction bits zero: nothing changes.
   How it runs — the exchange of columns of an axis launch, generalised to a unimodular shear; no compute kernel differs.
   With p the first axis with d_p = +1 and s(.) the exchange of columns 0 and p, in fp32 and in exactly this order:
     packed coordinate map (the first Linear, or the rows of Fourier B):
       column 0 = W[:,p] + sum_{c != p, d_c != 0} d_c W[:,c], one add or subtract per c in ascending c; column j != 0 = W[:,s(j)];
     coordinates the kernels read: x'_0 = x_p;  x'_j = x_{s(j)} - d_{s(j)} x_p (one add or subtract);  t untouched;
     map gradient coming back: dW[:,p] += g[:,0];  dW[:,c] += g[:,s(c)] + d_c g[:,0] for c != p;
     x_grad coming back: xbar_c = xbar'_{s(c)} for c != p;  xbar_p = xbar'_0 - sum_{c != p} d_c xbar'_{s(c)}, ascending c.
   u(x) = u'(x') for every x, so the streams along column 0 of the sheared network ARE the directional derivatives of the
   network as given and every cotangent is exact.  PINN_FLAG_DETERMINISTIC holds as for an axis launch. */
#define PINN_FLAG_SPACE_DIRECTION(d0, d1, d2) \
  (((((d0) < 0 ? 2 : (d0)) & 3) << 10) | ((((d1) < 0 ? 2 : (d1)) & 3) << 12) | ((((d2) < 0 ? 2 : (d2)) & 3) << 14))
#define PINN_FLAG_SPACE_DIRECTION_MASK 0xFC00

typedef enum PinnStatus {
  PINN_OK = 0,
  PINN_ERR_BAD_DESC = -1,
  PINN_ERR_UNSUPPORTED = -2,
  PINN_ERR_MISALIGNED = -3,
  PINN_ERR_WORKSPACE = -4,
  PINN_ERR_HIP = -5,
  PINN_ERR_BAD_ORDER = -6
} PinnStatus;

typedef enum PinnArch {
  PINN_ARCH_FEEDFORWARD = 0, /* feedforward.py:9-73 (PINN_FLAG_LAYER_NORM: Linear, LayerNorm, act per hidden layer) */
  PINN_ARCH_FOURIER = 1,     /* fourier.py:65-124 */
  PINN_ARCH_SIREN = 2,       /* siren.py:49-90 */
  PINN_ARCH_RESNET = 3,      /* resnet.py:68-142 */
  PINN_ARCH_ATTENTION = 4,   /* attention.py:110-183 (sequence length 1 => an MLP with LayerNorm) */
  PINN_ARCH_AUTOENCODER = 5  /* autoencoder.py:9-100.  With n = len(hidden_dims) >= 1: num_blocks = n, num_linear = 2 n + 2,
                                widths = [h_1 .. h_n, latent_dim, h_n .. h_1, 1], activation = the hidden activation,
                                PINN_FLAG_LAYER_NORM as for feedforward.  Tensors in state_dict order: encoder.{0, 3, ..}
                                (with LayerNorm: each Linear followed by its LayerNorm at +1; without: Linears at 0, 2, ..),
                                the latent Linear, the decoder the same way, the output Linear last: 8 n + 4 tensors with
                                LayerNorm, 4 n + 4 without.  Nothing sits between the latent Linear and the first decoder
                                Linear.  num_linear != 2 num_blocks + 2: PINN_ERR_BAD_DESC; n = 0 (a purely linear model):
                                PINN_ERR_UNSUPPORTED; PINN_MAX_LINEAR caps n at 11.  Always the layer-major engine. */
} PinnArch;

typedef enum PinnAct { /* base_network.py:91-104, plus SIREN's sin(omega_0 z) */
  PINN_ACT_TANH = 0,
  PINN_ACT_SIN = 1,
  PINN_ACT_GELU = 2,
  PINN_ACT_SIGMOID = 3,
  PINN_ACT_RELU = 4,
  PINN_ACT_LEAKY_RELU = 5,
  PINN_ACT_IDENTITY = 6
} PinnAct;

typedef enum PinnPde { /* as-reference residuals; see DESIGN.md for the quirks kept */
  PINN_PDE_BURGERS = 0,       /* u_t + u u_x - c0 u_xx              c0 = nu        */
  PINN_PDE_HEAT = 1,          /* u_t - c0 u_x   (reference: "dx2" is a FIRST derivative) */
  PINN_PDE_ALLEN_CAHN = 2,    /* u_t - c0^2 u_xx - u + u^3          c0 = epsilon   */
  PINN_PDE_KDV = 3,           /* u_t + 6 u u_x + u_xxx                             */
  PINN_PDE_CAHN_HILLIARD = 4, /* u_t - d_xx(-c0^2 u_xx + c^3 - c), c = clamp(u,+-10) */
  PINN_PDE_WAVE = 5,          /* u_tt - c0^2 u_xx                                  */
  PINN_PDE_CONVECTION = 6,    /* u_t + c0 u_x                                      */
  PINN_PDE_BLACK_SCHOLES = 7, /* u_t + .5 c0^2 x^2 u_xx + c1 x u_x - c1 u  (sigma, r) */
  PINN_PDE_PENDULUM = 8,      /* u_tt + c0 sin(u)                   c0 = g/L       */
  PINN_PDE_HEAT_LAPLACIAN = 9 /* u_t - c0 u_xx  (the intended heat equation; never the parity path) */
} PinnPde;

typedef enum PinnLoss { PINN_LOSS_MSE = 0, PINN_LOSS_MAE = 1, PINN_LOSS_HUBER = 2 } PinnLoss;

typedef struct PinnNetDesc {
  int32_t arch;                    /* PinnArch */
  int32_t activation;              /* PinnAct of the hidden layers */
  int32_t input_dim;               /* spatial dimension + 1 */
  int32_t num_linear;              /* Linear layers including the output layer */
  int32_t widths[PINN_MAX_LINEAR]; /* out_features of each Linear (1 .. 1024, any value); widths[num_linear-1] must be 1 */
  int32_t mapping_size;            /* fourier: columns of B (features = 2 * mapping_size) */
  float act_param;                 /* omega_0 for PINN_ACT_SIN */
  float ln_eps;                    /* LayerNorm epsilon (resnet / attention) */
  int32_t num_blocks;              /* resnet blocks / attention layers / autoencoder hidden layers per side */
  int32_t flags;                   /* PINN_FLAG_* */
} PinnNetDesc;

typedef struct PinnPdeDesc {
  int32_t kind;      /* PinnPde */
  int32_t dimension; /* spatial dimension; >= 2 keeps only the terms the reference keeps */
  int32_t loss;      /* PinnLoss */
  float coef[4];
  float huber_delta;
} PinnPdeDesc;

int pinn_abi_version(void);
const char* pinn_last_error(void);

/* How the library was built: one line per kernel translation unit that did not build in its preferred form
 * (see csrc/Makefile), or "" — so that a degraded build is visible to callers, tests and the bench line. */
const char* pinn_build_info(void);

/* Number of tensors the reference's state_dict holds for this descriptor — the length every `weights` /
 * `weight_grads` table passed below must have (`num_tensors`).  Negative PinnStatus on a bad descriptor. */
int pinn_num_tensors(const PinnNetDesc* net);

/* (time_order, space_order) of the jet streams a PDE's residual consumes; K = 1 + nt + nx. */
int pinn_pde_streams(const PinnPdeDesc* pde, int32_t* time_order, int32_t* space_order);

/* Bytes of scratch a call on N points needs (`backward` = 0 for the forward-only entry points, 2 for
 * pinn_jet_backward_inputs — which always runs the layer-major engine — and 1 for the other entry points).
 * Zero is a valid answer (small networks run from registers and LDS alone); 0 is also returned for a descriptor the
 * library cannot run — the compute entry points then report why. */
size_t pinn_workspace_bytes(const PinnNetDesc* net, int64_t N, int32_t time_order, int32_t space_order, int32_t backward);

/* Which kernel a call on N points with stream set (time_order, space_order) takes — the decisions the compute entry points
 * make, from the same code.  `backward` as for pinn_workspace_bytes (0 forward-only, 1 reverse, 2
 * pinn_jet_backward_inputs).  No tensors are passed: the query assumes 16-byte-aligned weights (a misaligned hidden
 * weight makes the compute call fail with PINN_ERR_MISALIGNED instead).  Fields that do not apply to the layer-major
 * engine are -1 (default_mfma_form 0).  PINN_OK, or the PinnStatus the compute call would return for the descriptor. */
typedef struct PinnKernelInfo {
  int32_t engine;            /* 0 layer-major, 1 fused tile-major */
  int32_t time_order, space_order, act_family, backward;  /* act_family: PinnAct of the compiled unit (leaky_relu and
                                                             identity run the relu unit) */
  int32_t hmax, na0;         /* compiled variant: LDS image height (64 | 128), k-tiles of the first MFMA layer's
                                weight-gradient accumulators (2 | 4) */
  int32_t grid;              /* workgroups of the launch */
  int32_t flush;             /* weight gradients / loss sum: 0 direct atomics, 1 store flush, 2 two-level atomic flush,
                                3 deterministic slab */
  int32_t default_mfma_form; /* this unit was built in the fallback (default) MFMA form, see pinn_build_info() */
} PinnKernelInfo;
int pinn_kernel_for(const PinnNetDesc* net, int64_t N, int32_t time_order, int32_t space_order, int32_t backward,
                    PinnKernelInfo* out);
/* Name of the kernel such a call takes, written NUL-terminated into buf (at most len bytes): "jet_kernel_u16" (fused
 * tile-major, 16-point units, reverse launches), "jet_kernel_wide" (fused tile-major, 32-point tiles) or "layer_major".
 * PINN_OK, or the PinnStatus pinn_kernel_for returns for the same arguments. */
int pinn_kernel_name(const PinnNetDesc* net, int64_t N, int32_t time_order, int32_t space_order, int32_t backward,
                     char* buf, size_t len);

/* Launch plan of the layer-major engine for the call pinn_kernel_for describes — from the functions the engine launches
 * from (fusion plan, features per thread, AUX choice of the fused kernels, LDS-DMA predicate of the LayerNorm adjoint),
 * under the policy this process read from its environment.  The engine is planned whether or not the call would take it
 * (what PINN_FLAG_LAYER_MAJOR selects; pinn_kernel_for says which engine runs).  Record m < n describes GEMM node m and
 * its prologue ([LayerNorm] [+ skip record] [activation] of the node's input); record n is the head: the prologue of the
 * output layer, and lm_head.  A prologue runs forward either in the epilogue of the GEMM before it (lm_fused forward of
 * node m - 1) or as an element-wise launch of its own; its adjoint runs in the epilogue of its own node's reverse GEMM
 * (lm_fused reverse of node m) or as an element-wise launch.  `backward` = 0: the reverse fields are -1 / 0.
 * Returns n (the number of GEMM nodes; n + 1 records are written, at most PINN_LM_MAX_PLAN), or a negative PinnStatus. */
#define PINN_LM_MAX_PLAN 41
typedef struct PinnLmNodePlan {
  int32_t rows, depth;    /* the node's GEMM: padded out- and in-features (head: 1, padded width) */
  int32_t width;          /* padded features of the prologue (= depth) */
  int32_t has_ln, has_skip, has_add;  /* prologue: LayerNorm, skip record; node: epilogue add record */
  int32_t act_family;     /* compiled family of the prologue: PinnAct 0..4 (leaky_relu, identity and "no activation" run
                             relu's), -1 for Fourier features and for an identity prologue (no launch) */
  int32_t src_kind;       /* 0 record, 1 first Linear of the coordinates, 2 Fourier features of the coordinates */
  /* forward: how the prologue is computed */
  int32_t fwd_fused;      /* 1: by lm_fused<nch, rt, .., LN, forward, aux> of the node before, on gy row blocks */
  int32_t fwd_nch, fwd_rt, fwd_gy, fwd_aux;  /* -1 unless fwd_fused */
  int32_t fwd_ew_kind;    /* 0 lm_ew_fwd, 2 lm_fourier_fwd, -1 none (fused, or an identity prologue) */
  int32_t fwd_fpt;        /* features per thread of that launch, -1 if none */
  /* reverse: how the prologue's adjoint is computed */
  int32_t bwd_fused;      /* 1: by lm_fused<nch, rt, .., LN, reverse, aux> of this node */
  int32_t bwd_nch, bwd_rt, bwd_gy, bwd_aux;
  int32_t bwd_ew_kind;    /* 0 lm_ew_bwd, 1 lm_ew_bwd_dma, 2 lm_fourier_bwd (backward = 2 only), -1 none */
  int32_t bwd_fpt;
  int32_t head_fpt;       /* head record: features per thread of lm_head; -1 elsewhere */
} PinnLmNodePlan;
int pinn_lm_plan(const PinnNetDesc* net, int64_t N, int32_t time_order, int32_t space_order, int32_t backward,
                 PinnLmNodePlan* out, int32_t max_records);

/* How jet_kernel_u16 deals N points to `grid` workgroups (the grid of pinn_kernel_for).  rounds = R = N / (16 grid):
 * workgroup b runs the 16-point units b, b + grid, ... of R full rounds.  The points from first_tail_point = 16 grid R on
 * are the last round, groups = G = ceil((N - first_tail_point) / (4 grid)) four-point groups per workgroup:
 *   G = 0      nothing is left;
 *   G = 1..3   one packed round (4 points x 4 streams per 16-column MFMA operand group): workgroup b takes the points
 *              first_tail_point + 4 G b .. + 4 G - 1 that lie below N, so the round costs G quarters of a unit's MFMAs and
 *              all workgroups run it;
 *   G = 4      ordinary units first_tail_point / 16 + b.
 * A unit that was built without the packed round (pinn_build_info(): "nopack ...") runs every G > 0 as G = 4.
 * Outputs are nullable.  PINN_OK, or PINN_ERR_BAD_DESC for N < 0 or grid < 1. */
int pinn_unit_tail_plan(int64_t N, int32_t grid, int64_t* rounds, int32_t* groups, int64_t* first_tail_point);

/* Every compute entry point: `weights` (and `weight_grads`) are tables of `num_tensors` device pointers in the
 * reference's state_dict order; the count is validated against the descriptor BEFORE any entry is read.
 * `workspace` must hold pinn_workspace_bytes(...) bytes, 16-byte aligned (may be NULL when that is 0).
 * Weight tensors: contiguous fp32, hidden-layer weight matrices 16-byte aligned where the descriptor takes the fused
 * tile-major kernel (plain MLP family, widths multiples of 32 up to 128: it reads them in place with 16-byte loads) —
 * a misaligned view there is refused with PINN_ERR_MISALIGNED rather than silently re-routed to the engine
 * pinn_workspace_bytes did not size for; PINN_FLAG_LAYER_MAJOR selects the packing engine, which takes any alignment.
 *
 * Components of a multi-output network.  A descriptor always ends in width 1 (another last width is PINN_ERR_UNSUPPORTED):
 * one launch computes one output.  Output k of a network whose last Linear has C rows (W_out: C x H, b_out: C) is exactly
 * the one-output network whose output layer is row k of W_out and entry k of b_out, so a component launch is the width-1
 * descriptor with the two output-layer entries of `weights` pointing at W_out + k H and b_out + k, and — in a reverse
 * launch — the same two entries of `weight_grads` pointing at row k of the gradients (H floats and 1 float are accumulated;
 * the other rows are not touched).  Every other entry is the network's own; the trunk is recomputed per component.  Row k
 * of a width such as 30 is only 4-byte aligned: PINN_FLAG_LAYER_MAJOR is required whenever row k is not 16-byte aligned
 * (the layer-major engine reads the output layer through its packing pass, at any alignment).  Composes with
 * PINN_FLAG_SPACE_AXIS and PINN_FLAG_SPACE_DIRECTION. */

/* jets_out[s] : N floats each, stream order [u, d/dt.., d/dx..]; all K = 1+nt+nx entries required. */
int pinn_jet_forward(const PinnNetDesc* net, const float* const* weights, int32_t num_tensors, const float* x,
                     const float* t, int64_t N, int32_t time_order, int32_t space_order, float* const* jets_out,
                     void* workspace, size_t ws_bytes, void* stream);

/* Recomputes the forward, then accumulates
 * d(sum_s sum_n jet_cotangents[s][n] * jet_s[n]) / d(weights) into weight_grads (+=). */
int pinn_jet_backward(const PinnNetDesc* net, const float* const* weights, int32_t num_tensors, const float* x,
                      const float* t, int64_t N, int32_t time_order, int32_t space_order,
                      const float* const* jet_cotangents, float* const* weight_grads, void* workspace, size_t ws_bytes,
                      void* stream);

/* The reverse sweep of pinn_jet_backward on the layer-major engine, whatever the descriptor's flags say (the descriptor is
 * not modified; size the workspace with pinn_workspace_bytes(..., backward = 2)):
 * weight_grads += d<c, J>/d(weights) (table may be NULL: input cotangents only, and no weight-gradient work is done);
 * x_grad[n*dim + c] = sum_s c_s[n] dJ_s[n]/dx[n,c]  (N x dim, row-major, overwritten, nullable);
 * t_grad[n]         = sum_s c_s[n] dJ_s[n]/dt[n]    (N, overwritten, nullable).
 * dim = input_dim - 1.  Mixed terms (e.g. d(u_t)/dx) and every spatial column are exact.  x_grad / t_grad are reduced over
 * the features in a fixed order: bit-identical across launches on the same inputs, with or without
 * PINN_FLAG_DETERMINISTIC.  Validation and error codes as pinn_jet_backward. */
int pinn_jet_backward_inputs(const PinnNetDesc* net, const float* const* weights, int32_t num_tensors, const float* x,
                             const float* t, int64_t N, int32_t time_order, int32_t space_order,
                             const float* const* jet_cotangents, float* const* weight_grads,
                             float* x_grad, float* t_grad, void* workspace, size_t ws_bytes, void* stream);

/* residual_out: N floats or NULL.  loss_sum_out: 1 float or NULL; receives += sum_n l(r_n)
 * (l = r^2 | |r| | huber), i.e. the UNnormalised loss — the caller divides by the global N. */
int pinn_residual_forward(const PinnNetDesc* net, const float* const* weights, int32_t num_tensors,
                          const PinnPdeDesc* pde, const float* x, const float* t, int64_t N, float* residual_out,
                          float* loss_sum_out, void* workspace, size_t ws_bytes, void* stream);

/* One call: residual, loss sum, and weight_grads += grad_scale * d(sum_n l(r_n))/d(weights).
 * For mean-squared loss over N_total points use grad_scale = upstream / N_total. */
int pinn_residual_loss_grad(const PinnNetDesc* net, const float* const* weights, int32_t num_tensors,
                            const PinnPdeDesc* pde, const float* x, const float* t, int64_t N, float grad_scale,
                            float* residual_out, float* loss_sum_out, float* const* weight_grads, void* workspace,
                            size_t ws_bytes, void* stream);

/* The same with trainable PDE coefficients (inverse problems, pinnrl/pdes/pde_base.py:246-279: get_parameter returns a live
 * nn.Parameter that sits inside the residual): additionally coef_grads[k] += grad_scale * d(sum_n l(r_n))/d(pde->coef[k])
 * for k = 0, 1 (device pointer to >= 2 floats, nullable = pinn_residual_loss_grad; coefficients 2 and 3 are unused by the nine
 * PDEs).  One extra per-point reduction in the residual epilogue of the layer-major engine's head kernel; no second pass.
 * Descriptors that would take the fused tile-major kernel must carry PINN_FLAG_LAYER_MAJOR for such a call (and for the
 * pinn_workspace_bytes query that sizes its workspace): PINN_ERR_UNSUPPORTED otherwise. */
int pinn_residual_loss_grad_coef(const PinnNetDesc* net, const float* const* weights, int32_t num_tensors,
                                 const PinnPdeDesc* pde, const float* x, const float* t, int64_t N, float grad_scale,
                                 float* residual_out, float* loss_sum_out, float* const* weight_grads, float* coef_grads,
                                 void* workspace, size_t ws_bytes, void* stream);

/* Inverse problems on the fused kernels: pinn_residual_loss_grad with the four PDE coefficients read at LAUNCH time from
 * `coef_values` (device pointer to 4 floats, owned by the caller; pde->coef is ignored), so that a call captured in a HIP
 * graph follows whatever the optimiser writes there, and coef_grads[k] += grad_scale * d(sum_n l(r_n))/d(c_k), k = 0, 1
 * (device pointer to >= 2 floats, nullable), from the same launch.  Descriptors of the plain-MLP family take the fused
 * tile-major kernels (their COEF units: jet_kernel_u16 / jet_kernel_wide, chosen as pinn_residual_loss_grad chooses
 * them); a stream set without such a unit (KdV's (1,3), the (1,0) of >= 2-D descriptors) and every other descriptor take
 * the layer-major engine.  Null coef_values: PINN_ERR_BAD_DESC.  Size the workspace with pinn_inverse_workspace_bytes;
 * for descriptors that take a tile-major unit it equals pinn_workspace_bytes(net, N, nt, nx, 1). */
int pinn_residual_loss_grad_inverse(const PinnNetDesc* net, const float* const* weights, int32_t num_tensors,
                                    const PinnPdeDesc* pde, const float* coef_values, const float* x, const float* t,
                                    int64_t N, float grad_scale, float* residual_out, float* loss_sum_out,
                                    float* const* weight_grads, float* coef_grads, void* workspace, size_t ws_bytes,
                                    void* stream);
size_t pinn_inverse_workspace_bytes(const PinnNetDesc* net, const PinnPdeDesc* pde, int64_t N);
/* "jet_kernel_u16" | "jet_kernel_wide" | "layer_major": the kernel such a call takes (as pinn_kernel_name). */
int pinn_inverse_kernel_name(const PinnNetDesc* net, const PinnPdeDesc* pde, int64_t N, char* buf, size_t len);
/* The translation unit family of the kernel that the residual-mode calls of (net, pde) take on N points; forward-only,
 * fused, residual-adjoint and inverse calls of a descriptor are routed together, so one answer holds for all of them:
 * "jet_u16mf_<family>" (merged stream set, the default network's shape compiled in; the inverse call takes its
 * jet_u16mfc_ sibling), "jet_u16m_<family>" (merged stream set, shape read from the descriptor; jet_u16mc_),
 * "jet_u16_<nt>_<nx>_<family>" (one stream per derivative; jet_u16c_), or "jet_kernel_wide" / "layer_major" as
 * pinn_kernel_name answers for the reverse launch.  A query: nothing is launched and no device is needed. */
int pinn_residual_unit_name(const PinnNetDesc* net, const PinnPdeDesc* pde, int64_t N, char* buf, size_t len);

/* weight_grads += d(sum_n residual_cotangent[n] * r_n)/d(weights): the backward of pinn_residual_forward for an
 * arbitrary downstream graph (loss.backward() through `residual`, trainer.py:689; LRW's per-component
 * backward passes, trainer.py:607-626). */
int pinn_residual_backward(const PinnNetDesc* net, const float* const* weights, int32_t num_tensors,
                           const PinnPdeDesc* pde, const float* x, const float* t, int64_t N,
                           const float* residual_cotangent, float* const* weight_grads, void* workspace,
                           size_t ws_bytes, void* stream);

/* ---- training step (pinnrl/training/trainer.py:686-698, pinnrl/pdes/pde_base.py:1101-1165) -------------------------
 * With these entry points a whole optimiser step is a handful of launches with no autograd in it (and can be
 * captured in a HIP graph): pinn_residual_loss_grad for the residual term, pinn_jet_forward / pinn_jet_backward
 * (orders 0, 0) for the network values on the boundary / initial points, pinn_point_losses for their loss terms,
 * pinn_adam_clip_step for clip_grad_norm_ + Adam — or, with adaptive loss weights, pinn_adaptive_adam_step.
 * With L-BFGS (optimizer "lbfgs" / "adam_lbfgs") the same list WITHOUT its optimiser tail is one closure evaluation
 * (loss and flat gradient), followed by pinn_lbfgs_eval_stats; pinn_lbfgs_direction is the direction update between two
 * line searches (section "L-BFGS" below). */
#define PINN_MAX_POINT_TERMS 8

/* Term k (k < n_terms) covers points [lo[k], hi[k]) of u and has its own target array of hi[k] - lo[k] floats:
 * term_losses[k] = mean l(u - target_k) with l = PinnLoss `loss` (pde_base.py:309-326), and
 * cotangent[n] = sum_k weights[k] * l'(u[n] - target_k[n]) / (hi[k] - lo[k])  (n_total floats, overwritten).
 * An empty term (lo[k] == hi[k]) is allowed: term_losses[k] = 0 and it adds no cotangent (torch's mean over nothing
 * would be NaN); its target must still be non-null.  n_terms = 0 is allowed too: the cotangent is all zero.
 * Only term_losses[0 .. n_terms) is written.
 * lo / hi / targets / weights are HOST arrays (read before the call returns); u, targets[k], outputs: device.
 * summary4 (nullable, device): {residual, boundary, initial, total} of compute_loss — residual = residual_sum[0] *
 * residual_scale (the residual launch's loss sum / N), boundary = sum of the first n_boundary_terms term losses,
 * initial = the rest, total = residual_weight * residual + sum_k weights[k] * term_losses[k]. */
int pinn_point_losses(const float* u, int32_t n_total, int32_t n_terms, const int32_t* lo, const int32_t* hi,
                      const float* const* targets, const float* weights, int32_t loss, float huber_delta,
                      float* term_losses, float* cotangent, const float* residual_sum, float residual_scale,
                      float residual_weight, int32_t n_boundary_terms, float* summary4, void* stream);

/* The general form of pinn_point_losses, for PDEs whose compute_loss reads more than the value stream on its boundary
 * points (HeatEquation.compute_loss, pinnrl/pdes/heat_equation.py:375-623: periodic boundary conditions on u AND du/dx at
 * paired wall points): jets is the (n_streams x n_total) output of pinn_jet_forward; term k reads stream stream_of[k] and is
 * either  l(J[n] - targets[k][n - lo[k]])  or — pair_offset[k] != 0, targets[k] may be null —  l(J[n] - J[n + pair_offset[k]])
 * for n in [lo[k], hi[k]) (the partner range must not overlap it).  cotangent: (n_streams x n_total), overwritten: the
 * jet_cotangents of pinn_jet_backward.  Everything else as pinn_point_losses. */
int pinn_jet_losses(const float* jets, int32_t n_streams, int32_t n_total, int32_t n_terms, const int32_t* lo, const int32_t* hi,
                    const int32_t* stream_of, const int32_t* pair_offset, const float* const* targets, const float* weights,
                    int32_t loss, float huber_delta, float* term_losses, float* cotangent, const float* residual_sum,
                    float residual_scale, float residual_weight, int32_t n_boundary_terms, float* summary4, void* stream);

/* The finite-difference smoothness term of HeatEquation.compute_loss (pinnrl/pdes/heat_equation.py:625-650), 1-D:
 *   S = mean|(u(x+e,t) - u(x,t))/e| + mean|(u(x,t) - u(x-e,t))/e|  over the N collocation points, shifted points clamped
 * to [x_lo, x_hi].  Two entry points around a pinn_jet_forward / pinn_jet_backward pair (orders 0, 0) on 3N points.
 *
 * pinn_fd_stencil_points: x3 = [x | clamp(x + e, x_lo, x_hi) | clamp(x - e, x_lo, x_hi)], t3 = [t | t | t], 3N floats each,
 * the segments at offsets 0, N, 2N.  e = (float)eps, the bounds are rounded to float, x + e is one fp32 add: bit-equal to
 * torch.clamp(x + eps, x_lo, x_hi) on fp32 tensors.  16-byte accesses on every segment whose base is 16-byte aligned,
 * scalar accesses on the others (N need not be a multiple of 4).  N < 0, eps <= 0, x_lo > x_hi, a null pointer with
 * N > 0: PINN_ERR_BAD_DESC before any launch.  N == 0: no-op.  One launch.
 *
 * pinn_fd_smoothness: u3 = the value stream on those points, [uc | up | um].  loss_out[0] = S, unweighted (fp32
 * differences, a true division per point, sums and means in double, rounded once);  cotangent3 (3N floats, overwritten) =
 * weight * dS/du3 = c * [sgn(uc - um) - sgn(up - uc) | sgn(up - uc) | -sgn(uc - um)], c = weight / (eps N), sgn(0) = 0 (a
 * point on a domain end has up == uc or um == uc exactly);  summary4 (nullable): summary4[3] += weight * S — call it
 * after the pinn_jet_losses call that wrote the summary.  scratch: PINN_FD_SCRATCH_DOUBLES doubles, 8-byte aligned.
 * N <= 0, eps <= 0, null u3 / loss_out / cotangent3 / scratch: PINN_ERR_BAD_DESC; misaligned scratch: PINN_ERR_MISALIGNED.
 * Two launches (a fixed grid of per-block partials and the cotangents, then their ordered sum); no atomics:
 * bit-identical across runs. */
#define PINN_FD_SCRATCH_DOUBLES 128
int pinn_fd_stencil_points(const float* x, const float* t, int64_t N, double eps, double x_lo, double x_hi, float* x3, float* t3,
                           void* stream);
int pinn_fd_smoothness(const float* u3, int64_t N, double eps, float weight, float* loss_out, float* cotangent3, float* summary4,
                       double* scratch, void* stream);

/* ---- causal residual weights (no counterpart in pinnrl; Wang, Sankaran, Perdikaris 2022, "Respecting causality is all
 * you need for training physics-informed neural networks") -----------------------------------------------------------
 * The residual loss of late times is held back until the loss of earlier times is small.  The time domain [t_lo, t_hi] is
 * cut into n_bins equal bins; the middle of the chain pinn_residual_forward -> pinn_causal_weights -> pinn_residual_backward.
 *   bin of a point    b(n) = (int) min(max((t_n - (float)t_lo) * s, 0), n_bins - 1), s = (float)(n_bins / (t_hi - t_lo)) with the
 *                     quotient in double; the subtraction and the product are one rounded fp32 operation each (no FMA):
 *                     bit-equal to torch's ((t - lo) * s).clamp(0, n_bins - 1).to(int32).  t_hi and beyond: the last bin;
 *                     below t_lo: bin 0.  t must be finite;
 *   bin statistics    S_i = sum_{b(n) = i} l(r_n), c_i = the count, L_i = S_i / c_i (0 for an empty bin), in double, l = PinnLoss
 *                     `loss` with l and l' as pinn_residual_loss_grad has them (sgn(0) = 0, Huber's quadratic branch on
 *                     |r| < delta);
 *   weights           w_i = (float) exp(-(double)eps_dev[0] * sum_{k < i} L_k), w_0 = 1: constants of the differentiation.
 *                     eps_dev is a DEVICE scalar (>= 0, finite) read at launch time — the `lr` convention of
 *                     pinn_adam_clip_step — so a captured graph follows a schedule of the sharpness;
 *   cotangent         N floats, overwritten: cotangent[n] = grad_scale * w_b(n) * l'(r_n), fp32, the product taken as
 *                     (grad_scale * w) * l' — the residual_cotangent of pinn_residual_backward;
 *   loss_sum_out      nullable: loss_sum_out[0] += sum_i w_i S_i, the UNnormalised, count-weighted loss (the convention of
 *                     pinn_residual_loss_grad: the caller divides by N).  With eps = 0 every weight is exactly 1 and this is
 *                     the plain residual loss;
 *   plain_sum_out     nullable: plain_sum_out[0] += sum_i S_i;  both are double sums in bin order, rounded once;
 *   bin_losses        nullable, n_bins floats: L_i;   bin_weights: n_bins floats, REQUIRED (the third launch reads it);
 *   scratch           PINN_CAUSAL_SCRATCH_DOUBLES doubles, 8-byte aligned.
 * Three launches on `stream`, no synchronisation, no allocation, no atomics: a fixed grid of at most 64 blocks x 256 threads
 * writes per-block, per-bin partial sums and counts (inside a wave the lanes of one bin are summed by a fixed butterfly,
 * bin after bin; the four wave rows are added in wave order); one workgroup adds the partials in block order, takes the
 * serial prefix in double and writes the weights and the two sums (the only launch that reads eps_dev); the third writes
 * the cotangents, 16 bytes at a time where a buffer is 16-byte aligned and the quad is whole, scalar accesses otherwise.
 * Two calls on the same inputs are bit-identical, whatever the alignment of the buffers.
 * Checked on the host before any HIP call: n_bins outside [1, PINN_CAUSAL_MAX_BINS], t_hi <= t_lo or a non-finite bound, an
 * unknown loss, N < 0, null residual / t / eps_dev / cotangent / bin_weights / scratch with N > 0: PINN_ERR_BAD_DESC;
 * misaligned scratch: PINN_ERR_MISALIGNED.  N == 0: no-op. */
#define PINN_CAUSAL_MAX_BINS 64
#define PINN_CAUSAL_SCRATCH_DOUBLES (64 * 2 * PINN_CAUSAL_MAX_BINS) /* 64 blocks x (sum, count) x 64 bins; the finish pass works in LDS */
int pinn_causal_weights(const float* residual, const float* t, int64_t N, int32_t n_bins, double t_lo, double t_hi,
                        const float* eps_dev, int32_t loss, float huber_delta, float grad_scale, float* cotangent,
                        float* loss_sum_out, float* plain_sum_out, float* bin_losses, float* bin_weights, double* scratch,
                        void* stream);

/* ---- face loss terms: Dirichlet, Neumann, Robin and periodic conditions per face (no counterpart in pinnrl) ----------
 * A superset of pinn_jet_losses for up to PINN_FACE_MAX_TERMS terms, on a grid instead of one workgroup.  The jets of ALL
 * launches of a boundary / initial chain lie in ONE buffer of n_floats floats (pinn_jet_forward writes its rows straight
 * into it), the cotangents in a second buffer of the same layout (row s of a launch is the jet_cotangents[s] of its
 * pinn_jet_backward).  Term k names up to four segments of n floats by their offsets in floats, -1 meaning absent:
 *   value, value_pair   A, A'   a value row segment and its optional partner (periodic pairs),
 *   deriv, deriv_pair   B, B'   a derivative row segment and its optional partner,
 * and  d_i = alpha (A[i] - A'[i]) + beta (B[i] - B'[i]) - T_i  for i < n,  T_i = target[i], or target_const when target is
 * null.  A missing segment contributes nothing.  fp32 evaluation order, every operation rounded once, none contracted:
 *   d = -T_i;   a = A[i], then a = a - A'[i] with a partner;   d = fma(alpha, a, d)   (with a value segment);
 *   b = B[i], then b = b - B'[i] with a partner;   d = fma(beta, b, d)   (with a derivative segment).
 * Outputs:
 *   term_losses[k] = (1/n) sum_i l(d_i): l in double from the fp32 d_i (l as pinn_causal_weights has it), double sums, the
 *                    mean rounded once;
 *   cotangent       with s = weight / (float)n, sa = s * alpha, sb = s * beta (fp32, in this order) and l' exact in fp32:
 *                    sa l'(d_i) on A, its negation on A', sb l'(d_i) on B, its negation on B'.  Every float a term names is
 *                    written exactly once; every other float of the buffer is left untouched (the caller zeroes it once:
 *                    the rows no term names, such as u_t of a (1, 1) launch, then stay zero without a fill per step);
 *   summary4        nullable: {residual, boundary, initial, total} as pinn_jet_losses defines them (residual = residual_sum[0]
 *                    * residual_scale in fp32; the three sums over the rounded term losses in double, term order, rounded
 *                    once).  n_terms == 0 with a summary still writes it.
 * terms is a HOST array, read before the call returns and handed to the kernels by value (no upload, no copy of jets);
 * jets, cotangent, target, term_losses, residual_sum, summary4, scratch: device.  scratch: PINN_FACE_SCRATCH_DOUBLES
 * doubles, 8-byte aligned.
 * Two launches on `stream`, no synchronisation, no allocation, no atomics: a fixed grid of min(64, ceil(max n / 256))
 * blocks x 256 threads (the term loop is wave-uniform; block b takes the points b * 256 + tid, + grid * 256, ... of every
 * term; 4-byte accesses, so which thread takes which point does not depend on alignment; per-block, per-term partial sums
 * in double: a fixed butterfly inside a wave, the four waves in order); one workgroup adds the partials in block order.
 * Two calls on the same inputs are bit-identical, and so are the term losses of the same data at other offsets.
 * Checked on the host before any launch, PINN_ERR_BAD_DESC: n_terms outside [0, PINN_FACE_MAX_TERMS]; an unknown loss;
 * n < 1; an offset other than -1 whose segment leaves [0, n_floats); alpha != 0 without a value segment or a value segment
 * with alpha == 0, and the same for beta and the derivative segment; a partner without its primary; any two segments that
 * overlap, of different terms or of one; with n_terms > 0 a null jets / cotangent / terms / term_losses / scratch.
 * Misaligned scratch: PINN_ERR_MISALIGNED. */
#define PINN_FACE_MAX_TERMS 32
#define PINN_FACE_SCRATCH_DOUBLES (64 * PINN_FACE_MAX_TERMS) /* 64 blocks x 32 terms */
typedef struct PinnFaceTerm {
  int32_t value, value_pair, deriv, deriv_pair; /* offsets in floats into jets / cotangent, -1: absent */
  int32_t n;                                    /* points of the term */
  float alpha, beta, target_const, weight;
  const float* target; /* n device floats, or null: target_const */
} PinnFaceTerm;
int pinn_face_losses(const float* jets, float* cotangent, int64_t n_floats, int32_t n_terms, const PinnFaceTerm* terms,
                     int32_t loss, float huber_delta, float* term_losses, const float* residual_sum, float residual_scale,
                     float residual_weight, int32_t n_boundary_terms, float* summary4, double* scratch, void* stream);

/* ---- residuals given as data (pinnrl: a user's PDEBase subclass, pinnrl/pdes/pde_base.py:574-588) ---------------------
 * A residual outside the nine compiled PDEs, as a sum of products of streams, coordinates and sin / cos of the value:
 *   r = sum_{m < n_terms} c_m prod_{f < n_factors[m]} phi_{m,f}
 * Each factor is one PinnTermFactor code, whatever the stream set; a repeated code is a power (u^3 = U, U, U); a term
 * without factors is a constant source.  The coefficients c_m are NOT in the descriptor: they are n_terms device floats
 * read at launch time (the `coef_values` convention of pinn_residual_loss_grad_inverse), so a captured graph follows a
 * coefficient that changes.
 *
 * pinn_term_residual is the element-wise middle of the chain pinn_jet_forward -> pinn_term_residual -> pinn_jet_backward:
 *   jets               K x N, K = 1 + time_order + space_order, stream s at jets + s N (what pinn_jet_forward writes into
 *                      K consecutive rows); x, t: N floats each (1-D problems), read only when a term names X / T;
 *   residual_out       N floats, nullable;
 *   loss_sum_out       nullable: loss_sum_out[0] += sum_n l(r_n), l = PinnLoss `loss` (as pinn_residual_loss_grad);
 *   jet_cotangents     K x N, nullable, overwritten with rbar_n dr_n/djet_s[n] — the jet_cotangents of pinn_jet_backward;
 *                      rbar_n = grad_scale l'(r_n) (sgn(0) = 0 for the absolute value, Huber's quadratic branch on
 *                      |r| < delta), or residual_cotangent[n] when that array (N floats, nullable) is given: the backward of
 *                      a residual tensor in an arbitrary downstream graph;
 *   coef_grads         nullable: coef_grads[m] += sum_n rbar_n prod_f phi_{m,f}, m < n_terms;
 *   scratch            PINN_TERM_SCRATCH_DOUBLES doubles, 8-byte aligned; may be NULL when neither loss_sum_out nor
 *                      coef_grads is given.
 * 256-thread blocks on a fixed grid of at most 64, one point per thread with its K streams in registers, the term list in
 * the kernel arguments.  The loss and coefficient sums are per-block partials in double that a second launch adds in block
 * order: no atomics, bit-identical across runs.  Without loss_sum_out and coef_grads the call is ONE launch.
 * Checked on the host before any HIP call: n_terms outside [0, PINN_TERM_MAX_TERMS], n_factors outside
 * [0, PINN_TERM_MAX_FACTORS], an unknown factor code, a factor naming a stream that (time_order, space_order) does not
 * hold, a stream set without a compiled unit, N < 0, null jets / coef_values (or x / t under an X / T factor, or scratch
 * where it is needed) with N > 0: PINN_ERR_BAD_DESC; misaligned scratch: PINN_ERR_MISALIGNED.  N == 0: no-op. */
#define PINN_TERM_MAX_TERMS 16
#define PINN_TERM_MAX_FACTORS 4
#define PINN_TERM_SCRATCH_DOUBLES (64 * (1 + PINN_TERM_MAX_TERMS))

typedef enum PinnTermFactor {
  PINN_TERM_U = 0,
  PINN_TERM_UT = 1,
  PINN_TERM_UTT = 2,
  PINN_TERM_UX = 3,
  PINN_TERM_UXX = 4,
  PINN_TERM_UXXX = 5,
  PINN_TERM_UXXXX = 6,
  PINN_TERM_X = 7,
  PINN_TERM_T = 8,
  PINN_TERM_SIN_U = 9,
  PINN_TERM_COS_U = 10
} PinnTermFactor;

typedef struct PinnTermPdeTerm {
  int32_t n_factors;                     /* 0 .. PINN_TERM_MAX_FACTORS */
  int32_t factor[PINN_TERM_MAX_FACTORS]; /* PinnTermFactor */
} PinnTermPdeTerm;

typedef struct PinnTermPde {
  int32_t time_order, space_order; /* the stream set of `jets`: one the library has a unit for */
  int32_t n_terms;                 /* 0 .. PINN_TERM_MAX_TERMS */
  int32_t loss;                    /* PinnLoss */
  float huber_delta;
  PinnTermPdeTerm terms[PINN_TERM_MAX_TERMS];
} PinnTermPde;

int pinn_term_residual(const PinnTermPde* pde, const float* coef_values, const float* jets, const float* x, const float* t,
                       int64_t N, float grad_scale, const float* residual_cotangent, float* residual_out, float* loss_sum_out,
                       float* jet_cotangents, float* coef_grads, double* scratch, void* stream);

/* ---- term residuals along every space axis (no counterpart in pinnrl: there every spatial derivative of a >= 2-D problem
 * is zero) -------------------------------------------------------------------------------------------------
 * The multi-axis form of pinn_term_residual for 2 or 3 space dimensions: a Laplacian, advection along y, ...  A pure
 * derivative along axis a is the jet recursion seeded from column a (PINN_FLAG_SPACE_AXIS), so the chain is
 *   pinn_jet_forward (axis 0, set (time_order, space_order[0])) and, for every axis a >= 1 with space_order[a] > 0, one more
 *   pinn_jet_forward (axis a, set (0, space_order[a]))  ->  pinn_term_residual_axes  ->  one pinn_jet_backward per launch,
 * all of them accumulating into the same weight gradients.  Mixed derivatives (u_xy) are not available here:
 * pinn_term_residual_mixed below has them.
 * Factor codes: 0 .. 10 keep their meaning (PinnTermFactor; U_X .. U_XXXX and X refer to axis 0), then PINN_TERM_UY ..
 * PINN_TERM_Z below.  Axis 0 takes any compiled set; the axes 1 and 2 take order 0, 1 or 2.
 *   jets               HOST table of `dimension` device pointers: jets[0] the (1 + time_order + space_order[0]) x N block of
 *                      the axis-0 launch, jets[a] (a >= 1) the (1 + space_order[a]) x N block [u, d/dx_a, d2/dx_a2] of the
 *                      axis-a launch (its row 0 is not read), NULL when space_order[a] is 0;
 *   x                  N x dimension, row-major; t: N floats; each read only when a term names X / Y / Z or T;
 *   jet_cotangents     nullable HOST table of blocks with the shapes of `jets`, overwritten.  The whole cotangent of u,
 *                      sin(u) and cos(u) goes to row 0 of block 0; row 0 of every other block is written as zeros, so each
 *                      block goes straight into pinn_jet_backward;
 *   coefficients, residual_out, loss_sum_out, coef_grads, residual_cotangent, grad_scale, scratch
 *                      (PINN_TERM_SCRATCH_DOUBLES), launches, grid and determinism: as pinn_term_residual.
 * Checked on the host before any HIP call: dimension outside {2, 3}, n_terms or n_factors out of range, an uncompiled
 * axis-0 set, space_order[a] outside [0, 2] for a >= 1 (or non-zero for a >= dimension), an unknown factor code, a factor
 * naming a stream or coordinate the descriptor does not hold, N < 0, a null jets table / coef_values / required block of
 * either table (or x / t under a coordinate factor, or scratch where it is needed) with N > 0: PINN_ERR_BAD_DESC;
 * misaligned scratch: PINN_ERR_MISALIGNED.  N == 0: no-op. */
#define PINN_TERM_UY 11
#define PINN_TERM_UYY 12
#define PINN_TERM_UZ 13
#define PINN_TERM_UZZ 14
#define PINN_TERM_Y 15
#define PINN_TERM_Z 16

typedef struct PinnTermPdeAxes {
  int32_t dimension;      /* 2 or 3 */
  int32_t time_order;     /* (time_order, space_order[0]): the stream set of jets[0] */
  int32_t space_order[3]; /* per axis; [1], [2]: 0 .. 2, 0 beyond `dimension` */
  int32_t n_terms;        /* 0 .. PINN_TERM_MAX_TERMS */
  int32_t loss;           /* PinnLoss */
  float huber_delta;
  PinnTermPdeTerm terms[PINN_TERM_MAX_TERMS];
} PinnTermPdeAxes;

int pinn_term_residual_axes(const PinnTermPdeAxes* pde, const float* coef_values, const float* const* jets, const float* x,
                            const float* t, int64_t N, float grad_scale, const float* residual_cotangent, float* residual_out,
                            float* loss_sum_out, float* const* jet_cotangents, float* coef_grads, double* scratch, void* stream);

/* ---- term residuals with mixed derivatives (u_xy, u_xxyy) -----------------------------------------------------------------
 * pinn_term_residual_axes plus the orders 3 and 4 along y and z and the mixed factors u_ab, u_aabb of every pair of axes.
 * A mixed derivative is a fixed linear combination of pure derivatives along a few lines (polarisation): with
 * P_k = (d_a + d_b)^k u and Q_k = (d_a - d_b)^k u, the streams of the jet launches along e_a + e_b and e_a - e_b
 * (PINN_FLAG_SPACE_DIRECTION),
 *   u_ab   = 0.5f * ((P_2 - A_2) - B_2)
 *   u_aabb = ((P_4 + Q_4) - 2.0f * (A_4 + B_4)) * (float)(1.0 / 12.0)
 * evaluated in fp32 in exactly this order; A_k, B_k are the order-k rows of the two axis blocks (axis 0: row time_order + k).
 * The chain is one pinn_jet_forward per block -> pinn_term_residual_mixed -> one pinn_jet_backward per block.
 *   jets, jet_cotangents   HOST tables of 9 device pointers [axis0, axis1, axis2, P_xy, P_xz, P_yz, Q_xy, Q_xz, Q_yz]:
 *                      axis blocks as for pinn_term_residual_axes, (1 + space_order[a]) x N for a >= 1; P_ab the
 *                      (1 + pair_order) x N block of the launch along e_a + e_b, Q_ab the same along e_a - e_b, required
 *                      only when pair_order = 4; blocks that are not needed are NULL.  From a P / Q block only the rows 2
 *                      and 4 are read.
 *   cotangents         the transposes, added to whatever the pure factors put there: with g = rbar dr/du_ab, +g/2 to row 2 of
 *                      P_ab and -g/2 to the order-2 rows of both axis blocks; with h for u_aabb, +h/12 to row 4 of P_ab and of
 *                      Q_ab and -h/6 to both order-4 rows.  Every row of a cotangent block that the program never reads —
 *                      row 0 of every block >= 1 among them — is written as zeros, so each block goes straight into
 *                      pinn_jet_backward.
 * Factor codes 0 .. 16 keep their meaning; PINN_TERM_UYYY .. PINN_TERM_UYYZZ below.
 * Everything else — coefficients, residual_out, loss_sum_out, coef_grads, residual_cotangent, grad_scale, scratch
 * (PINN_TERM_SCRATCH_DOUBLES), the loss kinds, sgn(0) = 0, launches, grid and determinism — as pinn_term_residual_axes.
 * Checked on the host before any HIP call: what pinn_term_residual_axes checks (space_order[a] in [0, 4] for a >= 1), a
 * pair_order outside {0, 2, 4} or non-zero on a pair touching an axis >= dimension, u_ab without pair_order >= 2 and order >= 2
 * on both axes, u_aabb without pair_order = 4 and order 4 on both axes, a null required block: PINN_ERR_BAD_DESC.
 * Not available: mixed space-time derivatives, third-order mixed (u_xxy) and u_xxxy-type factors. */
#define PINN_TERM_UYYY 17
#define PINN_TERM_UYYYY 18
#define PINN_TERM_UZZZ 19
#define PINN_TERM_UZZZZ 20
#define PINN_TERM_UXY 21
#define PINN_TERM_UXZ 22
#define PINN_TERM_UYZ 23
#define PINN_TERM_UXXYY 24
#define PINN_TERM_UXXZZ 25
#define PINN_TERM_UYYZZ 26
#define PINN_TERM_MIXED_BLOCKS 9

typedef struct PinnTermPdeMixed {
  int32_t dimension;      /* 2 or 3 */
  int32_t time_order;     /* (time_order, space_order[0]): the stream set of jets[0] */
  int32_t space_order[3]; /* per axis; [1], [2]: 0 .. 4, 0 beyond `dimension` */
  int32_t pair_order[3];  /* pairs (x,y), (x,z), (y,z): 0, 2 or 4; 0 for a pair touching an axis >= dimension */
  int32_t n_terms;        /* 0 .. PINN_TERM_MAX_TERMS */
  int32_t loss;           /* PinnLoss */
  float huber_delta;
  PinnTermPdeTerm terms[PINN_TERM_MAX_TERMS];
} PinnTermPdeMixed;

int pinn_term_residual_mixed(const PinnTermPdeMixed* pde, const float* coef_values, const float* const* jets, const float* x,
                             const float* t, int64_t N, float grad_scale, const float* residual_cotangent, float* residual_out,
                             float* loss_sum_out, float* const* jet_cotangents, float* coef_grads, double* scratch, void* stream);

/* ---- term residuals of coupled systems (several unknowns, several equations) ----------------------------------------------
 * E residuals in C fields, the fields being the components of one C-output network (component launches, above):
 *   r_e = sum_{m: equation_of[m] = e} c_m prod_{f < n_factors[m]} phi_{m,f},   e < n_equations,
 * with one term list of at most PINN_SYSTEM_MAX_TERMS terms shared by all equations.  A factor is ONE BYTE,
 * PINN_SYSTEM_FACTOR(field, code) = field * 32 + code: `code` is a PinnTermFactor 0 .. 10 or PINN_TERM_UY .. PINN_TERM_Z
 * (11 .. 16) with its meaning for that field; coordinates ignore the field bits; no mixed derivatives
 * (pinn_term_residual_system_mixed below has u_xy, u_xz, u_yz of every field).  Dimension 1 to 3.
 * Per field c, (time_order[c], space_order[c][0]) is a compiled axis-0 set and the axes 1 and 2 take the orders 0 .. 2
 * (0 beyond `dimension`).  The chain is one pinn_jet_forward per (field, axis with streams) -> pinn_term_residual_system ->
 * one pinn_jet_backward per block, all accumulating into the same weight gradients.
 *   jets, jet_cotangents   HOST tables of 3 C device pointers, entry 3 c + a: block (c, 0) the
 *                      (1 + time_order[c] + space_order[c][0]) x N block of field c's axis-0 launch (always required), block
 *                      (c, a >= 1) the (1 + space_order[c][a]) x N block of its axis-a launch (row 0 is not read), NULL when
 *                      that order is 0.  jet_cotangents is nullable; its blocks are overwritten.  The whole cotangent of field
 *                      c's value, sin and cos goes to row 0 of block (c, 0); row 0 of every other block of the field and every
 *                      row the program never reads are written as zeros (a field no term names gets all-zero blocks), so each
 *                      block goes straight into pinn_jet_backward;
 *   x, t               N x dimension row-major, N floats; read only under a coordinate factor;
 *   coef_values        n_terms device floats c_m, read at launch time;
 *   residual_out       E x N (equation e at residual_out + e N), nullable;
 *   rbar_e,n           (grad_scale * eq_weight[e]) * l'(r_e,n), the product in parentheses rounded to fp32 once on the host,
 *                      or residual_cotangent[e N + n] when that array (E x N, nullable) is given; l, l' as pinn_term_residual
 *                      (sgn(0) = 0, Huber's quadratic branch on |r| < delta);
 *   loss_sum_out       nullable: loss_sum_out[0] += sum_e eq_weight[e] sum_n l(r_e,n);
 *   eq_loss_sums       nullable, E floats: eq_loss_sums[e] += sum_n l(r_e,n), unweighted;
 *   coef_grads         nullable: coef_grads[m] += sum_n rbar_{equation_of[m],n} prod_f phi_{m,f};
 *   scratch            PINN_SYSTEM_SCRATCH_DOUBLES doubles, 8-byte aligned; may be NULL when no sum is wanted.
 * Rounding order, per point, in fp32.  Sweep 1: the terms in ascending m, each product formed as ((c_m phi_0) phi_1) ... and
 * added to r_{equation_of[m]} (the order of pinn_term_residual_axes).  Then l, l' and rbar_e of every equation.  Sweep 2: the
 * terms in ascending m again; the derivative of term m with respect to factor f is (((c_m phi_g) ...) over g != f in ascending
 * g, times cos(u) under sin(u), or negated after the product with sin(u) under cos(u); the summands of ONE term that belong
 * to the same (field, stream) — at most four — are summed first in ascending f, that sum is multiplied by
 * rbar_{equation_of[m]}, and the product is added to the (field, stream) accumulator, which is what the cotangent row
 * receives.  The sums over the points are per-block partials in double (one point per thread per grid-stride round,
 * 256-thread blocks on a fixed grid of at most 64) that a second launch adds in block order; the weighted loss is formed
 * from the per-equation sums in double, in ascending e.  No atomics, bit-identical across runs; a call that produces no loss
 * or coefficient sum is ONE launch.
 * Checked on the host before any HIP call: dimension, n_fields, n_equations, n_terms or n_factors out of range, an
 * uncompiled axis-0 set, space_order[c][a] outside [0, 2] for a >= 1 (or non-zero for a >= dimension), equation_of[m] outside
 * [0, E), a negative or non-finite eq_weight, a factor that is not one byte, an unknown code, a field index >= C, a factor
 * naming a stream or coordinate the descriptor does not hold, N < 0, a null jets table / coef_values / required block of either
 * table (or x / t under a coordinate factor, or scratch where it is needed) with N > 0: PINN_ERR_BAD_DESC; misaligned
 * scratch: PINN_ERR_MISALIGNED.  N == 0: no-op. */
#define PINN_SYSTEM_MAX_FIELDS 4
#define PINN_SYSTEM_MAX_EQUATIONS 4
#define PINN_SYSTEM_MAX_TERMS 32
#define PINN_SYSTEM_SCRATCH_DOUBLES (64 * (4 + 32))
#define PINN_SYSTEM_FACTOR(field, code) ((field) * 32 + (code))

typedef struct PinnTermPdeSystem {
  int32_t dimension;                                   /* 1 .. 3 */
  int32_t n_fields;                                    /* C: 1 .. PINN_SYSTEM_MAX_FIELDS */
  int32_t n_equations;                                 /* E: 1 .. PINN_SYSTEM_MAX_EQUATIONS */
  int32_t time_order[PINN_SYSTEM_MAX_FIELDS];          /* per field; with space_order[c][0] the stream set of block (c, 0) */
  int32_t space_order[PINN_SYSTEM_MAX_FIELDS][3];      /* per field and axis; [c][1], [c][2]: 0 .. 2, 0 beyond `dimension` */
  int32_t n_terms;                                     /* 0 .. PINN_SYSTEM_MAX_TERMS, shared by all equations */
  int32_t equation_of[PINN_SYSTEM_MAX_TERMS];          /* the equation of term m */
  float eq_weight[PINN_SYSTEM_MAX_EQUATIONS];          /* omega_e >= 0, finite */
  int32_t loss;                                        /* PinnLoss */
  float huber_delta;
  PinnTermPdeTerm terms[PINN_SYSTEM_MAX_TERMS];        /* factor[f] = PINN_SYSTEM_FACTOR(field, code) */
} PinnTermPdeSystem;

int pinn_term_residual_system(const PinnTermPdeSystem* pde, const float* coef_values, const float* const* jets, const float* x,
                              const float* t, int64_t N, float grad_scale, const float* residual_cotangent, float* residual_out,
                              float* loss_sum_out, float* eq_loss_sums, float* const* jet_cotangents, float* coef_grads,
                              double* scratch, void* stream);

/* ---- term residuals of coupled systems with mixed derivatives (u_xy of any field) ------------------------------------------
 * pinn_term_residual_system plus the factors u_ab of every field: the grad-div term of linear elasticity,
 * mu Lap(u) + (lambda + mu) grad(div u), names v_xy in the u-equation and u_xy in the v-equation.  The factor byte stays
 * PINN_SYSTEM_FACTOR(field, code); the codes 0 .. 16 keep their meaning, PINN_TERM_UXY, PINN_TERM_UXZ and PINN_TERM_UYZ
 * (21 .. 23) are the mixed derivative of THAT field along the pair k = code - 21 of (x,y), (x,z), (y,z).  The codes 17 .. 20
 * (order > 2 along y / z) and 24 .. 26 (u_aabb) are refused by name.  pair_order[c][k] is 0 or 2 (0 for a pair that touches an
 * axis >= dimension); u_ab of field c needs pair_order[c][k] == 2 and order >= 2 of that field on both axes.
 *   jets, jet_cotangents   HOST tables of 6 C device pointers (PINN_SYSTEM_MIXED_BLOCKS(C)).  Entry 3 c + a is the axis block
 *                      (c, a) exactly as for pinn_term_residual_system.  Entry 3 C + 3 c + k is the 3 x N block of field c's
 *                      launch along e_a + e_b for pair k on the set (0, 2) — a component launch with
 *                      PINN_FLAG_SPACE_DIRECTION; only its row 2 (P_2) is read; NULL where pair_order[c][k] == 0.
 *   value              u_ab = 0.5f * ((P_2 - A_2) - B_2), evaluated in fp32 in exactly this order (pinn_term_residual_mixed's);
 *                      A_2, B_2 are the order-2 rows of the field's two axis blocks (axis 0: row time_order + 2).
 *   cotangents         u_ab of a field is a (field, stream) target of its own under the sweep-2 rule of
 *                      pinn_term_residual_system: the summands of one term that hit it are summed first, the sum is multiplied
 *                      by rbar_{equation_of[m]} and the product is added to the accumulator g_k.  At write-out, per field and
 *                      in ascending pair index k: p_k = 0.5f * g_k goes to row 2 of the P block, and the accumulator of the
 *                      order-2 row of axis a, then that of axis b, has p_k subtracted from it (an x row that two pairs touch
 *                      receives (acc - p_0) - p_1, the order of pinn_term_residual_mixed).  Rows 0 and 1 of every P cotangent
 *                      block are written as zeros, as is every row the program never reads, so each block goes straight into
 *                      pinn_jet_backward.
 * Everything else — residual_out (E x N), residual_cotangent, loss_sum_out, eq_loss_sums, coef_grads, grad_scale * eq_weight[e]
 * rounded once on the host, the loss kinds, sgn(0) = 0, scratch (PINN_SYSTEM_SCRATCH_DOUBLES), the rounding order of the pure
 * factors, per-block double partials added in block order by the finish launch, no atomics, one launch when no sum is wanted,
 * N == 0 a no-op — as pinn_term_residual_system: with every pair_order 0 the residuals and cotangent blocks are the same.
 * Checked on the host before any HIP call: every check of pinn_term_residual_system; a pair_order outside {0, 2} or non-zero
 * on a pair beyond the dimension (dimension 1 among them); a u_ab factor without pair_order[field][k] == 2 and order >= 2 on both
 * axes of that field; a null required P block in either table: PINN_ERR_BAD_DESC, the message naming the field and the pair. */
#define PINN_SYSTEM_MIXED_BLOCKS(C) (6 * (C))

typedef struct PinnTermPdeSystemMixed {
  int32_t dimension;                                   /* 1 .. 3 (a mixed factor needs 2 or 3) */
  int32_t n_fields;
  int32_t n_equations;
  int32_t time_order[PINN_SYSTEM_MAX_FIELDS];
  int32_t space_order[PINN_SYSTEM_MAX_FIELDS][3];
  int32_t n_terms;
  int32_t equation_of[PINN_SYSTEM_MAX_TERMS];
  float eq_weight[PINN_SYSTEM_MAX_EQUATIONS];
  int32_t loss;
  float huber_delta;
  PinnTermPdeTerm terms[PINN_SYSTEM_MAX_TERMS];        /* factor[f] = PINN_SYSTEM_FACTOR(field, code), code 0 .. 16 or 21 .. 23 */
  int32_t pair_order[PINN_SYSTEM_MAX_FIELDS][3];       /* per field, pairs (x,y), (x,z), (y,z): 0 or 2 */
} PinnTermPdeSystemMixed;

int pinn_term_residual_system_mixed(const PinnTermPdeSystemMixed* pde, const float* coef_values, const float* const* jets,
                                    const float* x, const float* t, int64_t N, float grad_scale, const float* residual_cotangent,
                                    float* residual_out, float* loss_sum_out, float* eq_loss_sums, float* const* jet_cotangents,
                                    float* coef_grads, double* scratch, void* stream);

/* ---- term residuals of coupled systems with known functions of (x, t) as factors -------------------------------------------
 * pinn_term_residual_system_mixed plus up to PINN_SYSTEM_MAX_FUNCTIONS factors g_k(x, t) that the caller has evaluated at the
 * points: a source term f(x, t), a coefficient that varies in space (kappa(x, y) u_xx), a given velocity field (a(x, y) c_x), a
 * body force.  r_e = sum_m c_m prod_f phi_{m,f} with phi a stream of a field, a coordinate, sin / cos of a field or g_k.  The
 * factor byte stays PINN_SYSTEM_FACTOR(field, code); every code of pinn_term_residual_system_mixed keeps its meaning and
 * PINN_TERM_FN0 .. PINN_TERM_FN3 (27 .. 30) name g_0 .. g_3; the field bits are ignored, as for coordinates.  Code 31 is unknown,
 * and the codes 17 .. 20 and 24 .. 26 stay refused by name.
 *   fn_values          n_functions x N device floats, function k at fn_values + k N, read at launch time.  A row that no term
 *                      names is never read (a host-made, wave-uniform mask); may be NULL when no term names a function.
 *   sweep 1            a function factor is a factor like PINN_TERM_X: it enters the product ((c_m phi_0) phi_1) ... at its position.
 *   sweep 2            a function factor contributes no derivative summand and is no cotangent target; it stays in the products
 *                      c_m prod_{g != f} phi_g of the other factors' derivatives and in coef_grads[m] = sum_n rbar prod_f phi_{m,f}.
 * Everything else — the 6 C block tables, u_ab and its cotangents, residual_out (E x N), residual_cotangent, loss_sum_out,
 * eq_loss_sums, coef_grads, grad_scale * eq_weight[e] rounded once on the host, the loss kinds, scratch
 * (PINN_SYSTEM_SCRATCH_DOUBLES), per-block double partials added in block order by the finish launch, no atomics, one launch
 * when no sum is wanted, N == 0 a no-op — as pinn_term_residual_system_mixed: with no function factor in the program the
 * residuals and every cotangent block are bit-identical to it on the same inputs, whatever n_functions is.
 * Checked on the host before any HIP call: every check of pinn_term_residual_system_mixed; n_functions outside [0, 4]; a code
 * 27 + k with k >= n_functions; null fn_values under a named function with N > 0: PINN_ERR_BAD_DESC, the message naming the
 * term. */
#define PINN_SYSTEM_MAX_FUNCTIONS 4
#define PINN_TERM_FN0 27
#define PINN_TERM_FN1 28
#define PINN_TERM_FN2 29
#define PINN_TERM_FN3 30

typedef struct PinnTermPdeSystemFn {
  int32_t dimension;                                   /* 1 .. 3 (a mixed factor needs 2 or 3) */
  int32_t n_fields;
  int32_t n_equations;
  int32_t time_order[PINN_SYSTEM_MAX_FIELDS];
  int32_t space_order[PINN_SYSTEM_MAX_FIELDS][3];
  int32_t n_terms;
  int32_t equation_of[PINN_SYSTEM_MAX_TERMS];
  float eq_weight[PINN_SYSTEM_MAX_EQUATIONS];
  int32_t loss;
  float huber_delta;
  PinnTermPdeTerm terms[PINN_SYSTEM_MAX_TERMS];        /* factor[f] = PINN_SYSTEM_FACTOR(field, code), code 0 .. 16, 21 .. 23, 27 .. 30 */
  int32_t pair_order[PINN_SYSTEM_MAX_FIELDS][3];       /* per field, pairs (x,y), (x,z), (y,z): 0 or 2 */
  int32_t n_functions;                                 /* 0 .. PINN_SYSTEM_MAX_FUNCTIONS: rows of fn_values */
} PinnTermPdeSystemFn;

int pinn_term_residual_system_fn(const PinnTermPdeSystemFn* pde, const float* coef_values, const float* const* jets,
                                 const float* x, const float* t, const float* fn_values, int64_t N, float grad_scale,
                                 const float* residual_cotangent, float* residual_out, float* loss_sum_out, float* eq_loss_sums,
                                 float* const* jet_cotangents, float* coef_grads, double* scratch, void* stream);

/* ---- term residuals of coupled systems with nonlinear functions of the unknowns as factors ----------------------------------
 * pinn_term_residual_system_fn plus up to PINN_SYSTEM_MAX_NONLINEAR factors w_k = g_k(shift_k + scale_k s_k), where s_k is a
 * stream of a field or an earlier w_j (j < k, so functions nest): 1 / rho, exp(u), u / (K + u), exp(-E / T), u^m, kappa(u).
 * The factor byte PINN_SYSTEM_FACTOR(k, PINN_TERM_NL) (code 31, the field bits carry k) names w_k; every other code keeps the
 * meaning it has in pinn_term_residual_system_fn, and the codes 17 .. 20 and 24 .. 26 stay refused by name.
 *   nl_op[k]           one of PINN_NL_*.
 *   nl_source[k]       a factor byte of the same encoding: a stream of a field (codes 0 .. 6, 11 .. 14, 21 .. 23: derivative
 *                      streams and u_ab included; no coordinate, no known function, no sin / cos code), or
 *                      PINN_SYSTEM_FACTOR(j, PINN_TERM_NL) with j < k.  The descriptor must hold a source exactly as it must hold
 *                      a term factor: the same checks, the messages saying "nonlinear function k" for "term m, factor f".
 *   nl_params          3 n_nonlinear device floats, {shift, scale, exponent} of function k at nl_params + 3 k, read at launch
 *                      time like coef_values.  exponent is read by PINN_NL_POW only.  May be NULL when no term names a
 *                      nonlinear function.
 * All in fp32.  arg = fmaf(scale, s, shift) (one rounding), w = g(arg) the value, slope = g'(arg), d_k = slope * scale (one
 * rounding):
 *   PINN_NL_EXP    w = expf(arg)      slope = w
 *   PINN_NL_LOG    w = logf(arg)      slope = 1.0f / arg
 *   PINN_NL_RECIP  w = 1.0f / arg     slope = -(w * w)
 *   PINN_NL_SQRT   w = sqrtf(arg)     slope = 0.5f / w
 *   PINN_NL_POW    w = powf(arg, p)   slope = p * powf(arg, p - 1.0f)       (p = exponent)
 *   PINN_NL_TANH   w = tanhf(arg)     slope = 1.0f - w * w
 *   PINN_NL_SINH   w = sinhf(arg)     slope = coshf(arg)
 *   PINN_NL_COSH   w = coshf(arg)     slope = sinhf(arg)
 *   PINN_NL_SIN    w = sinf(arg)      slope = cosf(arg)
 *   PINN_NL_COS    w = cosf(arg)      slope = -sinf(arg)
 * An argument outside a function's domain (log or sqrt of a negative number, 1 / 0, a negative base under a fractional
 * exponent) is NOT checked: the value and the slope are what IEEE arithmetic gives, NaN or inf, and they spread through the
 * residual, the loss sums and every cotangent the function reaches.
 *   value pass         once per point, in ascending k, after the fields' values and the known functions: only the k of a
 *                      host-made, wave-uniform mask, which holds the functions some term names, closed under "is the source of
 *                      a masked function".  A function outside the mask is never evaluated and its parameters are never read.
 *   sweep 1            a nonlinear factor enters the product ((c_m phi_0) phi_1) ... at its position, like a known function;
 *                      likewise in coef_grads[m] = sum_n rbar prod_f phi_{m,f}.
 *   sweep 2            w_k is a cotangent target of its own, wbar_k, under the rule of the other targets: the summands of one term
 *                      that go to the same target are summed first in ascending f, multiplied by rbar, then added.  After the
 *                      term loop, in descending k over the mask, wbar_k * d_k (one rounding) is added to the accumulator of the
 *                      source: the (field, stream) accumulator, the pair accumulator g of a u_ab source, or wbar_j.  The
 *                      transposed polarisation and the write-out follow unchanged.
 * No gradient with respect to nl_params is produced.  Everything else as pinn_term_residual_system_fn: with n_nonlinear = 0, or
 * with no nonlinear factor named by a term, the residuals, every cotangent block and the sums are bit-identical to it on the same
 * inputs.
 * Checked on the host before any HIP call: every check of pinn_term_residual_system_fn; n_nonlinear outside [0, 4]; an unknown
 * nl_op; a source that is neither a stream nor an earlier nonlinear function, or that the descriptor does not hold; code 31 with
 * k >= n_nonlinear; null nl_params under a non-empty mask with N > 0: PINN_ERR_BAD_DESC, the message naming the function or the
 * term. */
#define PINN_SYSTEM_MAX_NONLINEAR 4
#define PINN_TERM_NL 31
#define PINN_NL_EXP 0
#define PINN_NL_LOG 1
#define PINN_NL_RECIP 2
#define PINN_NL_SQRT 3
#define PINN_NL_POW 4
#define PINN_NL_TANH 5
#define PINN_NL_SINH 6
#define PINN_NL_COSH 7
#define PINN_NL_SIN 8
#define PINN_NL_COS 9

typedef struct PinnTermPdeSystemNl {
  int32_t dimension;                                   /* 1 .. 3 (a mixed factor needs 2 or 3) */
  int32_t n_fields;
  int32_t n_equations;
  int32_t time_order[PINN_SYSTEM_MAX_FIELDS];
  int32_t space_order[PINN_SYSTEM_MAX_FIELDS][3];
  int32_t n_terms;
  int32_t equation_of[PINN_SYSTEM_MAX_TERMS];
  float eq_weight[PINN_SYSTEM_MAX_EQUATIONS];
  int32_t loss;
  float huber_delta;
  PinnTermPdeTerm terms[PINN_SYSTEM_MAX_TERMS];        /* factor[f] = PINN_SYSTEM_FACTOR(field, code), code 0 .. 16, 21 .. 23, 27 .. 31 */
  int32_t pair_order[PINN_SYSTEM_MAX_FIELDS][3];       /* per field, pairs (x,y), (x,z), (y,z): 0 or 2 */
  int32_t n_functions;                                 /* 0 .. PINN_SYSTEM_MAX_FUNCTIONS: rows of fn_values */
  int32_t n_nonlinear;                                 /* 0 .. PINN_SYSTEM_MAX_NONLINEAR: triples of nl_params */
  int32_t nl_op[PINN_SYSTEM_MAX_NONLINEAR];            /* PINN_NL_* */
  int32_t nl_source[PINN_SYSTEM_MAX_NONLINEAR];        /* a stream byte, or PINN_SYSTEM_FACTOR(j, PINN_TERM_NL) with j < k */
} PinnTermPdeSystemNl;

int pinn_term_residual_system_nl(const PinnTermPdeSystemNl* pde, const float* coef_values, const float* const* jets,
                                 const float* x, const float* t, const float* fn_values, const float* nl_params, int64_t N,
                                 float grad_scale, const float* residual_cotangent, float* residual_out, float* loss_sum_out,
                                 float* eq_loss_sums, float* const* jet_cotangents, float* coef_grads, double* scratch,
                                 void* stream);

/* ---- term residuals of coupled systems with learnable parameters (inverse problems) -----------------------------------------
 * pinn_term_residual_system_nl with up to PINN_SYSTEM_MAX_PARAMS learnable scalars theta_p behind the coefficients and the
 * entries of the nonlinear triples: a viscosity, a diffusion tensor, a Monod constant K in u / (K + u), an exponent.
 *   coef_param[m]      -1, or the index p of the parameter c_m is a multiple of;
 *   nl_param[k][j]     the same for shift (j = 0), scale (1) and exponent (2) of function k; a learnable exponent needs PINN_NL_POW;
 *   param_values       n_params device floats, read at launch time like coef_values (no host copy: a captured graph follows an
 *                      optimiser that updates them in place); may be NULL when every index is -1;
 *   effective values   c_m = coef_param[m] < 0 ? coef_values[m] : coef_values[m] * param_values[coef_param[m]] (one rounding), and
 *                      the same rule for each entry of a triple from nl_params: for a learnable entry the stored number is the
 *                      scale.  A function outside the evaluation mask has none of its three entries read.
 * Residuals, losses, cotangent blocks, eq_loss_sums and coef_grads are pinn_term_residual_system_nl's on the effective values,
 * in its arithmetic and rounding order; coef_grads[m] is the derivative with respect to the EFFECTIVE c_m.  With n_params = 0
 * and both parameter pointers NULL every output is bit-identical to pinn_term_residual_system_nl on the same inputs.
 *   param_grads        nullable, n_params floats:
 *                        param_grads[p] += sum_{m: coef_param[m] = p} coef_values[m] G_m
 *                                        + sum_{(k, j): nl_param[k][j] = p} nl_params[3 k + j] H_kj,
 *                      G_m = sum_n rbar prod_f phi_{m,f} (the coefficient sum), and with wbar_k the COMPLETE cotangent of w_k (after
 *                      the pushes of the later functions, in descending k), slope = g_k'(arg_k) as tabulated above (without the
 *                      scale) and s_k the source value:
 *                        H_k0 = sum_n wbar_k * slope,   H_k1 = sum_n (wbar_k * slope) * s_k,
 *                        H_k2 = sum_n (wbar_k * w_k) * logf(arg_k)          (PINN_NL_POW only).
 *                      Each product is rounded to fp32 in the order written; the sums over the points are per-block partials in
 *                      double, added in block order by the finish launch, which also forms the combination in double, over m,
 *                      then over (k, j), ascending, and rounds once at the add to param_grads[p].  A function outside the mask
 *                      contributes 0.  param_grads carries grad_scale, the equation weights and a given residual_cotangent exactly
 *                      as coef_grads does (through rbar).  With jet_cotangents NULL the kernel still runs sweep 2 where an H sum is
 *                      wanted, and the sums have the bits of the full call.  No atomics: two calls are bit-identical.
 *   scratch            PINN_SYSTEM_INV_SCRATCH_DOUBLES doubles, 8-byte aligned: 64 blocks x {4 equation sums, 32 G, 12 H (3 k + j)}.
 * Checked on the host before any HIP call: every check of pinn_term_residual_system_nl; n_params outside [0, 8]; a coef_param
 * (m < n_terms) or nl_param (k < n_nonlinear) outside [-1, n_params); a learnable exponent on another operation than
 * PINN_NL_POW; NULL param_values with any index >= 0 and N > 0; param_grads without scratch: PINN_ERR_BAD_DESC, the message
 * naming the term or the function. */
#define PINN_SYSTEM_MAX_PARAMS 8
#define PINN_SYSTEM_INV_SCRATCH_DOUBLES (64 * (4 + 32 + 12))

typedef struct PinnTermPdeSystemInv {
  int32_t dimension;                                   /* the fields of PinnTermPdeSystemNl, in its order */
  int32_t n_fields;
  int32_t n_equations;
  int32_t time_order[PINN_SYSTEM_MAX_FIELDS];
  int32_t space_order[PINN_SYSTEM_MAX_FIELDS][3];
  int32_t n_terms;
  int32_t equation_of[PINN_SYSTEM_MAX_TERMS];
  float eq_weight[PINN_SYSTEM_MAX_EQUATIONS];
  int32_t loss;
  float huber_delta;
  PinnTermPdeTerm terms[PINN_SYSTEM_MAX_TERMS];
  int32_t pair_order[PINN_SYSTEM_MAX_FIELDS][3];
  int32_t n_functions;
  int32_t n_nonlinear;
  int32_t nl_op[PINN_SYSTEM_MAX_NONLINEAR];
  int32_t nl_source[PINN_SYSTEM_MAX_NONLINEAR];
  int32_t n_params;                                    /* 0 .. PINN_SYSTEM_MAX_PARAMS */
  int32_t coef_param[PINN_SYSTEM_MAX_TERMS];           /* -1 or a parameter index */
  int32_t nl_param[PINN_SYSTEM_MAX_NONLINEAR][3];      /* -1 or a parameter index: shift, scale, exponent */
} PinnTermPdeSystemInv;

int pinn_term_residual_system_inv(const PinnTermPdeSystemInv* pde, const float* coef_values, const float* const* jets,
                                  const float* x, const float* t, const float* fn_values, const float* nl_params,
                                  const float* param_values, int64_t N, float grad_scale, const float* residual_cotangent,
                                  float* residual_out, float* loss_sum_out, float* eq_loss_sums, float* const* jet_cotangents,
                                  float* coef_grads, float* param_grads, double* scratch, void* stream);

/* torch.nn.utils.clip_grad_norm_(params, max_norm) (skipped when max_norm <= 0) followed by
 * torch.optim.Adam(lr, (beta1, beta2), eps, weight_decay).step() on ONE flat fp32 buffer of n elements.
 * lr and step are DEVICE scalars (step = number of steps taken so far, incremented by the call) so that a captured
 * graph follows a learning-rate schedule; scratch64: 64 floats; grad_norm_out: nullable, receives the norm before
 * clipping.  The norm is reduced in a fixed order: deterministic. */
int pinn_adam_clip_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, const float* lr,
                        float beta1, float beta2, float eps, float weight_decay, float max_norm, float* step,
                        float* scratch64, float* grad_norm_out, void* stream);

/* Adaptive loss weights (pinnrl/components/adaptive_weights.py:35-107, the trainer block trainer.py:586-684) fused with the
 * optimiser step: weight update + combination of the component gradients + clip_grad_norm_ + Adam, all on the device.
 * The weights are detached numbers, so the gradient of  total = sum_c w_c L_c  is  sum_c w_c grad(L_c).
 *   comp_grads   n_components (<= 4) rows of `ld` >= n floats: row c = gradient of the UNweighted component c
 *                (the trainer: residual, boundary, initial);
 *   comp_losses  HOST table of n_components device pointers, one float each; L_c = comp_losses[c][0] * loss_scales[c]
 *                (loss_scales: host, nullable = ones; e.g. a residual launch's loss sum with scale 1 / N);
 *   strategy     PINN_ADAPTIVE_RBW: v = L (loss magnitudes), PINN_ADAPTIVE_LRW: v_c = |grad(L_c)|_2;
 *   initial_weights  host, n_components floats, nullable = ones: the weights of the first call;
 *   state16      16 device floats owned by the caller, zero before the first call:
 *                {running[4], prev_weights[4], weights[4], calls, has_prev, -, -};
 *   weights4_out (nullable) the weights of this step, padded with 0;  summary4 (nullable) {L_0, L_1, L_2, sum_c w_c L_c};
 *   grad_norm_out (nullable) the norm of the combined gradient before clipping;  grad_out (nullable) the combined
 *                gradient before clipping, n floats — it is not written to memory otherwise;
 *   scratch      PINN_ADAPTIVE_SCRATCH_FLOATS floats, 8-byte aligned;  the rest as pinn_adam_clip_step (`step` is incremented).
 * The rule: first call running = v, weights = initial_weights; later calls running = alpha running + (1 - alpha) v and
 * LRW  w = inv / sum(inv), inv = 1 / (running + aw_eps);  RBW  w = running / (sum(running) + aw_eps), smoothed with the
 * previous RBW weights from the third call on (w = alpha prev + (1 - alpha) w).
 * Three launches: a Gram pass <g_a, g_b> over a fixed grid (partials and their sum in double, fixed order), one workgroup
 * for the rule and the clip norm sqrt(w^T G w) (the only launch that writes the state), the update pass.  No atomics:
 * bit-identical across runs.  16-byte loads where params / moments / rows (base and ld) are 16-byte aligned, else scalar. */
#define PINN_ADAPTIVE_RBW 0
#define PINN_ADAPTIVE_LRW 1
#define PINN_ADAPTIVE_SCRATCH_FLOATS 1296
int pinn_adaptive_adam_step(float* params, const float* comp_grads, int64_t ld, int32_t n_components,
                            const float* const* comp_losses, const float* loss_scales, int32_t strategy, double alpha,
                            double aw_eps, const float* initial_weights, float* state16, float* weights4_out, float* summary4,
                            float* exp_avg, float* exp_avg_sq, int64_t n, const float* lr, float beta1, float beta2, float eps,
                            float weight_decay, float max_norm, float* step, float* scratch, float* grad_norm_out,
                            float* grad_out, void* stream);

/* ---- L-BFGS (pinnrl/training/trainer.py:299-309, 373-389; torch/optim/lbfgs.py) --------------------------------------
 * torch.optim.LBFGS on ONE flat fp32 buffer of n elements.  The host keeps the control flow of step() and of the strong-Wolfe
 * line search on scalars; these two entry points do everything that touches the n-vectors and hand the host one small record
 * per call.  All memory is the caller's:
 *   ring       2 * (history_size + 1) rows of `ld` >= n floats: the s rows of the history_size + 1 slots, then their y rows.
 *              The spare slot takes the tentative pair, so a rejected pair destroys nothing;
 *   prev_grad, direction   n floats each (direction: zero before the first call);
 *   state      pinn_lbfgs_state_bytes(history_size) bytes, 8-byte aligned, doubles: {ring head, count, n_iter, H_diag, 4 spare},
 *              ro per slot, and the Gram matrix of the ring rows.  ALL ZERO = empty history, n_iter = 0;
 *   scratch    pinn_lbfgs_scratch_bytes(history_size) bytes, 8-byte aligned (partials, coefficients);
 *   record     PINN_LBFGS_RECORD_DOUBLES doubles, 8-byte aligned (PINN_LBFGS_REC_*).
 * history_size in [1, PINN_LBFGS_MAX_HISTORY]; the two size queries return 0 outside it.
 *
 * pinn_lbfgs_direction: one direction update (lbfgs.py:396-460) from the gradient `grad` of the accepted point, in three
 * launches.  (1) Update pass, fixed grid: the tentative pair y = grad - prev_grad, s = (float)t_prev * direction into the
 * spare slot, prev_grad = grad, and per-block partials (double products and sums) of the inner products of {s, y, grad}
 * with every live ring row and each other, of max|grad| and sum|grad|.  With n_iter == 0 it does none of the pair work.
 * (2) One workgroup, the only launch that writes the state: sums the partials in a fixed order; accepts the pair iff
 * y.s > 1e-10 (advance the ring, evict the oldest pair of a full ring, ro = 1 / y.s, H_diag = y.s / y.y, new Gram row and
 * column; a rejected pair leaves ring and Gram untouched); runs the two-loop recursion in COEFFICIENT space — q and r are
 * combinations of {grad, s_i, y_i}, so each s_i.q and y_i.r is a dot of a Gram row with the coefficients, in double, in
 * torch's order (newest to oldest, scale by H_diag, oldest to newest); writes the 2 count + 1 coefficients and
 * gtd = grad.direction from the Gram matrix.  With n_iter == 0: direction = -grad, an empty history, H_diag = 1.
 * (3) Combine pass: direction[i] = sum_j coef_j basis_j[i], accumulated in double in registers and rounded once, and one
 * max|direction| partial per block.
 * Record: LOSS 0, GTD, GMAX = max|grad|, GSUM = sum|grad|, ACCEPTED (0 | 1), COUNT (live pairs), ITER (n_iter after the
 * call), HDIAG, and from PINN_LBFGS_REC_DMAX on 64 per-block partials whose maximum is max|direction|.
 * Numerics: the coefficient-space recursion equals torch's vector recursion mathematically; its scalars are double and its
 * Gram entries are double sums of exact fp32 products; it would lose accuracy against the direct form only under
 * cancellation of order 1e7 or more.
 *
 * pinn_lbfgs_eval_stats: what the line search reads of one evaluated trial point, two launches (partials, then a
 * fixed-order sum in double): LOSS = loss[0] (device float, e.g. the total of summary4; nullable = 0), GTD = grad.direction,
 * GMAX, GSUM; the rest of the record is zeroed.  scratch: 192 doubles (pinn_lbfgs_scratch_bytes covers them).
 * No atomics anywhere: bit-identical across runs.  16-byte loads where every n-vector (base, and ld of the ring) is
 * 16-byte aligned, scalar loads otherwise. */
#define PINN_LBFGS_MAX_HISTORY 64
#define PINN_LBFGS_RECORD_DOUBLES 72
#define PINN_LBFGS_REC_LOSS 0
#define PINN_LBFGS_REC_GTD 1
#define PINN_LBFGS_REC_GMAX 2
#define PINN_LBFGS_REC_GSUM 3
#define PINN_LBFGS_REC_ACCEPTED 4
#define PINN_LBFGS_REC_COUNT 5
#define PINN_LBFGS_REC_ITER 6
#define PINN_LBFGS_REC_HDIAG 7
#define PINN_LBFGS_REC_DMAX 8
size_t pinn_lbfgs_state_bytes(int32_t history_size);
size_t pinn_lbfgs_scratch_bytes(int32_t history_size);
int pinn_lbfgs_direction(const float* grad, float* prev_grad, float* direction, float* ring, int64_t ld, int64_t n,
                         int32_t history_size, double t_prev, double* state, double* scratch, double* record, void* stream);
int pinn_lbfgs_eval_stats(const float* grad, const float* direction, int64_t n, const float* loss, double* scratch,
                          double* record, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PINN_JET_H */
