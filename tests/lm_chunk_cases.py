"""GPU cases: every entry point of the layer-major engine across the chunk loop of lm_run, against fp64 autograd.

lm_run (csrc/lm_engine.hip) cuts a batch into chunks of `ct` tiles so that one record stays near record_target_bytes() —
1 GB, so at test sizes the loop body runs once.  PINN_LM_RECORD_MB is read once per process: this module is NOT collected by
the ordinary run (its name does not match test_*.py); tests/test_fused_policies.py::test_chunk_loop_cases_under_policy runs it
by path in child processes with PINN_LM_RECORD_MB=1, fused and unfused, and checks that all N_CASES cases passed.

Multi-chunk, proved per case before anything is compared.  With a 1 MB target make_layout gives
ct = max(64, 2^20 / (K round32(hmax) 128)) tiles: 64 tiles = 2048 points exactly when K round32(hmax) >= 128.  Every case
asserts that the kernel query of its own launch descriptor names the layer-major engine and that pinn_workspace_bytes of that
descriptor, with the launch's own `backward` code, is the same for its N as for N = 2048 (the records are sized by ct alone;
a sheared launch adds two N-sized coordinate copies, which are subtracted first): then ct is 64 tiles and the call takes at
least two chunks.  N = 5127: three chunks, a ragged last tile of 7 points; 4097: the third chunk holds ONE point; 4096: two
exact chunks, no ragged tile anywhere.

The reference (never the engine): fp64 autograd through oracle.network_forward / oracle.compute_residual (the autoencoder, which
the oracle does not have: through the node model of tests/jet_model.py, as tests/test_autoencoder_gpu.py does), evaluated on
P_DISTINCT = 203 distinct points only.  Point i of a launch is distinct point i mod 203.  203 is odd and 2048 mod 203 = 18, so
no two tiles and no two chunks hold the same points in the same places: a launch that reads another chunk's coordinates
(p_base of EwArgs / HeadArgs) changes every per-point output.  The cotangents `cot` (K, N) and `res_bar` (N) are random PER
INDEX i, not per distinct point — a launch that reads another chunk's cotangents is wrong too — fp32-representable, stream s
scaled by 1 / |jet_s|.  What makes 203 points enough:
  * the pairing sum_i c_i J(p_{i mod 203}) is linear in the jets, so its parameter gradient is the gradient of
    sum_j C_j J(p_j) over the 203 distinct points with C_j = sum_{i = j mod 203} c_i accumulated in fp64; the same for
    <res_bar, r>;
  * the loss and its gradients (parameters and PDE coefficients) weight distinct point j by the number of times it occurs;
  * per-point outputs — every jet stream, the residual, every column of x_grad, t_grad — are compared at ALL N indices against
    ref[i mod 203]; x_grad[i] = sum_s c_{s,i} dJ_s/dx(p_{i mod 203}) uses index i's own cotangent.  The indices next to the
    chunk borders (2047, 2048, 4095, 4096, N - 1) are where an offset goes wrong, so nothing is compared on a sample.
tests/test_lm_chunk_reference_cpu.py proves the construction without a GPU: fp64 autograd over all N points reproduces it to
1e-12.

Every reverse launch starts from a workspace filled with NaN (sized for the launch first) and from accumulators — flat_grad,
coef_grads — holding a known non-zero fill of the size of the expected gradient (a fill of another size would cost the fp32 sum
the digits the bars ask for): what is compared is result minus fill.  x_grad and t_grad are allocated by engine.py inside the
call and written, not accumulated.  In deterministic mode every reverse launch runs twice and every output is bit-identical.
Per-point outputs of one multi-chunk launch are bit-equal to the concatenation of per-chunk launches of the same engine.

Bars are the project's: tests/test_lm_variants_gpu.py (residual, loss, concatenated gradient 1e-5; u and derivative streams
2e-5, derivative streams of LayerNorm networks 5e-5), hip_helpers.check_tensors per tensor (1e-4 with its fp32-floor rule, at
most WIDENED_CAP of the compared tensors on a widened bar: the last case), tests/test_input_grad_gpu.py for x_grad / t_grad
(1e-5), tests/test_data_modes.py for coefficient sums (2e-5 relative + 1e-9).  Measured values: profiles/parity_lm_chunks.md.
"""

import ctypes
import dataclasses
import json
import os
from typing import Optional, Tuple

import pytest
import torch

from conftest import _PARITY_LOG, rel_err, rel_l2
from hip_helpers import check_tensors, pde_desc_from_spec, program_from_spec
from test_input_grad_gpu import TOL as INPUT_TOL
from test_lm_variants_gpu import LN_STREAM_TOL, STREAM_TOL, TOL, WIDENED_CAP
from test_wide_variants_gpu import P_DISTINCT, PDE_PARAMS, _cotangent, _grads, _params64, _points, _poison, _trainable

pytestmark = pytest.mark.gpu

COEF_TOL, COEF_ABS = 2e-5, 1e-9  # tests/test_data_modes.py::test_fused_coefficient_gradients_match_the_oracle
CHUNK_POINTS = 64 * 32           # ct = 64 tiles of 32 points
N_FULL, N_ONE, N_EXACT = 5127, 4097, 4096
COEFS = {"burgers": ("nu",), "allen_cahn": ("epsilon",), "black_scholes": ("sigma", "r")}
MAX_SHARE = 0.25  # of the squared norm of a per-point output that one of the 203 distinct points may carry (an even share: 0.005)


@dataclasses.dataclass(frozen=True)
class Net:
    name: str
    streams: Tuple[int, int]
    seed: int
    spec: object = None              # oracle.ArchSpec, or None for the autoencoder
    auto: Optional[str] = None       # a shape of tests/test_autoencoder_gpu.py::SHAPES
    pde: Optional[str] = None        # None: the three jet entry points only
    axis: int = 0
    direction: Optional[Tuple[int, ...]] = None
    component: int = 0

    @property
    def input_dim(self):
        return 2 if self.spec is None else self.spec.input_dim

    def line(self):
        """The direction the space streams differentiate along, one entry per space column."""
        if self.direction is not None:
            return [float(v) for v in self.direction]
        return [1.0 if c == self.axis else 0.0 for c in range(self.input_dim - 1)]

    def sheared(self):
        return self.axis != 0 or self.direction is not None


def networks():
    """One network per structure the chunk loop treats differently (name -> Net)."""
    import oracle as O

    ff3 = O.ArchSpec("feedforward", input_dim=3, hidden_dim=128, num_layers=3, activation="tanh")
    nets = [
        # Stats and skip records, 256-multiple dW jobs batched across the sweep, lm_gemm_wres
        Net("resnet_2x256", (1, 2), 7100, O.ArchSpec("resnet", hidden_dim=256, num_layers=2, num_blocks=2, activation="tanh"), pde="allen_cahn"),
        # merged W_p W_v gradient (lm_unmerge_pv_kernel behind the loop), depth 512
        Net("attention_1x128", (1, 4), 7110, O.ArchSpec("attention", hidden_dim=128, num_layers=1, num_heads=4, activation="gelu"), pde="cahn_hilliard"),
        Net("siren_3x128", (1, 3), 7120, O.ArchSpec("siren", hidden_dim=128, num_layers=3, omega_0=4.0), pde="kdv"),
        Net("fourier_4x128_burgers", (1, 2), 7130, O.ArchSpec("fourier", hidden_dim=128, num_layers=4, mapping_size=64, scale=2.0, activation="tanh"), pde="burgers"),
        # the epilogue reads x at the point
        Net("fourier_4x128_black_scholes", (1, 2), 7140, O.ArchSpec("fourier", hidden_dim=128, num_layers=4, mapping_size=64, scale=2.0, activation="tanh"), pde="black_scholes"),
        # time order 2, element-wise units only
        Net("ff_ln_gelu_3x64", (2, 2), 7150, O.ArchSpec("feedforward", hidden_dim=64, num_layers=3, activation="gelu", layer_norm=True), pde="wave"),
        Net("autoencoder_latent40", (1, 2), 11, auto="latent40", pde="burgers"),
        # xswap / xgswap are sized by N, the records by the chunk
        Net("ff3_axis1", (1, 2), 7170, ff3, axis=1),
        Net("ff3_direction", (0, 2), 7170, ff3, direction=(1, -1)),
        Net("ff_two_outputs_component1", (1, 2), 7190, O.ArchSpec("feedforward", hidden_dim=128, num_layers=3, activation="tanh", output_dim=2), component=1),
    ]
    return {n.name: n for n in nets}


REDUCED = ("resnet_2x256", "attention_1x128")  # the networks of the N = 4097 and N = 4096 cases
NET_NAMES = ("resnet_2x256", "attention_1x128", "siren_3x128", "fourier_4x128_burgers", "fourier_4x128_black_scholes",
             "ff_ln_gelu_3x64", "autoencoder_latent40", "ff3_axis1", "ff3_direction", "ff_two_outputs_component1")
CASES = ([(name, N_FULL, det) for name in NET_NAMES for det in (False, True)]
         + [(name, n, det) for name in REDUCED for n in (N_ONE, N_EXACT) for det in (False, True)])
N_CASES = len(CASES) + 1  # and the widened-bar cap, last


# ---- the fp64 reference -------------------------------------------------------------------------------------------------
def has_ln(net):
    if net.auto is not None:
        from test_autoencoder_gpu import SHAPES

        return SHAPES[net.auto][3]
    return net.spec.architecture in ("resnet", "attention") or bool(net.spec.layer_norm)


def state_dict(net):
    """theta_0 with every 1-D tensor (biases, LayerNorm weights and biases) perturbed by 0.2 N(0, 1), as the fixtures of the
    autoencoder and tests/test_components_gpu.py do.  With theta_0's zero biases a LayerNorm that sits on the first Linear
    (attention) is singular near the origin, and ONE of the 203 points then carries 99 % of the norm of u_xxx, u_xxxx and
    the residual: the comparison of those outputs, and of every sum over the points, would be a one-point comparison
    (tests/test_lm_chunk_reference_cpu.py holds every output's largest share below MAX_SHARE)."""
    import autoencoder_model as AM
    import oracle as O

    if net.auto is not None:
        from test_autoencoder_gpu import _random_sd

        return _random_sd(net.auto, net.seed)
    return AM.perturb(O.init_state_dict(net.spec, seed=net.seed), net.seed + 1, 0.2)


def forward(net, params, inp):
    """u (P, 1) of the launch's component, in the dtype of `params`."""
    import oracle as O

    if net.auto is not None:
        import autoencoder_model as AM
        import jet_model as JM
        from test_autoencoder_gpu import SHAPES

        hidden, _, act, ln = SHAPES[net.auto]
        return JM.program_forward(AM.autoencoder_program(params, len(hidden), act, ln), inp, 0, 0)[0][0]
    return O.network_forward(net.spec, params, inp, "composite")[:, net.component : net.component + 1]


def distinct_points(net):
    return _points(net.input_dim, P_DISTINCT, net.seed + 1)


def _f32(v):
    return float(torch.tensor(float(v), dtype=torch.float32))


def pde_parameters():
    """The coefficients as the fp32 numbers the descriptor holds."""
    return {k: _f32(v) for k, v in dict(PDE_PARAMS, sigma=0.2, r=0.05).items()}


def pde_spec(net, live=None):
    import oracle as O

    return O.PdeSpec(name=net.pde, dimension=1, domain=((-1.0, 1.0),), parameters=dict(pde_parameters(), **(live or {})))


def line_jets(net, params, x, t, dtype=torch.float64):
    """[u, d/dt .., (sum_c line_c d/dx_c)^k ..] ((P,) each) with the graph kept; x, t are leaves."""
    nt, nx = net.streams
    tau = torch.zeros(x.shape[0], 1, dtype=dtype, requires_grad=True)
    u = forward(net, params, torch.cat([x + tau * torch.tensor(net.line(), dtype=dtype), t], 1))
    out, cur = [u], u
    for _ in range(nt):
        cur = torch.autograd.grad(cur, t, torch.ones_like(cur), create_graph=True)[0]
        out.append(cur)
    cur = u
    for _ in range(nx):
        cur = torch.autograd.grad(cur, tau, torch.ones_like(cur), create_graph=True)[0]
        out.append(cur)
    return [j[:, 0] for j in out]


def _cast(params, dtype):
    if dtype == torch.float64:
        return params
    return {k: v.detach().to(dtype).requires_grad_(v.requires_grad) for k, v in params.items()}


def reference(net, N, x=None, t=None, idx=None, like=None, dtype=torch.float64):
    """The reference of an N-point launch whose point i is row idx[i] of (x, t) — by default the 203 distinct points and
    idx[i] = i mod 203.  `like`: take the cotangents of that evaluation (the fp32 floor of a tensor; the all-points proof of
    tests/test_lm_chunk_reference_cpu.py, which passes the N launch points themselves and idx[i] = i)."""
    import oracle as O

    if x is None:
        x, t = distinct_points(net)
        idx = torch.arange(N) % P_DISTINCT
    P, K = x.shape[0], 1 + sum(net.streams)
    sd = state_dict(net)
    params = _cast(_params64(sd), dtype)
    names = _trainable(params)
    xl, tl = x.to(dtype).clone().requires_grad_(True), t.to(dtype).clone().requires_grad_(True)
    J = line_jets(net, params, xl, tl, dtype)
    jets = torch.stack([j.detach() for j in J])
    cot = like["cot"] if like else _cotangent([j[idx] for j in jets.double()], net.seed + 2)   # (K, N): per index
    C = torch.zeros(K, P, dtype=torch.float64).index_add_(1, idx, cot)
    adj = _grads(sum((C[s].to(dtype) * J[s]).sum() for s in range(K)), params, names, retain_graph=True)
    xg = torch.zeros(N, x.shape[1], dtype=dtype)
    tg = torch.zeros(N, 1, dtype=dtype)
    for s in range(K):  # J_s at point j depends on point j alone: the gradient of the sum is the per-point derivative
        gx, gt = torch.autograd.grad(J[s].sum(), (xl, tl), retain_graph=True, allow_unused=True)
        c = cot[s].to(dtype).unsqueeze(1)
        if gx is not None:
            xg += c * gx[idx]
        if gt is not None:
            tg += c * gt[idx]
    res = {"sd": sd, "x": x, "t": t, "idx": idx, "names": names, "jets": jets, "cot": cot, "adj": adj, "xg": xg, "tg": tg}
    if net.pde is None:
        return res
    w = torch.bincount(idx, minlength=P).to(dtype).unsqueeze(1)
    live = {k: torch.tensor(pde_parameters()[k], dtype=dtype, requires_grad=True) for k in COEFS.get(net.pde, ())}
    pde = pde_spec(net, live)
    params = _cast(_params64(sd), dtype)
    r = O.compute_residual(pde, lambda inp: forward(net, params, inp), x.to(dtype).clone(), t.to(dtype).clone())
    L = (w * r**2).sum() / N  # mse over the N points of the launch
    rbar = like["rbar"] if like else torch.randn(N, generator=torch.Generator().manual_seed(net.seed + 3), dtype=torch.float64).float().double()
    R = torch.zeros(P, dtype=torch.float64).index_add_(0, idx, rbar).unsqueeze(1)
    gL = torch.autograd.grad(L, [params[k] for k in names] + list(live.values()), retain_graph=True, allow_unused=True)
    res.update(pde=pde_spec(net), r=r.detach(), L=L.detach(), rbar=rbar,
               gL={k: (g.detach() if g is not None else torch.zeros_like(params[k])) for k, g in zip(names, gL)},
               dcoef=[float(g) for g in gL[len(names):]], gR=_grads((R.to(dtype) * r).sum(), params, names))
    return res


# ---- the cases ----------------------------------------------------------------------------------------------------------
POLICY = "unfused" if os.environ.get("PINN_LM_FUSED") == "0" else "default"
TENSORS = {"compared": 0, "widened": []}
WORST = {}   # output kind -> (value, where)
RAN = []
_REFS = {}
_GPU_ERROR = []  # a HIP error in an earlier case: nothing further is launched


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _ref(net, N):
    if (net.name, N) not in _REFS:
        _REFS[(net.name, N)] = reference(net, N)
    return _REFS[(net.name, N)]


def _seen(kind, e, where):
    if e > WORST.get(kind, (0.0, ""))[0]:
        WORST[kind] = (e, where)


def _program(net, sd, dev):
    if net.auto is not None:
        from test_autoencoder_gpu import _program as auto_program

        return auto_program(net.auto, sd, dev), list(sd)
    return program_from_spec(net.spec, sd, dev)


class _DescView:
    """What the kernel queries read of a program, with the descriptor of the launch (axis, direction, component)."""

    def __init__(self, desc):
        self.desc = desc


def shear_copy_bytes(net, n, backward):
    """Bytes of the N-sized coordinate copies of a sheared launch (make_layout: xswap, and xgswap on every reverse call)."""
    if not net.sheared():
        return 0
    return 4 * (2 if backward else 1) * ((n * (net.input_dim - 1) + 3) & ~3)


def assert_multi_chunk(net, desc, N, what):
    """Item 2 of the module docstring, for the three `backward` codes of the entry points."""
    from pinnrl_amd import _lib

    nt, nx = net.streams
    lib = _lib.load()
    for backward in (0, 1, 2):
        assert _lib.kernel_for(_DescView(desc), N, nt, nx, backward)["engine"] == "layer_major", (what, backward)
        b_n = lib.pinn_workspace_bytes(ctypes.byref(desc), N, nt, nx, backward)
        b_c = lib.pinn_workspace_bytes(ctypes.byref(desc), CHUNK_POINTS, nt, nx, backward)
        assert b_n > 0 and b_c > 0, (what, backward)
        if net.sheared():  # the total is rounded up to 256 bytes after the copies; one more tile costs >= 4096 bytes per record
            assert abs((b_n - shear_copy_bytes(net, N, backward)) - (b_c - shear_copy_bytes(net, CHUNK_POINTS, backward))) < 256, (what, backward, b_n, b_c)
        else:
            assert b_n == b_c, (what, backward, b_n, b_c)
    assert N > CHUNK_POINTS


def _poison_sized(prog, dev, nbytes, N, nt, nx):
    from pinnrl_amd import engine as E

    E._workspace(dev, nbytes)
    _poison(prog, dev, N, nt, nx)


class _Filled:
    """A flat gradient that starts from a known non-zero fill of the size of the expected gradient, per tensor."""

    def __init__(self, prog, names_all, want, dev, seed):
        from pinnrl_amd import engine as E

        self.prog, self.names_all = prog, names_all
        self.flat = E.new_flat_grad(prog, dev)
        g = torch.Generator().manual_seed(seed)
        for name, slot in zip(names_all, E.split_flat_grad(prog, self.flat)):
            if slot is None:
                continue
            rms = float(want[name].norm()) / max(want[name].numel(), 1) ** 0.5 if name in want else 0.0
            slot.copy_(((rms if rms > 0.0 else 1.0) * (1.0 + torch.rand(slot.shape, generator=g))).to(dev))
        self.fill = self.flat.clone()

    def result(self):
        """{name: what the launch added}, on the CPU in fp64."""
        from pinnrl_amd import engine as E

        assert not torch.equal(self.flat, self.fill), "the launch left the gradient buffer untouched"
        delta = self.flat.double() - self.fill.double()
        return {n: g.cpu() for n, g in zip(self.names_all, E.split_flat_grad(self.prog, delta)) if g is not None}


SURVEY = bool(os.environ.get("PINN_LM_CHUNK_SURVEY"))  # evaluate every check of a case and report all that miss, not the first
_MISSED = []


def _expect(ok, message):
    """A comparison of a case: an assertion, or under PINN_LM_CHUNK_SURVEY=1 an entry of the list the case fails with at its
    end (which checks see a deliberately broken engine: profiles/parity_lm_chunks.md)."""
    if SURVEY and not ok:
        _MISSED.append(message)
        return
    assert ok, message


def _check_grads(net, got, want, what, floor):
    keys = list(want)
    assert set(keys) <= set(got), what
    flat_got = torch.cat([got[k].flatten() for k in keys])
    _expect(torch.isfinite(flat_got).all(), f"{what}: non-finite gradient")

    def seen(k, e):
        TENSORS["compared"] += 1
        _seen("state_dict tensor", e, f"{what} {k}")

    try:
        TENSORS["widened"] += check_tensors(got, want, what, floor, seen)
    except AssertionError as exc:
        _expect(False, str(exc).split("\n")[0])
    e = rel_l2(flat_got, torch.cat([want[k].flatten() for k in keys]), label=f"{what} gradient", tol=TOL)
    _seen("concatenated gradient", e, what)
    print(f"{what}: concatenated gradient {e:.2e}")
    _expect(e <= TOL, f"{what}: concatenated gradient {e:.2e}")


def _run_case(net, N, det, dev):
    from pinnrl_amd import _lib
    from pinnrl_amd import engine as E

    nt, nx = net.streams
    K = 1 + nt + nx
    full = N == N_FULL
    tag = f"{net.name} N={N} {'deterministic' if det else 'default'}"
    o = _ref(net, N)
    floors = {}

    def floor(which):
        def get():
            if "o32" not in floors:
                floors["o32"] = reference(net, N, like=o, dtype=torch.float32)
            return floors["o32"][which]
        return get

    prog, names_all = _program(net, o["sd"], dev)
    prog.set_layer_major(True)
    prog.set_deterministic(det)
    line = dict(axis=net.axis, direction=net.direction, component=net.component)
    desc = E._launch_desc(prog, net.axis, net.direction, net.component)
    assert_multi_chunk(net, desc, N, tag)
    lib = _lib.load()
    ws_bytes = max(lib.pinn_workspace_bytes(ctypes.byref(desc), N, nt, nx, b) for b in (1, 2))
    idx = o["idx"].to(dev)
    x, t = o["x"].to(dev)[idx].contiguous(), o["t"].to(dev)[idx].contiguous()
    cot = o["cot"].float().to(dev)
    ln = has_ln(net)
    chunks = [(lo, min(N, lo + CHUNK_POINTS)) for lo in range(0, N, CHUNK_POINTS)]
    assert len(chunks) == (2 if N == N_EXACT else 3)
    want_adj = dict(o["adj"])
    if prog.n_outputs > 1:  # the reference differentiates u[:, component]: the other rows of the output layer get exact zeros
        for k in names_all[-2:]:
            assert float(want_adj[k][net.component].norm()) > 0.0 and all(
                float(want_adj[k][j].norm()) == 0.0 for j in range(prog.n_outputs) if j != net.component)

    def twice(launch):
        """Run a reverse launch (twice in deterministic mode: every output bit-identical); its outputs."""
        out = launch()
        if det:
            again = launch()
            for a, b in zip(out, again):
                _expect((a is None and b is None) or torch.equal(a, b), f"{tag}: deterministic launches differ")
        return out

    # (a) every stream of the forward launch, at every index; bit-equal to per-chunk launches
    if full:
        jets = E.jets_forward(prog, x, t, nt, nx, **line)
        for s in range(K):
            bar = STREAM_TOL if s == 0 else (LN_STREAM_TOL if ln else STREAM_TOL)
            e = rel_l2(jets[s].cpu(), o["jets"][s][o["idx"]], label=f"{tag} jet stream {s}", tol=bar)
            _seen("u" if s == 0 else "derivative stream", e, f"{tag} stream {s}")
            print(f"{tag}: jet stream {s}: {e:.2e}")
            _expect(e <= bar, f"{tag}: jet stream {s}: {e:.2e}")
        parts = torch.cat([E.jets_forward(prog, x[lo:hi], t[lo:hi], nt, nx, **line) for lo, hi in chunks], 1)
        _expect(torch.equal(parts, jets), f"{tag}: jets differ between one multi-chunk launch and per-chunk launches")

        # (b) the jet adjoint
        def jets_backward():
            _poison_sized(prog, dev, ws_bytes, N, nt, nx)
            f = _Filled(prog, names_all, want_adj, dev, net.seed + 5)
            E.jets_backward(prog, x, t, nt, nx, cot, f.flat, **line)
            jets_backward.filled = f
            return (f.flat,)
        twice(jets_backward)
        _check_grads(net, jets_backward.filled.result(), want_adj, f"{tag} adjoint", floor("adj"))

    # (c) input cotangents: with a gradient table, without one (no dW path), x alone; at every index
    def inputs(with_table, want_x, want_t):
        def launch():
            _poison_sized(prog, dev, ws_bytes, N, nt, nx)
            f = _Filled(prog, names_all, want_adj, dev, net.seed + 6) if with_table else None
            xg, tg = E.jets_backward_inputs(prog, x, t, nt, nx, cot, f.flat if f else None, want_x, want_t, **line)
            launch.filled = f
            return xg, tg, (f.flat if f else None)
        out = twice(launch)
        return out[0], out[1], launch.filled

    xg, tg, f = inputs(True, True, True)
    e_x = rel_l2(xg.cpu(), o["xg"], label=f"{tag} x_grad", tol=INPUT_TOL)
    e_t = rel_l2(tg.cpu(), o["tg"], label=f"{tag} t_grad", tol=INPUT_TOL)
    _seen("x_grad", e_x, tag)
    _seen("t_grad", e_t, tag)
    print(f"{tag}: x_grad {e_x:.2e}, t_grad {e_t:.2e}")
    _expect(e_x <= INPUT_TOL and e_t <= INPUT_TOL, f"{tag}: x_grad {e_x:.2e}, t_grad {e_t:.2e}")
    got = f.result()
    if prog.n_outputs > 1:  # rows of the other components: the fill, bit for bit
        for k, slot, fill in zip(names_all, E.split_flat_grad(prog, f.flat), E.split_flat_grad(prog, f.fill)):
            if k in names_all[-2:]:
                for j in range(prog.n_outputs):
                    _expect(j == net.component or torch.equal(slot[j], fill[j]), f"{tag}: {k} row {j} was written")
    _check_grads(net, got, want_adj, f"{tag} adjoint with inputs", floor("adj"))
    xg2, tg2, _ = inputs(False, True, True)
    _expect(torch.equal(xg2, xg) and torch.equal(tg2, tg), f"{tag}: input cotangents differ without a gradient table")
    parts = [E.jets_backward_inputs(prog, x[lo:hi], t[lo:hi], nt, nx, cot[:, lo:hi].contiguous(), None, True, True, **line) for lo, hi in chunks]
    _expect(torch.equal(torch.cat([p[0] for p in parts]), xg), f"{tag}: x_grad differs between one multi-chunk launch and per-chunk launches")
    _expect(torch.equal(torch.cat([p[1] for p in parts]), tg), f"{tag}: t_grad differs between one multi-chunk launch and per-chunk launches")
    if full:
        xg3, tg3, _ = inputs(False, True, False)
        _expect(tg3 is None and torch.equal(xg3, xg), f"{tag}: x_grad differs when it is the only output")
    if net.pde is None:
        return

    # (d) residual + loss + gradient at every index; the forward-only launch gives the same bits
    pd = pde_desc_from_spec(o["pde"])
    assert _lib.residual_unit_name(prog, pd, N) == "layer_major" and E.inverse_kernel_name(prog, pd, N) == "layer_major", tag
    assert lib.pinn_inverse_workspace_bytes(ctypes.byref(prog.desc), ctypes.byref(pd), N) == \
        lib.pinn_inverse_workspace_bytes(ctypes.byref(prog.desc), ctypes.byref(pd), CHUNK_POINTS) > 0, tag

    def check_loss_outputs(r, s, f, what):
        e = rel_l2(r.cpu(), o["r"][o["idx"]], label=f"{what} residual", tol=TOL)
        _seen("residual", e, what)
        print(f"{what}: residual {e:.2e}")
        _expect(e <= TOL, f"{what}: residual {e:.2e}")
        e = rel_err(float(s) / N, float(o["L"]), label=f"{what} loss", tol=TOL)
        _seen("loss", e, what)
        _expect(e <= TOL, f"{what}: loss {e:.2e}")
        _check_grads(net, f.result(), o["gL"], what, floor("gL"))

    def loss_grad():
        _poison_sized(prog, dev, ws_bytes, N, nt, nx)
        f = _Filled(prog, names_all, o["gL"], dev, net.seed + 7)
        r, s = E.residual_loss_grad(prog, pd, x, t, 1.0 / N, f.flat, want_residual=True)
        loss_grad.filled = f
        return r, s, f.flat
    r, s, _ = twice(loss_grad)
    check_loss_outputs(r, s, loss_grad.filled, f"{tag} loss")
    r0, s0 = E.residual_forward(prog, pd, x, t)
    _expect(torch.equal(r0, r), f"{tag}: residual_forward and residual_loss_grad differ")
    e = rel_err(float(s0) / N, float(o["L"]), label=f"{tag} forward loss", tol=TOL)
    _expect(e <= TOL, f"{tag}: forward loss {e:.2e}")
    parts = torch.cat([E.residual_forward(prog, pd, x[lo:hi], t[lo:hi])[0] for lo, hi in chunks])
    _expect(torch.equal(parts, r), f"{tag}: residuals differ between one multi-chunk launch and per-chunk launches")
    if not full:
        return

    # (e) coefficient sums: by value (residual_loss_grad(coef_grads=)) and read from the device (residual_loss_grad_inverse)
    if net.pde in COEFS:
        coefs = [pde_parameters()[k] for k in COEFS[net.pde]]
        for entry in ("coef", "inverse"):
            def coef_launch():
                _poison_sized(prog, dev, ws_bytes, N, nt, nx)
                f = _Filled(prog, names_all, o["gL"], dev, net.seed + 8)
                cg = torch.tensor([2.0 * c if c != 0.0 else 1.0 for c in o["dcoef"]] + [0.0] * (2 - len(coefs)), device=dev)
                coef_launch.fill, coef_launch.filled = cg.clone(), f
                if entry == "coef":
                    r, s = E.residual_loss_grad(prog, pd, x, t, 1.0 / N, f.flat, want_residual=True, coef_grads=cg)
                else:  # the descriptor's own coefficients are not read
                    junk = E.pde_desc(net.pde, 1, [123.0, 456.0], o["pde"].loss_function, o["pde"].huber_delta)
                    cv = torch.tensor(coefs + [0.0] * (4 - len(coefs)), device=dev)
                    r, s = E.residual_loss_grad_inverse(prog, junk, cv, x, t, 1.0 / N, f.flat, cg, want_residual=True)
                return r, s, f.flat, cg
            r1, s1, _, cg = twice(coef_launch)
            check_loss_outputs(r1, s1, coef_launch.filled, f"{tag} {entry}")
            for k, want in enumerate(o["dcoef"]):
                got_k = float(cg[k].double() - coef_launch.fill[k].double())
                e = rel_err(got_k, want, label=f"{tag} {entry} d loss / d {COEFS[net.pde][k]}", tol=COEF_TOL)
                _seen("coefficient sum", e, f"{tag} {entry} {COEFS[net.pde][k]}")
                print(f"{tag} {entry}: d loss / d {COEFS[net.pde][k]}: {e:.2e}")
                _expect(abs(got_k - want) <= COEF_TOL * abs(want) + COEF_ABS, f"{tag} {entry}: d loss / d {COEFS[net.pde][k]}: {got_k} vs {want}")

    # (f) the residual adjoint
    def res_backward():
        _poison_sized(prog, dev, ws_bytes, N, nt, nx)
        f = _Filled(prog, names_all, o["gR"], dev, net.seed + 9)
        E.residual_backward(prog, pd, x, t, o["rbar"].float().to(dev), f.flat)
        res_backward.filled = f
        return (f.flat,)
    twice(res_backward)
    _check_grads(net, res_backward.filled.result(), o["gR"], f"{tag} residual adjoint", floor("gR"))


@pytest.mark.parametrize("name,N,det", CASES, ids=lambda v: str(v))
def test_chunk_case(name, N, det, dev):
    if _GPU_ERROR:
        pytest.fail(f"not started: an earlier case met a GPU error: {_GPU_ERROR[0]}")
    del _MISSED[:]
    try:
        _run_case(networks()[name], N, det, dev)
        assert not _MISSED, f"{len(_MISSED)} checks missed:\n" + "\n".join(_MISSED)
    except AssertionError:
        raise
    except Exception as exc:  # a HIP error leaves the device in an unknown state: nothing further is launched on it
        _GPU_ERROR.append(f"{name} N={N}: {exc!r}"[:300])
        raise
    RAN.append((name, N, det))


def test_every_case_ran_and_the_widened_cap_holds():
    """Runs last (file order): every declared case ran, and the tensors on a widened bar stay below WIDENED_CAP of all compared
    tensors of this process."""
    n_w, n_c = len(TENSORS["widened"]), TENSORS["compared"]
    summary = {"policy": POLICY, "cases": len(RAN), "tensors_compared": n_c, "widened": TENSORS["widened"],
               "worst": {k: {"value": v, "where": w} for k, (v, w) in sorted(WORST.items())}}
    print(f"chunk-loop cases ({POLICY}): {len(RAN)} of {len(CASES)} ran; {n_w} of {n_c} tensors on a widened bar")
    for k, (v, w) in sorted(WORST.items()):
        print(f"worst {k}: {v:.2e} ({w})")
    try:  # next to the log of every measured error: what profiles/parity_lm_chunks.md is made from
        out_dir = os.path.dirname(_PARITY_LOG)
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, f"lm_chunks_{POLICY}.json"), "w") as fh:
            json.dump(summary, fh, indent=1)
    except OSError:
        pass
    assert sorted(RAN) == sorted(CASES), f"cases that did not run: {sorted(set(CASES) - set(RAN))}"
    assert n_c > 0 and n_w < WIDENED_CAP * n_c, TENSORS["widened"]
