"""The cells of the PDE epilogue (`csrc/jet_device.h`: pde_residual, pde_coef_grads, loss_term), their fp64 reference and
the lanes (kernel families) every cell is run on.  Importable without a GPU; the routing helpers only query the library.

A cell is (kind, dimension).  `cahn_hilliard_clamped` is Cahn-Hilliard on a network whose output layer is rescaled so that
u leaves [-10, 10] on part of the points: the clamp mask of the residual is then 0 there.

The reference is the oracle (`oracle.compute_residual`, the restatement of the reference's residuals) in fp64 with the PDE
coefficients as live tensors, `oracle.apply_loss_fn` on top and ONE `torch.autograd.grad` call for d/d(theta) and d/d(c).
`heat_laplacian` (u_t - alpha u_xx) has no counterpart in the oracle and is built here from autograd derivatives of
`oracle.network_forward`.  `tests/jet_model.py` mirrors the kernels and is never the GPU reference.

Conditions that keep a comparison well-posed are asserted on the fp64 reference here (so they are checked on the CPU and
hold whatever the GPU computes); no point and no cell is ever left out of a comparison:
  mae     min |r| >= 1e-4 rms(r): no point sits where fp32 can flip sign(r); the positive and the negative residuals differ
          in number: where dr/du is a constant (Black-Scholes) the output bias's gradient is that constant times the sum
          of the signs, and with the signs balanced the fp64 reference would hold rounding dust where the exact value is 0;
  huber   delta = the fp64 median of |r| rounded to fp32; 30 .. 70 % of the points on the quadratic branch;
  clamp   >= 5 points with u > 10, >= 5 with u < -10, >= 5 inside, and min | |u| - 10 | >= 1e-3.
"""

import torch

N = 50  # one 32-point tile + an 18-point tail; three 16-point units + a 2-point tail (the packed round)
LOSSES = ("mse", "mae", "huber")

KINDS_1D = ("burgers", "heat", "heat_laplacian", "allen_cahn", "kdv", "cahn_hilliard", "cahn_hilliard_clamped", "wave",
            "convection", "black_scholes", "pendulum")
KINDS_ND = ("burgers", "heat", "heat_laplacian", "allen_cahn", "kdv", "cahn_hilliard", "wave", "black_scholes", "pendulum")
CELLS = [(k, 1) for k in KINDS_1D] + [(k, 2) for k in KINDS_ND]

# kind -> (oracle parameter names of coefficients 0 / 1, their values): deliberately not the defaults
COEF = {
    "burgers": (("nu",), (0.02,)),
    "heat": (("alpha",), (0.05,)),
    "heat_laplacian": (("alpha",), (0.05,)),
    "allen_cahn": (("epsilon",), (0.05,)),
    "kdv": ((), ()),
    "cahn_hilliard": (("epsilon",), (0.05,)),
    "wave": (("c",), (1.3,)),
    "convection": (("velocity",), (0.8,)),
    "black_scholes": (("sigma", "r"), (0.3, 0.07)),
    "pendulum": (("g",), (9.81 / 1.3,)),  # c0 = g / L, passed as g with L = 1
}
# (time order, space order) of the streams a residual reads: include/pinn_jet.h, pinn_pde_streams
STREAMS_1D = {"burgers": (1, 2), "heat": (1, 1), "heat_laplacian": (1, 2), "allen_cahn": (1, 2), "kdv": (1, 3),
              "cahn_hilliard": (1, 4), "wave": (2, 2), "convection": (1, 1), "black_scholes": (1, 2), "pendulum": (2, 0)}

CLAMP_SPAN = 14.0  # the clamped cell's u spans [-14, 14]

# lane -> network; "lm" and "wide64" share one network and so do the three 128-wide lanes: one reference serves them
LANES = ("lm", "wide64", "wide128", "u16", "u16_plain")
LANE_NET = {"lm": "ff64", "wide64": "ff64", "wide128": "fourier128", "u16": "fourier128", "u16_plain": "fourier128"}
NET_SEED = {"ff64": 4100, "fourier128": 4150}
# point seeds: 4200 + 10 * index of the cell + dimension unless listed here (chosen so that the conditions above hold on
# the fp64 reference; tests/test_pde_epilogue_cpu.py checks every one of them)
POINT_SEED = {("cahn_hilliard_clamped", 1): 5004, ("pendulum", 2): 5011, ("heat_laplacian", 1): 5006, ("allen_cahn", 2): 5007,
              ("black_scholes", 2): 5100}


def base_kind(kind):
    return "cahn_hilliard" if kind == "cahn_hilliard_clamped" else kind


def cell_id(kind, dim):
    return f"{kind}-{dim}d"


def streams(kind, dim):
    if dim > 1:
        return (2, 0) if base_kind(kind) in ("wave", "pendulum") else (1, 0)
    return STREAMS_1D[base_kind(kind)]


def branch(kind, dim):
    """The `case` of jet_device.h::pde_residual the cell runs."""
    k = base_kind(kind)
    if dim > 1:
        return f"nd_{k}" if k in ("wave", "pendulum", "allen_cahn", "black_scholes") else "nd_u_t"
    return kind  # the clamped cell is the m = 0 side of the Cahn-Hilliard case


BRANCHES = sorted({branch(k, d) for k, d in CELLS})


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def coef_values(kind):
    """(c0, c1) rounded to fp32, 0 where the kind has no such coefficient."""
    v = [f32(c) for c in COEF[base_kind(kind)][1]]
    return tuple(v + [0.0] * (2 - len(v)))


def spec_of(net, dim):
    import oracle as O

    if net == "ff64":
        return O.ArchSpec("feedforward", input_dim=dim + 1, hidden_dim=64, num_layers=3)
    if net == "fourier128":  # the network of tests/test_unit16_kernel_gpu.py::_spec("tanh")
        return O.ArchSpec("fourier", input_dim=dim + 1, hidden_dim=128, num_layers=3, mapping_size=32, scale=2.0, activation="tanh")
    raise KeyError(net)


def point_seed(kind, dim):
    return POINT_SEED.get((kind, dim), 4200 + 10 * (KINDS_1D.index(kind)) + dim)


def points(kind, dim, seed=None):
    """x in [-1, 1]^dim (Black-Scholes: [0, 2]^dim, so that x0 matters), t in [0, 1]; fp32."""
    g = torch.Generator().manual_seed(point_seed(kind, dim) if seed is None else seed)
    x = torch.rand(N, dim, generator=g) * 2.0 - (0.0 if base_kind(kind) == "black_scholes" else 1.0)
    t = torch.rand(N, 1, generator=g)
    return x, t


def _params(sd, dtype):
    return {k: v.to(dtype).clone().requires_grad_(not k.endswith("fourier.B")) for k, v in sd.items()}


def clamped_state_dict(spec, sd, x, t):
    """The same network with the output layer's weight and bias rescaled so that u spans [-CLAMP_SPAN, CLAMP_SPAN] on the
    points (in fp64; the result is rounded to fp32, which is what both sides then compute with)."""
    import oracle as O

    p = {k: v.double() for k, v in sd.items()}
    u = O.network_forward(spec, p, torch.cat([x, t], 1).double())
    lo, hi = float(u.min()), float(u.max())
    a = 2.0 * CLAMP_SPAN / (hi - lo)
    out = dict(sd)
    wk, bk = list(sd.keys())[-2:]
    out[wk] = (sd[wk].double() * a).float()
    out[bk] = ((sd[bk].double() - 0.5 * (hi + lo)) * a).float()
    return out


def network(kind, dim, net):
    """(spec, state_dict fp32, x, t) of a cell on a network."""
    import oracle as O

    spec = spec_of(net, dim)
    sd = O.init_state_dict(spec, seed=NET_SEED[net] + dim)
    x, t = points(kind, dim)
    if kind == "cahn_hilliard_clamped":
        sd = clamped_state_dict(spec, sd, x, t)
    return spec, sd, x, t


def _grad(y, wrt):
    return torch.autograd.grad(y, wrt, grad_outputs=torch.ones_like(y), create_graph=True, allow_unused=True)[0]


def residual_live(kind, dim, spec, params, live, x, t):
    """The residual (N, 1) with the coefficients `live` (tensors) inside it, in the dtype of x."""
    import oracle as O

    k = base_kind(kind)
    model = lambda z: O.network_forward(spec, params, z)  # noqa: E731
    x, t = x.clone(), t.clone()
    if k == "heat_laplacian":  # u_t - alpha u_xx; >= 2-D as every kind of the reference: a derivative w.r.t. a fresh slice of x vanishes
        x.requires_grad_(True)
        t.requires_grad_(True)
        u = model(torch.cat([x, t], 1))
        u_t = _grad(u, t)
        lap = torch.zeros_like(u)
        for c in range(dim):
            xc = x if dim == 1 else x[:, c:c + 1]
            u_x = _grad(u, xc)
            if u_x is not None:
                u_xx = _grad(u_x, xc)
                if u_xx is not None:
                    lap = lap + u_xx
        return u_t - live[0] * lap
    par = {"L": 1.0} if k == "pendulum" else {}
    for name, c in zip(COEF[k][0], live):
        par[name] = [c] if name == "velocity" else c
    dom = (0.0, 2.0) if k == "black_scholes" else (-1.0, 1.0)
    pde = O.PdeSpec(name=k, dimension=dim, domain=(dom,) * dim, time_domain=(0.0, 1.0), parameters=par)
    return O.compute_residual(pde, model, x, t)


def cotangent(kind, dim):
    """The fixed res_bar of a cell: random, rounded to fp32."""
    g = torch.Generator().manual_seed(point_seed(kind, dim) + 5)
    return torch.randn(N, 1, generator=g)


def evaluate(kind, dim, spec, sd, x, t, dtype=torch.float64, delta=None, check=True):
    """Everything the four calls are compared with, in `dtype`:
    {"r", "u", "delta", "rbar", "gR": {name: d<rbar, r>/dtheta}, loss: {"L", "dc": (dc0, dc1), "g": {name: dL/dtheta}}}."""
    import oracle as O

    params = _params(sd, dtype)
    names = [k for k, v in params.items() if v.requires_grad]
    live = [torch.tensor(c, dtype=dtype, requires_grad=True) for c in coef_values(kind)[: len(COEF[base_kind(kind)][1])]]
    xd, td = x.to(dtype), t.to(dtype)
    r = residual_live(kind, dim, spec, params, live, xd, td)
    u = O.network_forward(spec, params, torch.cat([xd, td], 1)).detach()
    rd = r.detach()
    if delta is None:
        delta = f32(float(rd.abs().median()))
    out = {"r": rd, "u": u, "delta": delta, "rbar": cotangent(kind, dim)}
    if check:
        conditions(kind, dim, rd, u, delta)
    wrt = live + [params[k] for k in names]

    def grads(scalar):
        g = torch.autograd.grad(scalar, wrt, allow_unused=True, retain_graph=True)
        g = [w.detach() if w is not None else torch.zeros_like(v) for w, v in zip(g, wrt)]
        dc = [float(v) for v in g[: len(live)]] + [0.0] * (2 - len(live))
        return (dc[0], dc[1]), dict(zip(names, g[len(live):]))

    _, out["gR"] = grads((r * out["rbar"].to(dtype)).sum())
    for loss in LOSSES:
        L = O.apply_loss_fn(r, loss, delta)
        dc, g = grads(L)
        out[loss] = {"L": float(L.detach()), "dc": dc, "g": g}
    return out


def condition_figures(kind, r, u, delta):
    r, u = r.double().flatten(), u.double().flatten()
    fig = {"mae_margin": float(r.abs().min() / r.pow(2).mean().sqrt()),
           "mae_sign_excess": int((r > 0).sum()) - int((r < 0).sum()),
           "huber_quadratic_share": float((r.abs() < delta).double().mean())}
    if kind == "cahn_hilliard_clamped":
        fig.update(above=int((u > 10).sum()), below=int((u < -10).sum()), inside=int((u.abs() <= 10).sum()),
                   clamp_margin=float((u.abs() - 10).abs().min()))
    return fig


def conditions(kind, dim, r, u, delta):
    """Asserted on the fp64 reference (module docstring)."""
    f = condition_figures(kind, r, u, delta)
    what = cell_id(kind, dim)
    assert torch.isfinite(r).all() and float(r.abs().max()) > 0, what
    assert f["mae_margin"] >= 1e-4, f"{what}: min |r| / rms(r) = {f['mae_margin']:.2e}"
    assert f["mae_sign_excess"] != 0, f"{what}: as many positive as negative residuals"
    assert 0.3 <= f["huber_quadratic_share"] <= 0.7, f"{what}: {f['huber_quadratic_share']:.2f} of the points on Huber's quadratic branch"
    if kind == "cahn_hilliard_clamped":
        assert f["above"] >= 5 and f["below"] >= 5 and f["inside"] >= 5 and f["clamp_margin"] >= 1e-3, f"{what}: {f}"
    return f


_REFERENCE = {}


def reference(kind, dim, net):
    """The fp64 reference of a cell on a network, computed once and shared (callers leave it unchanged)."""
    key = (kind, dim, net)
    if key not in _REFERENCE:
        spec, sd, x, t = network(kind, dim, net)
        ref = evaluate(kind, dim, spec, sd, x, t)
        ref.update(spec=spec, sd=sd, x=x, t=t)
        _REFERENCE[key] = ref
    return _REFERENCE[key]


def fp32_floor(kind, dim, net, which):
    """{name: gradient} of the same oracle evaluated in fp32 on the CPU (`hip_helpers.check_tensors`' floor); `which`: a loss
    kind or "gR"."""
    ref = reference(kind, dim, net)
    o = evaluate(kind, dim, ref["spec"], ref["sd"], ref["x"], ref["t"], dtype=torch.float32, delta=ref["delta"], check=False)
    return o["gR"] if which == "gR" else o[which]["g"]


# ----------------------------------------------------------------------------------------------------------------------
# lanes and routing (queries only: nothing is launched)
# ----------------------------------------------------------------------------------------------------------------------
def lane_cells(lane):
    if lane in ("lm", "wide64"):
        return list(CELLS)
    if lane == "u16_plain":  # the four-stream units where the merged ones run by default
        return [("burgers", 1)]
    return [(k, d) for k, d in CELLS if sum(streams(k, d)) <= 3]  # K <= 4: the sets (1,0), (1,1), (1,2), (2,0)


CASES = [(k, d, lane) for lane in LANES for k, d in lane_cells(lane)]


def apply_lane(prog, lane):
    from pinnrl_amd import _lib

    if lane == "lm":
        prog.set_layer_major(True)
    elif lane == "wide128":
        prog.desc.flags |= _lib.PINN_FLAG_WIDE_TILE32
    elif lane == "u16_plain":
        prog.desc.flags |= _lib.PINN_FLAG_PLAIN_STREAMS
    return prog


def descriptor(lane, dim):
    """Descriptor-only program of a lane: the queries read no tensor."""
    from pinnrl_amd import engine as E

    if LANE_NET[lane] == "ff64":
        prog = E.NetProgram("feedforward", "tanh", dim + 1, [64, 64, 64, 1], [], [])
    else:
        prog = E.NetProgram("fourier", "tanh", dim + 1, [128, 128, 1], [], [], mapping_size=32)
    return apply_lane(prog, lane)


def pde_desc(kind, dim, loss="mse", delta=1.0, coef=None):
    from pinnrl_amd import engine as E

    return E.pde_desc(base_kind(kind), dim, coef_values(kind) if coef is None else coef, loss, delta)


def route(prog, kind, dim):
    """What the queries say the calls of (program, cell) take: the forward-only and the reverse kernel, the translation unit
    family of the residual-mode calls and the kernel of the inverse call."""
    from pinnrl_amd import _lib
    from pinnrl_amd import engine as E

    pd = pde_desc(kind, dim)
    nt, nx = E.pde_streams(pd)
    assert (nt, nx) == streams(kind, dim)
    return {"forward": _lib.kernel_name(prog, N, nt, nx, 0), "reverse": _lib.kernel_name(prog, N, nt, nx, 1),
            "unit": _lib.residual_unit_name(prog, pd, N), "inverse": E.inverse_kernel_name(prog, pd, N)}


def family(name):
    if name == "layer_major":
        return "lm"
    if name == "jet_kernel_wide":
        return "wide"
    if name.startswith("jet_u16m"):
        return "u16m"
    assert name.startswith("jet_u16_") or name == "jet_kernel_u16", name
    return "u16"


# stream sets the tile-major families are compiled for (csrc/pinn_abi.hip: u16_set_compiled, widec_set_compiled, u16c_set_compiled;
# the 32-point kernel and the layer-major head have every set)
U16_SETS = {(1, 0), (1, 1), (1, 2), (2, 0)}
U16C_SETS = {(1, 1), (1, 2), (2, 0)}
WIDEC_SETS = {(1, 1), (1, 2), (1, 4), (2, 0), (2, 2)}


def claimed(lane, kind, dim):
    """(family of the residual-mode calls, family of the inverse call) a lane claims for a cell on a build in which every
    unit has its preferred form.  `pinn_inverse_kernel_name` does not tell the merged COEF units from the plain ones."""
    s = streams(kind, dim)
    if lane == "lm":
        return "lm", "lm"
    if lane in ("wide64", "wide128"):
        return "wide", "wide" if s in WIDEC_SETS else "lm"
    merged = lane == "u16" and (kind, dim) == ("burgers", 1)
    return "u16m" if merged else "u16", "u16" if s in U16C_SETS else "lm"


def table():
    """[(cell id, lane, unit, inverse kernel)] of every case, from the queries."""
    rows = []
    for kind, dim, lane in CASES:
        q = route(descriptor(lane, dim), kind, dim)
        rows.append((cell_id(kind, dim), lane, q["unit"], q["inverse"]))
    return rows
