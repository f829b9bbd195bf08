"""GPU: `pinn_residual_loss_grad_inverse` — inverse problems on the fused tile-major kernels.

The call reads the four PDE coefficients from a device array at launch time and returns, from the one launch, the loss
sum, the weight gradient and the gradient w.r.t. coefficients 0 and 1.  Checked here against fp64 autograd through the
oracle with the coefficients as live tensors (what the reference does, pinnrl/pdes/pde_base.py:246-279), at the bar
`tests/test_data_modes.py::test_fused_coefficient_gradients_match_the_oracle` holds the same quantities to (2e-5), on
the 16-point COEF unit (jet_u16c_*), the 32-point one (jet_widec_*) and the layer-major engine; additivity over a
partition of the batch (bars of tests/test_full_size_properties.py); device residency of the coefficients, also through a
captured graph; bit reproducibility.  `pde->coef` holds garbage in every call: the entry point must not read it.
The cached workspace is filled with NaN before every launch (as tests/test_wide_variants_gpu.py does), so that a slab slot
the launch does not write cannot pass for a stale value."""

import ctypes
import re

import pytest
import torch

from conftest import rel_err, rel_l2

pytestmark = pytest.mark.gpu

TOL = 2e-5
GARBAGE = (-7.5e3, 1.0e9, float("nan"), -3.0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


# kind -> (oracle parameter names of coefficients 0 / 1, values, spatial domain, time domain)
PDES = {
    "burgers": (("nu",), (0.02,), (-1.0, 1.0), (0.0, 1.0)),
    "heat": (("alpha",), (0.05,), (0.0, 1.0), (0.0, 1.0)),
    "allen_cahn": (("epsilon",), (0.05,), (-1.0, 1.0), (0.0, 1.0)),
    "wave": (("c",), (1.3,), (0.0, 1.0), (0.0, 1.0)),
    "cahn_hilliard": (("epsilon",), (0.05,), (0.0, 1.0), (0.0, 1.0)),
    "black_scholes": (("sigma", "r"), (0.2, 0.05), (0.0, 2.0), (0.0, 1.0)),
    "pendulum": (("g",), (9.81 / 1.3,), (0.0, 1.0), (0.0, 2.0)),  # c0 = g / L passed as a value: L = 1 in the oracle
}


def _arch(name):
    import oracle as O

    return {
        "fourier3x32": O.ArchSpec("fourier", hidden_dim=32, num_layers=3, mapping_size=16, scale=4.0),
        "fourier4x128": O.ArchSpec("fourier", hidden_dim=128, num_layers=4, mapping_size=32, scale=4.0),
        "ff4x128": O.ArchSpec("feedforward", hidden_dim=128, num_layers=4),
        "ffgelu3x64": O.ArchSpec("feedforward", hidden_dim=64, num_layers=3, activation="gelu"),
        "ff3x32": O.ArchSpec("feedforward", hidden_dim=32, num_layers=3),
        "siren3x32": O.ArchSpec("siren", hidden_dim=32, num_layers=3, omega_0=30.0),
    }[name]


def _points(kind, n, seed):
    _, _, dom, tdom = PDES[kind]
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 1, generator=g) * (dom[1] - dom[0]) + dom[0]
    t = torch.rand(n, 1, generator=g) * (tdom[1] - tdom[0]) + tdom[0]
    return x, t


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def _oracle(kind, spec, sd, x, t, values):
    """fp64: (mean of r^2, d/d c_0, d/d c_1, {name: d/d theta}) with the coefficients as live tensors."""
    import oracle as O

    names, _, dom, tdom = PDES[kind]
    live = [torch.tensor(_f32(v), dtype=torch.float64, requires_grad=True) for v in values]
    par = {"L": 1.0} if kind == "pendulum" else {}
    par.update({k: c for k, c in zip(names, live)})
    pde = O.PdeSpec(name=kind, domain=(dom,), time_domain=tdom, parameters=par)
    params = {k: v.double().clone().requires_grad_(not k.endswith("fourier.B")) for k, v in sd.items()}
    pn = [k for k in params if params[k].requires_grad]
    r = O.compute_residual(pde, lambda z: O.network_forward(spec, params, z, "composite"), x.double(), t.double())
    L = (r**2).mean()
    g = torch.autograd.grad(L, live + [params[k] for k in pn], allow_unused=True)
    g = [w.detach() if w is not None else torch.zeros_like(v) for w, v in zip(g, live + [params[k] for k in pn])]
    dc = [float(v) for v in g[: len(live)]] + [0.0] * (2 - len(live))
    return float(L.detach()), dc[0], dc[1], dict(zip(pn, g[len(live):]))


def _pd(kind):
    from pinnrl_amd import engine as E

    return E.pde_desc(kind, 1, GARBAGE)  # the entry point ignores pde->coef


def _coef_values(values, dev):
    v = list(values) + [0.0] * (4 - len(values))
    return torch.tensor(v, dtype=torch.float32, device=dev)


def _poison(prog, pd, dev, N):
    from pinnrl_amd import _lib
    from pinnrl_amd import engine as E

    nbytes = _lib.load().pinn_inverse_workspace_bytes(ctypes.byref(prog.desc), ctypes.byref(pd), N)
    if nbytes:
        E._workspace(dev, nbytes)
    for ws in E._workspaces.values():
        ws.view(torch.float32).fill_(float("nan"))


def _launch(prog, pd, cv, x, t, scale, dev, poison=True):
    """(loss sum, coefficient gradients (4,), flat weight gradient) of one call."""
    from pinnrl_amd import engine as E

    if poison:
        _poison(prog, pd, dev, x.shape[0])
    flat = E.new_flat_grad(prog, dev)
    cg = torch.zeros(4, dtype=torch.float32, device=dev)
    _, s = E.residual_loss_grad_inverse(prog, pd, cv, x, t, scale, flat, cg)
    return s, cg, flat


def _check(tag, prog, names_all, got, want, n):
    from pinnrl_amd import engine as E

    s, cg, flat = got
    L, dc0, dc1, gw = want
    assert torch.isfinite(flat).all() and torch.isfinite(cg).all() and torch.isfinite(s).all(), f"{tag}: non-finite result"
    e = rel_err(float(s) / n, L, label=f"{tag} loss", tol=TOL)
    print(f"{tag}: loss rel err {e:.2e}")
    assert e <= TOL, f"{tag}: loss {e:.2e}"
    for k, w in enumerate((dc0, dc1)):
        g = float(cg[k])
        print(f"{tag}: d loss / d c{k}: {g!r} vs {w!r}")
        assert abs(g - w) <= TOL * abs(w) + 1e-9, f"{tag}: d loss / d c{k}: {g} vs {w}"
    assert float(cg[2]) == 0.0 and float(cg[3]) == 0.0, f"{tag}: slots 2, 3 of coef_grads were written"
    by_name = {n_: g for n_, g in zip(names_all, E.split_flat_grad(prog, flat)) if g is not None}
    gt = torch.cat([by_name[k].flatten().cpu() for k in gw])
    wt = torch.cat([gw[k].flatten() for k in gw])
    e = rel_l2(gt, wt, label=f"{tag} weight gradient", tol=TOL)
    print(f"{tag}: weight gradient rel l2 {e:.2e}")
    assert e <= TOL, f"{tag}: weight gradient {e:.2e}"


def _u16_expected(nt, nx, fam):
    from pinnrl_amd import _lib

    return "jet_kernel_wide" if f"jet_u16c_{nt}_{nx}_{fam}:" in _lib.build_info() else "jet_kernel_u16"


CASES = [
    ("burgers", "fourier3x32", "jet_kernel_wide"),
    ("burgers", "fourier4x128", "u16"),            # the headline network: the 16-point COEF unit
    ("allen_cahn", "ff4x128", "jet_kernel_wide"),  # image height 128, first MFMA layer reads 128 features
    ("heat", "ffgelu3x64", "jet_kernel_wide"),
    ("wave", "ff3x32", "jet_kernel_wide"),
    ("cahn_hilliard", "ff3x32", "jet_kernel_wide"),
    ("black_scholes", "ff3x32", "jet_kernel_wide"),  # two coefficients
    ("pendulum", "siren3x32", "jet_kernel_wide"),
]


@pytest.mark.parametrize("layer_major", [False, True], ids=["default", "layer_major"])
@pytest.mark.parametrize("kind,arch,kernel", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_inverse_call_matches_the_fp64_oracle(kind, arch, kernel, layer_major, dev):
    import oracle as O
    from hip_helpers import program_from_spec
    from pinnrl_amd import engine as E

    spec = _arch(arch)
    sd = O.init_state_dict(spec, seed=81)
    x, t = _points(kind, 211, 82)
    values = PDES[kind][1]
    want = _oracle(kind, spec, sd, x, t, values)
    prog, names_all = program_from_spec(spec, sd, dev)
    prog.set_layer_major(layer_major)
    pd = _pd(kind)
    nt, nx = E.pde_streams(pd)
    if layer_major:
        kernel = "layer_major"
    elif kernel == "u16":
        kernel = _u16_expected(nt, nx, 0)
    assert E.inverse_kernel_name(prog, pd, 211) == kernel
    got = _launch(prog, pd, _coef_values(values, dev), x.to(dev), t.to(dev), 1.0 / 211, dev)
    _check(f"{kind} {arch} {kernel}", prog, names_all, got, want, 211)


def _fallen_back_units():
    from pinnrl_amd import _lib

    return sorted(set(re.findall(r"jet_(widec|u16c)_(\d)_(\d)_(\d):", _lib.build_info())))


KIND_OF_SET = {(1, 1): "heat", (1, 2): "burgers", (1, 4): "cahn_hilliard", (2, 0): "pendulum", (2, 2): "wave"}
FAMILY = {0: "tanh", 1: "sin", 2: "gelu", 3: "sigmoid", 4: "relu"}


def test_every_fallen_back_coef_unit_runs(dev):
    """A jet_widec_* unit built in the default MFMA form runs its reverse launch at width 64; the calls of a jet_u16c_* unit
    that is not routed to take the jet_widec_* unit of the same stream set and family (checked at width 128)."""
    import oracle as O
    from hip_helpers import program_from_spec
    from pinnrl_amd import engine as E

    units = _fallen_back_units()
    print("COEF units listed by pinn_build_info():", units)
    for which, nt, nx, fam in units:
        nt, nx, fam = int(nt), int(nx), int(fam)
        kind = KIND_OF_SET[(nt, nx)]
        act = FAMILY[fam]
        h = 64 if which == "widec" else 128
        if act == "sin":
            spec = O.ArchSpec("siren", hidden_dims=[64, h, h], num_layers=3, omega_0=4.0)
        else:
            spec = O.ArchSpec("fourier", hidden_dim=h, num_layers=3, mapping_size=16 if h == 64 else 32, scale=2.0, activation=act)
        sd = O.init_state_dict(spec, seed=300 + 10 * nt + nx + fam)
        x, t = _points(kind, 211, 301)
        values = PDES[kind][1]
        want = _oracle(kind, spec, sd, x, t, values)
        prog, names_all = program_from_spec(spec, sd, dev)
        pd = _pd(kind)
        assert E.inverse_kernel_name(prog, pd, 211) == "jet_kernel_wide", (which, nt, nx, fam)
        got = _launch(prog, pd, _coef_values(values, dev), x.to(dev), t.to(dev), 1.0 / 211, dev)
        if act == "relu":  # kinks: a pre-activation within fp32 rounding of 0 may take the other branch than fp64 (1e-4 bar
            # of tests/test_wide_variants_gpu.py); the unit must still run and give finite results
            assert torch.isfinite(got[2]).all() and torch.isfinite(got[1]).all()
            continue
        _check(f"fallback {which}_{nt}_{nx}_{fam}", prog, names_all, got, want, 211)


def _headline(dev, seed=91):
    import oracle as O
    from hip_helpers import program_from_spec

    spec = _arch("fourier4x128")
    sd = O.init_state_dict(spec, seed=seed)
    prog, names_all = program_from_spec(spec, sd, dev)
    return spec, sd, prog, names_all


@pytest.mark.parametrize("N", [17, 33, 4900, 49729])
def test_additivity_and_ragged_ends_on_the_headline_network(N, dev):
    """Several units per workgroup, ragged last unit: the call on N points equals the sum of the calls on a partition of
    them (bars of tests/test_full_size_properties.py: loss 2e-5, gradients 1e-4 — fp32 sums of the same terms in another
    order; the coefficient gradient is such a sum too)."""
    from pinnrl_amd import engine as E

    spec, sd, prog, names_all = _headline(dev)
    pd = _pd("burgers")
    assert E.inverse_kernel_name(prog, pd, N) == _u16_expected(1, 2, 0)
    x, t = _points("burgers", N, 92)
    x, t = x.to(dev), t.to(dev)
    cv = _coef_values((0.02,), dev)
    s, cg, flat = _launch(prog, pd, cv, x, t, 1.0 / N, dev)
    cut = N // 3 + 5
    sa, ca, fa = _launch(prog, pd, cv, x[:cut], t[:cut], 1.0 / N, dev)
    sb, cb, fb = _launch(prog, pd, cv, x[cut:], t[cut:], 1.0 / N, dev)
    print(f"N={N}: loss {float(s)!r} vs {float(sa) + float(sb)!r}; dnu {float(cg[0])!r} vs {float(ca[0]) + float(cb[0])!r}; "
          f"grad rel l2 {rel_l2((fa + fb).cpu(), flat.cpu()):.2e}")
    assert abs(float(sa) + float(sb) - float(s)) <= 2e-5 * abs(float(s))
    assert rel_l2((fa + fb).cpu(), flat.cpu()) <= 1e-4
    assert abs(float(ca[0]) + float(cb[0]) - float(cg[0])) <= 1e-4 * abs(float(cg[0]))
    assert float(cg[1]) == 0.0
    if N == 49729:  # a 256-point seeded sample of the batch against the fp64 oracle
        idx = torch.randperm(N, generator=torch.Generator().manual_seed(93))[:256]
        xs, ts = x[idx.to(dev)].contiguous(), t[idx.to(dev)].contiguous()
        want = _oracle("burgers", spec, sd, xs.cpu(), ts.cpu(), (0.02,))
        got = _launch(prog, pd, cv, xs, ts, 1.0 / 256, dev)
        _check("headline sample", prog, names_all, got, want, 256)


def test_coefficients_are_read_from_the_device_at_launch_time(dev):
    """Overwrite coef_values in place between two calls, and between capture and replay of a graph holding one call."""
    import oracle as O
    from pinnrl_amd import engine as E

    spec, sd, prog, names_all = _headline(dev, seed=95)
    pd = _pd("burgers")
    n = 211
    x, t = _points("burgers", n, 96)
    xd, td = x.to(dev), t.to(dev)
    cv = _coef_values((0.02,), dev)
    got = _launch(prog, pd, cv, xd, td, 1.0 / n, dev)
    _check("nu = 0.02", prog, names_all, got, _oracle("burgers", spec, sd, x, t, (0.02,)), n)
    cv[0] = 0.3
    got = _launch(prog, pd, cv, xd, td, 1.0 / n, dev)
    _check("nu = 0.3 in place", prog, names_all, got, _oracle("burgers", spec, sd, x, t, (0.3,)), n)

    # a captured call follows the buffer
    flat = E.new_flat_grad(prog, dev)
    cg = torch.zeros(4, dtype=torch.float32, device=dev)
    s = torch.zeros(1, dtype=torch.float32, device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):  # sizes the stream's workspace before the capture
        E.residual_loss_grad_inverse(prog, pd, cv, xd, td, 1.0 / n, flat, cg, loss_sum=s)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        E.residual_loss_grad_inverse(prog, pd, cv, xd, td, 1.0 / n, flat, cg, loss_sum=s)
    for nu in (0.07, 0.011):
        cv[0] = nu
        flat.zero_()
        cg.zero_()
        s.zero_()
        graph.replay()
        torch.cuda.synchronize(dev)
        _check(f"graph replay, nu = {nu}", prog, names_all, (s, cg, flat), _oracle("burgers", spec, sd, x, t, (nu,)), n)


def test_null_coefficient_array_is_refused(dev):
    from pinnrl_amd import _lib

    spec, sd, prog, names_all = _headline(dev)
    pd = _pd("burgers")
    lib = _lib.load()
    x, t = _points("burgers", 8, 1)
    x, t = x.to(dev), t.to(dev)
    flat = torch.zeros(prog.grad_layout()[1], device=dev)
    from pinnrl_amd import engine as E

    rc = lib.pinn_residual_loss_grad_inverse(ctypes.byref(prog.desc), prog._weight_ptrs(), prog.num_tensors, ctypes.byref(pd), None,
                                             x.data_ptr(), t.data_ptr(), 8, 1.0, None, None, E._grad_ptrs(prog, flat), None, None, 0,
                                             None)
    assert rc == -1, rc  # PINN_ERR_BAD_DESC
    assert b"coef_values" in lib.pinn_last_error()


@pytest.mark.parametrize("case", ["headline", "headline_tile32", "deep_deterministic", "layer_major_deterministic"])
def test_two_launches_give_identical_bits(case, dev):
    """Wherever the weight gradient is bit-reproducible (the store-flush class by default, everything under
    PINN_FLAG_DETERMINISTIC), so are the coefficient gradients."""
    import oracle as O
    from hip_helpers import program_from_spec
    from pinnrl_amd import _lib
    from pinnrl_amd import engine as E

    N = 16401
    if case.startswith("headline"):
        spec, sd, prog, _ = _headline(dev)
        if case == "headline_tile32":
            prog.desc.flags |= _lib.PINN_FLAG_WIDE_TILE32
    elif case == "deep_deterministic":  # four MFMA layers: per-tile flushes, the deterministic slab
        spec = O.ArchSpec("fourier", hidden_dim=64, num_layers=5, mapping_size=16, scale=2.0)
        prog, _ = program_from_spec(spec, O.init_state_dict(spec, seed=97), dev)
        prog.set_deterministic(True)
    else:
        spec = O.ArchSpec("resnet", hidden_dim=32, num_layers=2, num_blocks=2)
        prog, _ = program_from_spec(spec, O.init_state_dict(spec, seed=98), dev)
        prog.set_deterministic(True)
    pd = _pd("burgers")
    name = E.inverse_kernel_name(prog, pd, N)
    want = {"headline": _u16_expected(1, 2, 0), "headline_tile32": "jet_kernel_wide", "deep_deterministic": "jet_kernel_wide",
            "layer_major_deterministic": "layer_major"}[case]
    assert name == want
    x, t = _points("burgers", N, 99)
    x, t = x.to(dev), t.to(dev)
    cv = _coef_values((0.02,), dev)
    s1, c1, f1 = _launch(prog, pd, cv, x, t, 1.0 / N, dev)
    s2, c2, f2 = _launch(prog, pd, cv, x, t, 1.0 / N, dev)
    assert torch.isfinite(f1).all() and float(c1[0]) != 0.0
    assert torch.equal(c1, c2), f"{case}: coefficient gradients differ: {c1.tolist()} vs {c2.tolist()}"
    assert torch.equal(f1, f2), f"{case}: weight gradients differ"
    assert torch.equal(s1, s2)
