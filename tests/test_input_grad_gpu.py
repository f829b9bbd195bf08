"""GPU: PINNModel outputs differentiable w.r.t. the input coordinates (pinn_jet_backward_inputs + JetFunction.backward),
against fp64 autograd through `oracle.network_forward` on the same state_dict.  Tolerance convention of
tests/test_hip_parity.py: relative L2 1e-5 (1e-4 for relu)."""

import pytest
import torch

import input_adjoint as IA
from conftest import rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


ARCHS = {
    "fourier_4x128": dict(architecture="fourier", hidden_dim=128, num_layers=4, mapping_size=32, scale=1.0, activation="tanh"),
    "ff_tanh_3x64": dict(architecture="feedforward", hidden_dim=64, num_layers=3, activation="tanh"),
    "ff_ln_tanh_3x64": dict(architecture="feedforward", hidden_dim=64, num_layers=3, activation="tanh", layer_norm=True),
    "siren_3x128": dict(architecture="siren", hidden_dim=128, num_layers=3, omega_0=3.0),
    "resnet_2x32": dict(architecture="resnet", hidden_dim=32, num_layers=2, num_blocks=2, activation="tanh"),
    "attention_2x32": dict(architecture="attention", hidden_dim=32, num_layers=2, num_heads=4, activation="tanh"),
    "ff_relu_3x64": dict(architecture="feedforward", hidden_dim=64, num_layers=3, activation="relu"),
}


def make(name, din, dev, seed=0):
    """(ArchSpec, fp32 state_dict on the CPU, PINNModel on the device with those weights)."""
    import oracle as O
    import pinnrl_amd  # noqa: F401
    from pinnrl_amd.config import Config, ModelConfig
    from pinnrl_amd.neural_networks import PINNModel

    spec = O.ArchSpec(input_dim=din, **ARCHS[name])
    sd = O.init_state_dict(spec, seed=seed)
    cfg = Config.__new__(Config)
    cfg.device = dev
    cfg.model = ModelConfig(input_dim=din, hidden_dim=spec.hidden_dim, output_dim=1, num_layers=spec.num_layers,
                            activation=spec.activation, architecture=spec.architecture, layer_norm=spec.layer_norm)
    cfg.model.mapping_size, cfg.model.scale = spec.mapping_size, spec.scale
    cfg.model.omega_0, cfg.model.num_heads = spec.omega_0, spec.num_heads
    if spec.num_blocks is not None:
        cfg.model.num_blocks = spec.num_blocks
    model = PINNModel(cfg, device=dev)
    model.load_state_dict({k: v.to(dev) for k, v in sd.items()})
    return spec, sd, model


def points(N, din, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(N, din - 1, generator=g) * 2 - 1, torch.rand(N, 1, generator=g)


def tol(name):
    return 1e-4 if "relu" in name else TOL


# ---- 1. first order through model(inp) --------------------------------------------------------------------------
@pytest.mark.parametrize("din", [2, 3])
@pytest.mark.parametrize("name", list(ARCHS))
def test_grad_of_model_output_wrt_input(name, din, dev):
    import oracle as O

    spec, sd, model = make(name, din, dev)
    x, t = points(1001, din)  # N not a multiple of 32
    w = torch.randn(x.shape[0], 1, generator=torch.Generator().manual_seed(2))
    inp = torch.cat([x, t], 1).to(dev).requires_grad_(True)
    (g,) = torch.autograd.grad((model(inp) * w.to(dev)).sum(), inp)
    inp64 = torch.cat([x, t], 1).double().requires_grad_(True)
    u64 = O.network_forward(spec, {k: v.double() for k, v in sd.items()}, inp64, layer_norm="composite")
    (g64,) = torch.autograd.grad((u64 * w.double()).sum(), inp64)
    assert rel_l2(g.cpu(), g64, label=f"{name} din={din} dinp", tol=tol(name)) <= tol(name)


# ---- 2. cotangents on every jet stream (mixed terms included) ---------------------------------------------------
@pytest.mark.parametrize("name", ["fourier_4x128", "ff_ln_tanh_3x64", "siren_3x128", "attention_2x32"])
def test_full_jet_cotangents(name, dev):
    spec, sd, model = make(name, 2, dev)
    x, t = points(777, 2)
    cot = torch.randn(4, x.shape[0], generator=torch.Generator().manual_seed(3))
    xd, td = x.to(dev).requires_grad_(True), t.to(dev).requires_grad_(True)
    J = model.jets(xd, td, 1, 2)
    gx, gt = torch.autograd.grad((J * cot.to(dev)).sum(), (xd, td))
    rx, rt = IA.input_grads_autograd(spec, sd, x, t, 1, 2, cot)
    assert rel_l2(gx.cpu(), rx, label=f"{name} xbar", tol=TOL) <= TOL
    assert rel_l2(gt.cpu(), rt, label=f"{name} tbar", tol=TOL) <= TOL


# ---- 3. reference-style residuals (autograd.grad(create_graph=True)) --------------------------------------------
def _g(y, v):
    return torch.autograd.grad(y, v, torch.ones_like(y), create_graph=True)[0]


def allen_cahn_residual(net, x, t, eps):  # allen_cahn.py:50-108, 1-D
    u = net(torch.cat([x, t], 1))
    u_t = _g(u, t)
    u_x = _g(u, x)
    u_xx = _g(u_x, x)
    return u_t - eps ** 2 * u_xx - u + u ** 3


def cahn_hilliard_residual(net, x, t, eps):  # cahn_hilliard.py:55-157, 1-D: mu = -eps^2 u_xx + c^3 - c, r = u_t - mu_xx
    u = net(torch.cat([x, t], 1))
    u_t = _g(u, t)
    u_x = _g(u, x)
    u_xx = _g(u_x, x)
    c = torch.clamp(u, -10.0, 10.0)
    mu = -eps ** 2 * u_xx + c ** 3 - c
    mu_x = _g(mu, x)
    mu_xx = _g(mu_x, x)
    return u_t - mu_xx


def _pde(kind, dev, eps):
    from pinnrl_amd import pdes as P

    cls = {"allen_cahn": P.AllenCahnEquation, "cahn_hilliard": P.CahnHilliardEquation}[kind]
    pc = P.PDEConfig(name=kind, domain=[(-1.0, 1.0)], time_domain=(0.0, 1.0), parameters={"epsilon": eps},
                     boundary_conditions={}, initial_condition={}, exact_solution={}, dimension=1, device=dev)
    return cls(pc)


@pytest.mark.parametrize("kind", ["allen_cahn", "cahn_hilliard"])
def test_reference_style_residual(kind, dev):
    import oracle as O

    eps = 0.3
    spec, sd, model = make("fourier_4x128", 2, dev)
    fn = allen_cahn_residual if kind == "allen_cahn" else cahn_hilliard_residual
    x, t = points(500, 2, seed=4)
    xd, td = x.to(dev).requires_grad_(True), t.to(dev).requires_grad_(True)
    r = fn(model, xd, td, eps)
    loss = (r ** 2).mean()
    model.zero_grad()
    loss.backward()
    got_w = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    # the product's fused residual and its weight gradient
    pde = _pde(kind, dev, eps)
    model.zero_grad()
    rf = pde.compute_residual(model, x.to(dev), t.to(dev))
    assert rel_l2(r.detach().cpu(), rf.detach().cpu(), label=f"{kind} residual vs fused", tol=TOL) <= TOL
    (rf ** 2).mean().backward()
    for k, p in model.named_parameters():
        assert rel_l2(got_w[k].cpu(), p.grad.cpu(), label=f"{kind} dW {k}", tol=TOL) <= TOL, k
    # x.grad against fp64 autograd through the oracle
    sd64 = {k: v.double() for k, v in sd.items()}
    x64, t64 = x.double().requires_grad_(True), t.double().requires_grad_(True)
    r64 = fn(lambda inp: O.network_forward(spec, sd64, inp), x64, t64, eps)
    assert rel_l2(r.detach().cpu(), r64.detach(), label=f"{kind} residual vs fp64", tol=TOL) <= TOL
    (r64 ** 2).mean().backward()
    assert rel_l2(xd.grad.cpu(), x64.grad, label=f"{kind} x.grad", tol=TOL) <= TOL
    assert rel_l2(td.grad.cpu(), t64.grad, label=f"{kind} t.grad", tol=TOL) <= TOL


def test_heat_periodic_derivative_pattern(dev):  # heat_equation.py:425-445: grad(u, points)[:, 0:1] at paired walls
    import oracle as O

    spec, sd, model = make("fourier_4x128", 2, dev)
    _, t = points(300, 2, seed=5)
    left = torch.cat([torch.full_like(t, -1.0), t], 1)
    right = torch.cat([torch.full_like(t, 1.0), t], 1)

    def diff(net, l, r):
        du = []
        for pts in (l, r):
            u = net(pts)
            du.append(torch.autograd.grad(u, pts, torch.ones_like(u), create_graph=True)[0][:, 0:1])
        return du[0] - du[1]

    l, r = left.to(dev).requires_grad_(True), right.to(dev).requires_grad_(True)
    d = diff(model, l, r)
    sd64 = {k: v.double() for k, v in sd.items()}
    l64, r64 = left.double().requires_grad_(True), right.double().requires_grad_(True)
    d64 = diff(lambda inp: O.network_forward(spec, sd64, inp), l64, r64)
    assert rel_l2(d.detach().cpu(), d64.detach(), label="heat du_dx_left - du_dx_right", tol=TOL) <= TOL
    (d ** 2).mean().backward()  # the periodic loss differentiates that slice again (pure x chain)
    (d64 ** 2).mean().backward()
    assert rel_l2(l.grad.cpu(), l64.grad, label="heat points.grad", tol=TOL) <= TOL


# ---- 4. mixed terms / beyond the compiled orders: exact values, loud errors ----------------------------------------
def test_mixed_and_out_of_range_derivatives(dev):
    spec, sd, model = make("ff_tanh_3x64", 2, dev)
    x, t = points(200, 2, seed=6)
    xd, td = x.to(dev).requires_grad_(True), t.to(dev).requires_grad_(True)
    u = model(torch.cat([xd, td], 1))
    u_t = _g(u, td)
    u_tx = _g(u_t, xd)
    sd64 = {k: v.double() for k, v in sd.items()}
    x64, t64 = IA.leaves(x, t)
    import oracle as O

    u64 = O.network_forward(spec, sd64, torch.cat([x64, t64], 1))
    u_tx64 = _g(_g(u64, t64), x64)
    assert rel_l2(u_tx.detach().cpu(), u_tx64.detach(), label="u_tx", tol=TOL) <= TOL
    assert float(u_tx.detach().abs().max()) > 0
    with pytest.raises(NotImplementedError, match="mixed"):
        torch.autograd.grad(u_tx.sum(), xd)
    u_tt = _g(u_t, td)
    u_ttt = _g(u_tt, td)  # time order 3: exact value from the kernel, not differentiable again
    u_ttt64 = _g(_g(_g(u64, t64), t64), t64)
    assert rel_l2(u_ttt.detach().cpu(), u_ttt64.detach(), label="u_ttt", tol=TOL) <= TOL
    with pytest.raises(NotImplementedError, match="t order 3"):
        torch.autograd.grad(u_ttt.sum(), td)


# ---- 5. bit-reproducible input cotangents ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fourier_4x128", "attention_2x32"])
def test_input_cotangents_bit_identical(name, dev):
    from pinnrl_amd import engine as E

    spec, sd, model = make(name, 3, dev)
    x, t = points(4097, 3, seed=7)
    x, t = x.to(dev), t.to(dev)
    cot = torch.randn(4, x.shape[0], generator=torch.Generator().manual_seed(8)).to(dev)
    prog = model.program()
    a = E.jets_backward_inputs(prog, x, t, 1, 2, cot, None, True, True)
    b = E.jets_backward_inputs(prog, x, t, 1, 2, cot, None, True, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    flat = E.new_flat_grad(prog, dev)
    c = E.jets_backward_inputs(prog, x, t, 1, 2, cot, flat, True, True)  # weight gradients in the same launch
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    ref = E.new_flat_grad(prog, dev)
    E.jets_backward(prog, x, t, 1, 2, cot, ref)
    assert rel_l2(flat.cpu(), ref.cpu(), label=f"{name} dW with inputs", tol=TOL) <= TOL


# ---- 6. compute_derivatives keeps treating the coordinates as constants -------------------------------------------
def test_compute_derivatives_still_detaches(dev):
    spec, sd, model = make("fourier_4x128", 2, dev)
    pde = _pde("allen_cahn", dev, 0.3)
    x, t = points(100, 2, seed=9)
    xd = x.to(dev).requires_grad_(True)
    d = pde.compute_derivatives(model, xd, t.to(dev), temporal_derivatives=[1], spatial_derivatives={1, 2})
    sum(v.sum() for v in d.values()).backward()
    assert xd.grad is None
