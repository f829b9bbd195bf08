"""GPU: the 16-point fused reverse kernel (jet_kernel_u16.h) against the fp64 oracle and against the 32-point kernel.

Every launch here is checked to take `jet_kernel_u16` (`pinn_kernel_name`); the comparison launches set
PINN_FLAG_WIDE_TILE32 and take `jet_kernel_wide`.  Point counts cover empty lanes of a unit (1, 15, 17, 31, 33), a
whole unit (16), a grid below the CU count (4 900: 154 workgroups) and the benchmark's 49 729 points.  The workspace is
filled with NaN before every reverse launch, so that a slab entry the store flush does not write cannot pass."""

import math

import pytest
import torch

from conftest import rel_err, rel_l2
from test_wide_variants_gpu import _check_grads, _oracle, _pde_desc, _poison

pytestmark = pytest.mark.gpu

TOL = 1e-5
RELU_TOL = 1e-4  # relu kinks, as in test_wide_variants_gpu
TENSOR_TOL = 1e-4
AB_TOL = 2e-6  # relative L2 against the 32-point kernel


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _spec(fam, loss="mse"):
    import oracle as O

    if fam == "sin":
        return O.ArchSpec("siren", hidden_dims=[64, 128, 128], num_layers=3, omega_0=4.0)
    return O.ArchSpec("fourier", hidden_dim=128, num_layers=3, mapping_size=32, scale=2.0, activation=fam)



def _setup(dev, fam, n, seed, loss="mse", grads=True):
    import oracle as O
    from hip_helpers import program_from_spec
    from pinnrl_amd import _lib

    spec = _spec(fam)
    o = _oracle(spec, ("burgers", 1), seed, n, grads)
    prog, names = program_from_spec(spec, o["sd"], dev)
    # a unit that needs scratch is listed in pinn_build_info() and keeps the 32-point kernel
    built = f"jet_u16_1_2_{_lib.ACT[fam]}:" not in _lib.build_info()
    assert _lib.kernel_name(prog, n, 1, 2, 1) == ("jet_kernel_u16" if built or fam != "gelu" else "jet_kernel_wide")
    pde = o["pde"]
    if loss != "mse":
        pde = O.PdeSpec(name=pde.name, dimension=pde.dimension, domain=pde.domain, parameters=dict(pde.parameters),
                        loss_function=loss, huber_delta=0.05)
    return o, prog, names, pde


def _loss_grad(prog, dev, pde, x, t, n):
    from pinnrl_amd import engine as E

    _poison(prog, dev, n, 1, 2)
    flat = E.new_flat_grad(prog, dev)
    r, s = E.residual_loss_grad(prog, _pde_desc(pde), x, t, 1.0 / n, flat, want_residual=True)
    torch.cuda.synchronize()
    return r.clone(), s.clone(), flat.clone()


def _tile32(prog, fn):
    from pinnrl_amd import _lib

    prog.desc.flags |= _lib.PINN_FLAG_WIDE_TILE32
    try:
        return fn()
    finally:
        prog.desc.flags &= ~_lib.PINN_FLAG_WIDE_TILE32


def _oracle_loss_grads(spec_sd, names, pde, x, t):
    """fp64 loss and gradient of mean l(r) for a loss kind other than the cached mse."""
    import oracle as O

    from test_wide_variants_gpu import _grads, _params64

    spec, sd = spec_sd
    params = _params64(sd)
    r = O.compute_residual(pde, lambda inp: O.network_forward(spec, params, inp), x.double(), t.double())
    L = O.apply_loss_fn(r, pde.loss_function, pde.huber_delta)
    return r.detach(), L.detach(), _grads(L, params, [k for k in names if k in params and params[k].requires_grad])


@pytest.mark.parametrize("n", [1, 15, 16, 17, 31, 33, 4_900])
def test_points_against_oracle_and_tile32(n, dev):
    """Loss, residual and loss gradient: <= 1e-5 against fp64, <= 2e-6 against the 32-point kernel, bitwise repeatable."""
    o, prog, names, pde = _setup(dev, "tanh", n, seed=11)
    x, t = o["x"].to(dev), o["t"].to(dev)
    r, s, flat = _loss_grad(prog, dev, pde, x, t, n)
    assert rel_l2(r.cpu(), o["r"], label=f"N={n} residual", tol=TOL) <= TOL
    assert rel_err(float(s) / n, float(o["L"]), label=f"N={n} loss", tol=TOL) <= TOL
    _check_grads(prog, names, flat, o["gL"], f"N={n} loss", TOL, TENSOR_TOL)
    r2, s2, flat2 = _loss_grad(prog, dev, pde, x, t, n)
    assert torch.equal(flat, flat2) and torch.equal(s, s2) and torch.equal(r, r2), "two launches differ"
    from pinnrl_amd import engine as E

    r_f, _ = E.residual_forward(prog, _pde_desc(pde), x, t)  # the forward-only launch runs the same forward code
    assert torch.equal(r_f, r), "forward-only and fused residuals differ"
    r3, s3, flat3 = _tile32(prog, lambda: _loss_grad(prog, dev, pde, x, t, n))
    assert rel_l2(flat.cpu(), flat3.cpu(), label=f"N={n} grad vs 32-point", tol=AB_TOL) <= AB_TOL
    assert rel_err(float(s), float(s3), label=f"N={n} loss vs 32-point", tol=AB_TOL) <= AB_TOL


def test_benchmark_size_against_tile32(dev):
    """49 729 points (the benchmark's count): the 32-point kernel's gradient and loss to 2e-6, bitwise repeatable."""
    from hip_helpers import program_from_spec

    import oracle as O

    n = 49_729
    spec = _spec("tanh")
    sd = O.init_state_dict(spec, seed=5)
    prog, _ = program_from_spec(spec, sd, dev)
    from pinnrl_amd import _lib

    assert _lib.kernel_name(prog, n, 1, 2, 1) == "jet_kernel_u16"
    g = torch.Generator().manual_seed(6)
    x = (torch.rand(n, 1, generator=g) * 2 - 1).to(dev)
    t = torch.rand(n, 1, generator=g).to(dev)
    pde = O.PdeSpec(name="burgers", dimension=1, domain=((-1.0, 1.0),), parameters={"nu": 0.01 / math.pi})
    _, s, flat = _loss_grad(prog, dev, pde, x, t, n)
    _, s2, flat2 = _loss_grad(prog, dev, pde, x, t, n)
    assert torch.equal(flat, flat2) and torch.equal(s, s2)
    assert torch.isfinite(flat).all()
    _, s3, flat3 = _tile32(prog, lambda: _loss_grad(prog, dev, pde, x, t, n))
    assert rel_l2(flat.cpu(), flat3.cpu(), label="49729 grad vs 32-point", tol=AB_TOL) <= AB_TOL
    assert rel_err(float(s), float(s3), label="49729 loss vs 32-point", tol=AB_TOL) <= AB_TOL


@pytest.mark.parametrize("loss", ["mae", "huber"])
def test_loss_kinds(loss, dev):
    n = 33
    o, prog, names, pde = _setup(dev, "tanh", n, seed=21, loss=loss)
    x, t = o["x"].to(dev), o["t"].to(dev)
    r_want, L_want, g_want = _oracle_loss_grads((_spec("tanh"), o["sd"]), o["gL"].keys(), pde, o["x"], o["t"])
    r, s, flat = _loss_grad(prog, dev, pde, x, t, n)
    assert rel_err(float(s) / n, float(L_want), label=f"{loss} loss", tol=TOL) <= TOL
    _check_grads(prog, names, flat, g_want, f"{loss} loss", TOL, TENSOR_TOL)
    _, s3, flat3 = _tile32(prog, lambda: _loss_grad(prog, dev, pde, x, t, n))
    assert rel_l2(flat.cpu(), flat3.cpu(), label=f"{loss} grad vs 32-point", tol=AB_TOL) <= AB_TOL


@pytest.mark.parametrize("fam", ["tanh", "sin", "gelu", "sigmoid", "relu"])
def test_families_res_bar_and_jets_adjoint(fam, dev):
    """Every routed activation family: the residual adjoint (res_bar) and the jets-mode reverse sweep."""
    from pinnrl_amd import engine as E

    n = 100
    o, prog, names, pde = _setup(dev, fam, n, seed=31)
    x, t = o["x"].to(dev), o["t"].to(dev)
    tol = RELU_TOL if fam == "relu" else TOL
    _poison(prog, dev, n, 1, 2)
    flat = E.new_flat_grad(prog, dev)
    E.residual_backward(prog, _pde_desc(pde), x, t, o["rbar"].float().to(dev), flat)
    _check_grads(prog, names, flat, o["gR"], f"{fam} residual adjoint", tol, TENSOR_TOL)
    _poison(prog, dev, n, 1, 2)
    flat = E.new_flat_grad(prog, dev)
    E.jets_backward(prog, x, t, 1, 2, o["cot"].float().to(dev), flat)
    _check_grads(prog, names, flat, o["adj"], f"{fam} jets adjoint", tol, TENSOR_TOL)

    def ab():
        _poison(prog, dev, n, 1, 2)
        f = E.new_flat_grad(prog, dev)
        E.jets_backward(prog, x, t, 1, 2, o["cot"].float().to(dev), f)
        return f

    flat3 = _tile32(prog, ab)
    assert rel_l2(flat.cpu(), flat3.cpu(), label=f"{fam} jets adjoint vs 32-point", tol=AB_TOL) <= AB_TOL
