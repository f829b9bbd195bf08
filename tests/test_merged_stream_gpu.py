"""GPU: 1-D Burgers on the merged stream set (u, u_t - nu u_xx, u_x) of the 16-point fused kernel (jet_kernel_u16.h, MRG;
units jet_u16m_<family> and jet_u16mc_<family>).

Helpers and bars of the 16-point kernel's tests: 1e-5 against the fp64 oracle (1e-4 per tensor, relu 1e-4), 2e-6 against
the same build with PINN_FLAG_PLAIN_STREAMS (one stream per derivative).  `pinn_kernel_name` answers as before, so that a
call really takes the merged unit is shown by its residual: the flag changes bits of it.  Point counts: 1 (one unit, one
point), 17 (a full unit and a packed round of one group), 27 (three groups, ragged), 50 (two workgroups), 32 (two full
units, for the bit identity of a point in a packed group and in a unit).
"""

import math

import pytest
import torch

from conftest import rel_err, rel_l2
from test_unit16_images_gpu import MFMA_LAYERS, _routed_to_u16, _well_conditioned
from test_unit16_images_gpu import _spec as _images_spec
from test_unit16_kernel_gpu import AB_TOL, RELU_TOL, TENSOR_TOL, TOL, _loss_grad, _setup
from test_wide_variants_gpu import _check_grads, _oracle, _pde_desc, _poison

pytestmark = pytest.mark.gpu

FOURIER_NETS = ["fourier_1", "fourier_2", "fourier_3"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _plain(prog, fn):
    from pinnrl_amd import _lib

    prog.desc.flags |= _lib.PINN_FLAG_PLAIN_STREAMS
    try:
        return fn()
    finally:
        prog.desc.flags &= ~_lib.PINN_FLAG_PLAIN_STREAMS


def _merged_built(fam):
    from pinnrl_amd import _lib

    a, info = _lib.ACT[fam], _lib.build_info()
    return all(f"{u}_{a}:" not in info for u in ("jet_u16m", "jet_u16mc")) and all(f"{u}_1_2_{a}:" not in info for u in ("jet_u16", "jet_u16c"))


def test_headline_units_are_built_without_scratch_and_carry_the_packed_round():
    from pinnrl_amd import _lib

    info = _lib.build_info()
    for unit in ("jet_u16m_0", "jet_u16mc_0"):
        assert f"{unit}:" not in info and f"nopack {unit} " not in info, info


@pytest.mark.parametrize("n", [1, 17, 27, 50])
@pytest.mark.parametrize("net", FOURIER_NETS)
def test_oracle_parity_and_bit_identity(net, n, dev):
    from hip_helpers import program_from_spec
    from pinnrl_amd import engine as E

    spec = _images_spec(net)
    o = _well_conditioned(spec, 60 + MFMA_LAYERS[net], n)
    prog, names = program_from_spec(spec, o["sd"], dev)
    _routed_to_u16(prog, n)
    pde = o["pde"]
    x, t = o["x"].to(dev), o["t"].to(dev)
    r, s, flat = _loss_grad(prog, dev, pde, x, t, n)
    e_r = rel_l2(r.cpu(), o["r"], label=f"{net} N={n} residual", tol=TOL)
    e_l = rel_err(float(s) / n, float(o["L"]), label=f"{net} N={n} loss", tol=TOL)
    print(f"{net} N={n}: residual rel l2 {e_r:.2e}, loss rel err {e_l:.2e}")
    assert e_r <= TOL
    assert e_l <= TOL
    _check_grads(prog, names, flat, o["gL"], f"{net} N={n} loss", TOL, TENSOR_TOL)
    r2, s2, flat2 = _loss_grad(prog, dev, pde, x, t, n)
    assert torch.equal(flat, flat2) and torch.equal(s, s2) and torch.equal(r, r2), "two launches differ"
    r_f, _ = E.residual_forward(prog, _pde_desc(pde), x, t)
    assert torch.equal(r_f, r), "forward-only and fused residuals differ"
    # the inverse call of the same descriptor, nu from the device
    nu = float(torch.tensor(float(pde.parameters["nu"]), dtype=torch.float32))
    cv = torch.tensor([nu, 0.0, 0.0, 0.0], dtype=torch.float32, device=dev)
    pd_by_value = E.pde_desc("burgers", 1, (nu,))
    r_v, _ = E.residual_forward(prog, pd_by_value, x, t)
    cg = torch.zeros(4, dtype=torch.float32, device=dev)
    r_i, _ = E.residual_loss_grad_inverse(prog, E.pde_desc("burgers", 1, (-7.5e3, 1.0e9, float("nan"), -3.0)), cv, x, t, 1.0 / n,
                                          E.new_flat_grad(prog, dev), cg, want_residual=True)
    assert torch.equal(r_i, r_v), "forward-only and inverse-call residuals differ"
    assert torch.equal(r_i, r), "fused and inverse-call residuals differ"
    # the merged unit ran: one stream per derivative rounds differently (several points: at least one differs)
    r_p, s_p, flat_p = _plain(prog, lambda: _loss_grad(prog, dev, pde, x, t, n))
    assert rel_l2(r_p.cpu(), o["r"], label=f"{net} N={n} four-stream residual", tol=TOL) <= TOL
    if n > 1:
        assert not torch.equal(r_p, r), "the call did not take the merged unit"


@pytest.mark.parametrize("n,point", [(17, 16), (27, 26)])
def test_a_point_has_the_same_bits_in_a_packed_group_and_in_a_full_unit(n, point, dev):
    o, prog, names, pde = _setup(dev, "tanh", 32, seed=63, grads=False)
    x, t = o["x"].to(dev), o["t"].to(dev)
    r32, _, _ = _loss_grad(prog, dev, pde, x, t, 32)
    rn, _, _ = _loss_grad(prog, dev, pde, x[:n].contiguous(), t[:n].contiguous(), n)
    print(f"N={n} point {point}: packed {float(rn[point]):.9e} full unit {float(r32[point]):.9e}")
    assert torch.equal(rn[point], r32[point]), f"{float(rn[point])!r} != {float(r32[point])!r}"
    assert torch.equal(rn[:16], r32[:16]), "the full unit ahead of the packed round changed"
    r_p, _, _ = _plain(prog, lambda: _loss_grad(prog, dev, pde, x, t, 32))
    assert not torch.equal(r_p, r32), "the call did not take the merged unit"


@pytest.mark.parametrize("net,n,nu", [("fourier_3", 17, 0.02), ("fourier_3", 17, 0.01 / math.pi), ("fourier_3", 50, 0.02),
                                      ("fourier_3", 50, 0.01 / math.pi), ("linear_2", 27, 0.02)])
def test_inverse_call(net, n, nu, dev):
    """d loss / d nu (the sum of the coefficient partials) and the weight gradient of the merged COEF unit.  `linear_2`:
    a first Linear as the encoding, whose activation has a coefficient partial too and no Fourier term."""
    import oracle as O
    from hip_helpers import program_from_spec
    from pinnrl_amd import engine as E

    import test_inverse_fused_gpu as I

    spec = _images_spec(net)
    sd = O.init_state_dict(spec, seed=65)
    x, t = I._points("burgers", n, 66)
    L, dnu, _, gw = I._oracle("burgers", spec, sd, x, t, (nu,))
    prog, names_all = program_from_spec(spec, sd, dev)
    pd = I._pd("burgers")
    assert E.inverse_kernel_name(prog, pd, n) == "jet_kernel_u16"
    cv = I._coef_values((nu,), dev)
    s, cg, flat = I._launch(prog, pd, cv, x.to(dev), t.to(dev), 1.0 / n, dev)
    assert torch.isfinite(flat).all() and torch.isfinite(cg).all() and torch.isfinite(s).all()
    e_l = rel_err(float(s) / n, L, label=f"inverse N={n} loss", tol=TOL)
    e_c = abs(float(cg[0]) - dnu) / abs(dnu)
    by_name = {k: g for k, g in zip(names_all, E.split_flat_grad(prog, flat)) if g is not None}
    e_g = rel_l2(torch.cat([by_name[k].flatten().cpu() for k in gw]), torch.cat([gw[k].flatten() for k in gw]),
                 label=f"inverse N={n} weight gradient", tol=TOL)
    print(f"inverse {net} N={n} nu={nu:.4g}: loss {e_l:.2e}, d loss / d nu {float(cg[0])!r} vs {dnu!r} ({e_c:.2e}), gradient {e_g:.2e}")
    assert e_l <= TOL
    assert e_c <= TOL
    assert e_g <= TOL
    assert float(cg[1]) == 0.0 and float(cg[2]) == 0.0 and float(cg[3]) == 0.0
    got2 = I._launch(prog, pd, cv, x.to(dev), t.to(dev), 1.0 / n, dev)
    assert all(torch.equal(a, b) for a, b in zip((s, cg, flat), got2)), "two launches differ"


def test_res_bar_call(dev):
    from pinnrl_amd import engine as E

    n = 17
    o, prog, names, pde = _setup(dev, "tanh", n, seed=67)
    x, t = o["x"].to(dev), o["t"].to(dev)
    _poison(prog, dev, n, 1, 2)
    flat = E.new_flat_grad(prog, dev)
    E.residual_backward(prog, _pde_desc(pde), x, t, o["rbar"].float().to(dev), flat)
    _check_grads(prog, names, flat, o["gR"], "residual adjoint", TOL, TENSOR_TOL)


def test_merged_against_four_streams(dev):
    n = 50
    o, prog, names, pde = _setup(dev, "tanh", n, seed=69)
    x, t = o["x"].to(dev), o["t"].to(dev)
    _, s, flat = _loss_grad(prog, dev, pde, x, t, n)
    _, s4, flat4 = _plain(prog, lambda: _loss_grad(prog, dev, pde, x, t, n))
    assert rel_l2(flat.cpu(), flat4.cpu(), label="merged grad vs four streams", tol=AB_TOL) <= AB_TOL
    assert rel_err(float(s), float(s4), label="merged loss vs four streams", tol=AB_TOL) <= AB_TOL


@pytest.mark.parametrize("fam", ["sin", "gelu", "sigmoid", "relu"])
def test_other_families(fam, dev):
    """`sin` is the SIREN network (first Linear as the encoding: the reverse sweep ends in the encoding backward)."""
    from pinnrl_amd import _lib

    n = 27
    o, prog, names, pde = _setup(dev, fam, n, seed=71)
    x, t = o["x"].to(dev), o["t"].to(dev)
    tol = RELU_TOL if fam == "relu" else TOL
    r, s, flat = _loss_grad(prog, dev, pde, x, t, n)
    assert rel_l2(r.cpu(), o["r"], label=f"{fam} residual", tol=tol) <= tol
    assert rel_err(float(s) / n, float(o["L"]), label=f"{fam} loss", tol=tol) <= tol
    _check_grads(prog, names, flat, o["gL"], f"{fam} loss", tol, TENSOR_TOL)
    r_p, _, _ = _plain(prog, lambda: _loss_grad(prog, dev, pde, x, t, n))
    if _merged_built(fam):
        assert not torch.equal(r_p, r), f"{fam}: the call did not take the merged unit"
    else:
        print(f"{fam}: not routed, pinn_build_info() = {_lib.build_info()}")
        assert torch.equal(r_p, r)


@pytest.mark.parametrize("case", ["allen_cahn", "jets"])
def test_unrouted_kinds_ignore_the_flag(case, dev):
    """Allen-Cahn (1, 2) and a MODE_JETS (1, 2) call: bit-identical with and without PINN_FLAG_PLAIN_STREAMS."""
    from hip_helpers import program_from_spec
    from pinnrl_amd import engine as E

    n = 27
    spec = _images_spec("fourier_3")
    o = _oracle(spec, ("allen_cahn", 1), 73, n, False)
    prog, names = program_from_spec(spec, o["sd"], dev)
    _routed_to_u16(prog, n)
    x, t = o["x"].to(dev), o["t"].to(dev)
    if case == "allen_cahn":
        fn = lambda: _loss_grad(prog, dev, o["pde"], x, t, n)  # noqa: E731
    else:
        def fn():
            _poison(prog, dev, n, 1, 2)
            f = E.new_flat_grad(prog, dev)
            E.jets_backward(prog, x, t, 1, 2, o["cot"].float().to(dev), f)
            return (f.clone(),)
    a = fn()
    b = _plain(prog, fn)
    assert all(torch.equal(u, v) for u, v in zip(a, b)), f"{case}: the flag changed a call that is not routed"
