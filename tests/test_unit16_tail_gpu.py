"""GPU: the packed last round of the 16-point fused kernel (jet_kernel_u16.h; plan: pinn_unit_tail_plan).

With `grid` workgroups, R = N // (16 grid) full rounds and M = N - 16 grid R points left, the last round is G = ceil(M /
(4 grid)) four-point groups per workgroup: G = 1..3 runs as one packed round (a 16-column MFMA operand group holds
4 points x 4 streams), G = 4 as ordinary units.  Helpers and bars of tests/test_unit16_kernel_gpu.py: fourier 3x128 tanh,
Burgers, NaN-poisoned workspace, every launch checked to take `jet_kernel_u16`; 1e-5 against the fp64 oracle (1e-4 per
tensor), 2e-6 against the 32-point kernel, two launches bit-equal, forward-only residual bit-equal to the fused one.

Point counts: the smallest at which each packed form exists (see CASES).  With the contiguous assignment (workgroup b takes
the points first_tail + 4 G b .. + 4 G - 1 below N) N = 98 leaves workgroup 3 without a tail point (34 points left, 12 per
workgroup).

A unit that would need scratch with the packed round is built without it (pinn_build_info(): "nopack <unit> ..."); its last
round stays ordinary units.  The tanh units of stream set (1, 2), jet_u16_1_2_0 and jet_u16c_1_2_0, must carry the round
(asserted), and so must the sin unit jet_u16_1_2_1 of the family case below, so that the case cannot quietly stop running
the round (if a compiler change makes that unit fall back, pick a family whose unit carries the round)."""

import pytest
import torch

from conftest import rel_err, rel_l2
from test_unit16_kernel_gpu import AB_TOL, TENSOR_TOL, TOL, _loss_grad, _oracle_loss_grads, _setup, _spec, _tile32
from test_wide_variants_gpu import _check_grads, _pde_desc, _poison

pytestmark = pytest.mark.gpu

# N: (grid, R, G)
CASES = {
    3: (1, 0, 1),    # R = 0, G = 1, ragged
    20: (1, 1, 1),   # G = 1, full group
    24: (1, 1, 2),   # G = 2
    27: (1, 1, 3),   # G = 3, ragged
    29: (1, 1, 4),   # G = 4: ordinary unit, the boundary
    50: (2, 1, 3),   # G = 3, second workgroup half full
    70: (3, 1, 2),   # G = 2
    98: (4, 1, 3),   # G = 3, workgroup 3 has no tail point
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _plan_is(prog, n, want):
    from pinnrl_amd import _lib

    grid = _lib.kernel_for(prog, n, 1, 2, 1)["grid"]
    rounds, groups, first = _lib.u16_tail_plan(n, grid)
    assert (grid, rounds, groups) == want, f"N={n}: grid, R, G = {(grid, rounds, groups)}, expected {want}"
    assert first == 16 * grid * rounds


def test_headline_units_carry_the_packed_round():
    from pinnrl_amd import _lib

    info = _lib.build_info()
    assert "nopack jet_u16_1_2_0 " not in info and "nopack jet_u16c_1_2_0 " not in info, info
    assert "jet_u16_1_2_0:" not in info and "jet_u16c_1_2_0:" not in info, info


@pytest.mark.parametrize("n", sorted(CASES))
def test_packed_forms_against_oracle_and_tile32(n, dev):
    from pinnrl_amd import engine as E

    o, prog, names, pde = _setup(dev, "tanh", n, seed=41)
    _plan_is(prog, n, CASES[n])
    x, t = o["x"].to(dev), o["t"].to(dev)
    r, s, flat = _loss_grad(prog, dev, pde, x, t, n)
    assert rel_l2(r.cpu(), o["r"], label=f"N={n} residual", tol=TOL) <= TOL
    assert rel_err(float(s) / n, float(o["L"]), label=f"N={n} loss", tol=TOL) <= TOL
    _check_grads(prog, names, flat, o["gL"], f"N={n} loss", TOL, TENSOR_TOL)
    r2, s2, flat2 = _loss_grad(prog, dev, pde, x, t, n)
    assert torch.equal(flat, flat2) and torch.equal(s, s2) and torch.equal(r, r2), "two launches differ"
    r_f, _ = E.residual_forward(prog, _pde_desc(pde), x, t)
    assert torch.equal(r_f, r), "forward-only and fused residuals differ"
    _, s3, flat3 = _tile32(prog, lambda: _loss_grad(prog, dev, pde, x, t, n))
    assert rel_l2(flat.cpu(), flat3.cpu(), label=f"N={n} grad vs 32-point", tol=AB_TOL) <= AB_TOL
    assert rel_err(float(s), float(s3), label=f"N={n} loss vs 32-point", tol=AB_TOL) <= AB_TOL


@pytest.mark.parametrize("n,point", [(17, 16), (27, 26)])
def test_a_point_has_the_same_bits_in_a_packed_group_and_in_a_full_unit(n, point, dev):
    """The first n points of a 32-point batch: point `point` sits in a packed group of the N = n launch (17: G = 1, 27:
    G = 3) and in a full unit of the N = 32 launch.  Equal bits: the packed GEMM keeps the k-order of the unit's."""
    o, prog, names, pde = _setup(dev, "tanh", 32, seed=43, grads=False)
    from pinnrl_amd import _lib

    assert _lib.kernel_name(prog, n, 1, 2, 1) == "jet_kernel_u16"
    _plan_is(prog, 32, (1, 2, 0))
    _plan_is(prog, n, (1, 1, 1 if n == 17 else 3))
    x, t = o["x"].to(dev), o["t"].to(dev)
    r32, _, _ = _loss_grad(prog, dev, pde, x, t, 32)
    rn, _, _ = _loss_grad(prog, dev, pde, x[:n].contiguous(), t[:n].contiguous(), n)
    print(f"N={n} point {point}: packed {float(rn[point]):.9e} full unit {float(r32[point]):.9e}")
    assert torch.equal(rn[point], r32[point]), f"{float(rn[point])!r} != {float(r32[point])!r}"
    assert torch.equal(rn[:16], r32[:16]), "the full unit ahead of the packed round changed"


@pytest.mark.parametrize("loss", ["mae", "huber"])
def test_loss_kinds_on_a_packed_round(loss, dev):
    n = 27
    o, prog, names, pde = _setup(dev, "tanh", n, seed=45, loss=loss)
    x, t = o["x"].to(dev), o["t"].to(dev)
    _, L_want, g_want = _oracle_loss_grads((_spec("tanh"), o["sd"]), o["gL"].keys(), pde, o["x"], o["t"])
    _, s, flat = _loss_grad(prog, dev, pde, x, t, n)
    assert rel_err(float(s) / n, float(L_want), label=f"{loss} loss", tol=TOL) <= TOL
    _check_grads(prog, names, flat, g_want, f"{loss} loss", TOL, TENSOR_TOL)
    _, s3, flat3 = _tile32(prog, lambda: _loss_grad(prog, dev, pde, x, t, n))
    assert rel_l2(flat.cpu(), flat3.cpu(), label=f"{loss} grad vs 32-point", tol=AB_TOL) <= AB_TOL


@pytest.mark.parametrize("fam", ["tanh", "sin"])
def test_res_bar_and_jets_adjoint_on_a_packed_round(fam, dev):
    """residual_backward (res_bar) and jets_backward at N = 27; `sin` is the SIREN network: first Linear as the encoding,
    so the reverse sweep ends in the encoding backward."""
    from pinnrl_amd import engine as E

    from pinnrl_amd import _lib

    n = 27
    o, prog, names, pde = _setup(dev, fam, n, seed=47)
    unit = f"jet_u16_1_2_{_lib.ACT[fam]}"
    packed = f"nopack {unit} " not in _lib.build_info()
    print(f"{fam}: {unit} {'carries the packed round' if packed else 'was built without the packed round'}")
    assert packed, f"{unit} was built without the packed round: this case would run ordinary units"
    assert _lib.kernel_name(prog, n, 1, 2, 1) == "jet_kernel_u16"
    x, t = o["x"].to(dev), o["t"].to(dev)
    _poison(prog, dev, n, 1, 2)
    flat = E.new_flat_grad(prog, dev)
    E.residual_backward(prog, _pde_desc(pde), x, t, o["rbar"].float().to(dev), flat)
    _check_grads(prog, names, flat, o["gR"], f"{fam} residual adjoint", TOL, TENSOR_TOL)

    def jets():
        _poison(prog, dev, n, 1, 2)
        f = E.new_flat_grad(prog, dev)
        E.jets_backward(prog, x, t, 1, 2, o["cot"].float().to(dev), f)
        return f

    flat = jets()
    _check_grads(prog, names, flat, o["adj"], f"{fam} jets adjoint", TOL, TENSOR_TOL)
    flat3 = _tile32(prog, jets)
    assert rel_l2(flat.cpu(), flat3.cpu(), label=f"{fam} jets adjoint vs 32-point", tol=AB_TOL) <= AB_TOL
    r, s, flat = _loss_grad(prog, dev, pde, x, t, n)
    assert rel_l2(r.cpu(), o["r"], label=f"{fam} residual", tol=TOL) <= TOL
    _check_grads(prog, names, flat, o["gL"], f"{fam} loss", TOL, TENSOR_TOL)


def test_inverse_call_on_a_packed_round(dev):
    """jet_u16c_1_2_0 at N = 27 against the fp64 oracle, as tests/test_inverse_fused_gpu.py checks the inverse call."""
    import oracle as O
    from hip_helpers import program_from_spec
    from pinnrl_amd import engine as E

    import test_inverse_fused_gpu as I

    n = 27
    spec = _spec("tanh")
    sd = O.init_state_dict(spec, seed=49)
    x, t = I._points("burgers", n, 50)
    values = I.PDES["burgers"][1]
    want = I._oracle("burgers", spec, sd, x, t, values)
    prog, names_all = program_from_spec(spec, sd, dev)
    pd = I._pd("burgers")
    assert E.inverse_kernel_name(prog, pd, n) == "jet_kernel_u16"
    got = I._launch(prog, pd, I._coef_values(values, dev), x.to(dev), t.to(dev), 1.0 / n, dev)
    I._check("burgers fourier3x128 packed round", prog, names_all, got, want, n)
    got2 = I._launch(prog, pd, I._coef_values(values, dev), x.to(dev), t.to(dev), 1.0 / n, dev)
    assert all(torch.equal(a, b) for a, b in zip(got, got2)), "two launches differ"
