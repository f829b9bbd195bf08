"""GPU: the fixed-shape merged units of the 16-point fused kernel (jet_u16mf_<family>, jet_u16mfc_<family>;
jet_kernel_u16.h, FIXED).  They compile the default network's shape in (64 Fourier features of two
coordinates, three MFMA layers 64 -> 128 -> 128 -> 128, head 128 -> 1: `fourier_3` below) and must give the bits of the
generic merged units, which the same descriptor takes with PINN_FLAG_GENERIC_UNITS.

Sizes, as in test_merged_wave0_gpu.py: 1 point (the packed round alone), 17 (a unit and a one-point round), 32 (one
workgroup, two units), 96 (three workgroups), and three full units per workgroup followed by a ragged packed round.
Bars of the merged units' tests: 1e-5 against the fp64 oracle (1e-4 per tensor, relu 1e-4), 2e-6 against the four-stream
units; against the generic merged units every comparison is `torch.equal`.

Networks that miss the shape (hidden width 64, two MFMA layers, 32 Fourier features, a first Linear as the encoding) keep
the generic units: the flag changes nothing for them and their results stay within the bars.

Equal bits cannot show which of the two units ran, so every case also asks `pinn_residual_unit_name`, the query that
makes the launch's routing decision in the launch's own helpers: `jet_u16mf_<family>` for the headline shape,
`jet_u16m_<family>` with the flag, and no fixed unit for a near miss.
"""

import pytest
import torch

from conftest import rel_err, rel_l2
from test_merged_keep_gpu import SEED, _three_units_and_a_ragged_round
from test_merged_stream_gpu import _plain
from test_merged_wave0_gpu import _check_biases, _hidden_biases
from test_unit16_images_gpu import _routed_to_u16, _well_conditioned
from test_unit16_images_gpu import _spec as _images_spec
from test_unit16_kernel_gpu import AB_TOL, RELU_TOL, TENSOR_TOL, TOL, _loss_grad
from test_wide_variants_gpu import _check_grads, _oracle, _pde_desc

pytestmark = pytest.mark.gpu

NET = "fourier_3"  # the shape the fixed units are compiled for


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _generic(prog, fn):
    from pinnrl_amd import _lib

    prog.desc.flags |= _lib.PINN_FLAG_GENERIC_UNITS
    try:
        return fn()
    finally:
        prog.desc.flags &= ~_lib.PINN_FLAG_GENERIC_UNITS


def _unit(prog, pde, n):
    from pinnrl_amd import _lib

    return _lib.residual_unit_name(prog, _pde_desc(pde), n)


def _takes_the_fixed_unit(prog, pde, n, fam="tanh"):
    """The descriptor's residual-mode calls take jet_u16mf_<family>, and jet_u16m_<family> with the flag."""
    from pinnrl_amd import _lib

    a = _lib.ACT[fam]
    assert _unit(prog, pde, n) == f"jet_u16mf_{a}", _unit(prog, pde, n)
    assert _generic(prog, lambda: _unit(prog, pde, n)) == f"jet_u16m_{a}"


def _inverse_launch(prog, pd, cv, xd, td, n, dev):
    from pinnrl_amd import engine as E

    import test_inverse_fused_gpu as I

    I._poison(prog, pd, dev, n)
    flat = E.new_flat_grad(prog, dev)
    cg = torch.zeros(4, dtype=torch.float32, device=dev)
    r, s = E.residual_loss_grad_inverse(prog, pd, cv, xd, td, 1.0 / n, flat, cg, want_residual=True)
    torch.cuda.synchronize()
    return r.clone(), s.clone(), cg.clone(), flat.clone()


def _same_bits(got, want, names, prog, spec, what):
    """(residual, loss sum, flat gradient) of the fixed and the generic unit: every tensor, and the bias vectors by name."""
    from pinnrl_amd import engine as E

    r, s, flat = got
    r_g, s_g, flat_g = want
    assert torch.equal(s, s_g), f"{what}: loss sum {float(s)!r} != {float(s_g)!r}"
    assert torch.equal(r, r_g), f"{what}: {int((r != r_g).sum())} residuals differ"
    by, by_g = (dict(zip(names, E.split_flat_grad(prog, f))) for f in (flat, flat_g))
    for k in _hidden_biases(names, spec):
        assert torch.equal(by[k], by_g[k]), f"{what}: bias gradient {k} differs"
    assert torch.equal(flat, flat_g), f"{what}: {int((flat != flat_g).sum())} gradient entries differ"


def test_build_lists_no_fixed_unit():
    from pinnrl_amd import _lib

    info = _lib.build_info()
    assert "jet_u16mf" not in info, info  # (jet_u16mfc_* too: neither scratch, nor the default MFMA form, nor "nopack")


@pytest.mark.parametrize("n", [1, 17, 32, 96])
def test_small_sizes(n, dev):
    from hip_helpers import program_from_spec
    from pinnrl_amd import _lib
    from pinnrl_amd import engine as E

    spec = _images_spec(NET)
    o = _well_conditioned(spec, SEED[NET] + 130, n) if n == 1 else _oracle(spec, ("burgers", 1), SEED[NET] + 130, n, True)
    prog, names = program_from_spec(spec, o["sd"], dev)
    _routed_to_u16(prog, n)
    grid = _lib.kernel_for(prog, n, 1, 2, 1)["grid"]
    plan = _lib.u16_tail_plan(n, grid)[:2]
    assert (grid, plan) == {1: (1, (0, 1)), 17: (1, (1, 1)), 32: (1, (2, 0)), 96: (3, (2, 0))}[n], (grid, plan)
    pde = o["pde"]
    _takes_the_fixed_unit(prog, pde, n)
    x, t = o["x"].to(dev), o["t"].to(dev)
    r, s, flat = _loss_grad(prog, dev, pde, x, t, n)
    e_r = rel_l2(r.cpu(), o["r"], label=f"N={n} residual", tol=TOL)
    e_l = rel_err(float(s) / n, float(o["L"]), label=f"N={n} loss", tol=TOL)
    print(f"N={n}: residual rel l2 {e_r:.2e}, loss rel err {e_l:.2e}")
    assert e_r <= TOL
    assert e_l <= TOL
    _check_grads(prog, names, flat, o["gL"], f"N={n} loss", TOL, TENSOR_TOL)
    _check_biases(prog, names, flat, o["gL"], spec, f"N={n}")
    _same_bits((r, s, flat), _generic(prog, lambda: _loss_grad(prog, dev, pde, x, t, n)), names, prog, spec, f"N={n}")
    r_f, _ = E.residual_forward(prog, _pde_desc(pde), x, t)
    assert torch.equal(r_f, r), "forward-only and fused residuals differ"
    r_fg, _ = _generic(prog, lambda: E.residual_forward(prog, _pde_desc(pde), x, t))
    assert torch.equal(r_fg, r), "forward-only residuals of the generic unit differ"
    r2, s2, flat2 = _loss_grad(prog, dev, pde, x, t, n)
    assert torch.equal(flat, flat2) and torch.equal(s, s2) and torch.equal(r, r2), "two launches differ"
    if n > 1:
        r_p, _, _ = _plain(prog, lambda: _loss_grad(prog, dev, pde, x, t, n))
        assert not torch.equal(r_p, r), "the call did not take a merged unit"


def test_three_units_then_a_ragged_packed_round(dev):
    import oracle as O
    from hip_helpers import program_from_spec
    from pinnrl_amd import _lib
    from pinnrl_amd import engine as E
    from test_inverse_fused_gpu import _points

    n, g = _three_units_and_a_ragged_round(dev)
    spec = _images_spec(NET)
    sd = O.init_state_dict(spec, seed=SEED[NET] + 140)
    x, t = (v.to(dev) for v in _points("burgers", n, SEED[NET] + 141))
    prog, names = program_from_spec(spec, sd, dev)
    _routed_to_u16(prog, n)
    assert _lib.kernel_for(prog, n, 1, 2, 1)["grid"] == g
    pde = O.PdeSpec(name="burgers", parameters={"nu": 0.02})
    _takes_the_fixed_unit(prog, pde, n)
    r, s, flat = _loss_grad(prog, dev, pde, x, t, n)
    assert torch.isfinite(flat).all() and torch.isfinite(s).all() and torch.isfinite(r).all()
    _same_bits((r, s, flat), _generic(prog, lambda: _loss_grad(prog, dev, pde, x, t, n)), names, prog, spec, f"N={n}")
    r4, s4, flat4 = _plain(prog, lambda: _loss_grad(prog, dev, pde, x, t, n))
    assert not torch.equal(r4, r), "the call did not take a merged unit"
    e_g = rel_l2(flat.cpu(), flat4.cpu(), label=f"N={n} fixed-shape grad vs four streams", tol=AB_TOL)
    e_l = rel_err(float(s), float(s4), label=f"N={n} fixed-shape loss vs four streams", tol=AB_TOL)
    e_p = float((r - r4).abs().max() / r4.abs().max())  # (bar: test_merged_wave0_gpu.py)
    print(f"N={n}: gradient rel l2 {e_g:.2e}, loss rel err {e_l:.2e}, residual max point error {e_p:.2e} against the four-stream unit")
    assert e_g <= AB_TOL
    assert e_l <= AB_TOL
    assert e_p <= 2 * TOL
    r_f, _ = E.residual_forward(prog, _pde_desc(pde), x, t)
    assert torch.equal(r_f, r), "forward-only and fused residuals differ"
    r2, s2, flat2 = _loss_grad(prog, dev, pde, x, t, n)
    assert torch.equal(flat, flat2) and torch.equal(s, s2) and torch.equal(r, r2), "two launches differ"


@pytest.mark.parametrize("size", ["two_units", "ragged"])
def test_inverse_call(size, dev):
    """jet_u16mfc_<family> against jet_u16mc_<family>, bit for bit; at 32 points against the fp64 oracle too."""
    import oracle as O
    from hip_helpers import program_from_spec
    from pinnrl_amd import engine as E

    import test_inverse_fused_gpu as I

    n = 32 if size == "two_units" else _three_units_and_a_ragged_round(dev)[0]
    nu = 0.02
    spec = _images_spec(NET)
    sd = O.init_state_dict(spec, seed=SEED[NET] + 150)
    x, t = I._points("burgers", n, SEED[NET] + 151)
    prog, names = program_from_spec(spec, sd, dev)
    pd = I._pd("burgers")
    assert E.inverse_kernel_name(prog, pd, n) == "jet_kernel_u16"
    _takes_the_fixed_unit(prog, O.PdeSpec(name="burgers", parameters={"nu": nu}), n)
    cv = I._coef_values((nu,), dev)
    xd, td = x.to(dev), t.to(dev)

    def launch():
        return _inverse_launch(prog, pd, cv, xd, td, n, dev)

    r, s, cg, flat = launch()
    assert torch.isfinite(flat).all() and torch.isfinite(cg).all() and torch.isfinite(s).all()
    r_g, s_g, cg_g, flat_g = _generic(prog, launch)
    assert torch.equal(cg, cg_g), f"d loss / d nu {float(cg[0])!r} != {float(cg_g[0])!r}"
    _same_bits((r, s, flat), (r_g, s_g, flat_g), names, prog, spec, f"inverse N={n}")
    assert all(torch.equal(a, b) for a, b in zip((r, s, cg, flat), launch())), "two launches differ"
    r_v, _ = E.residual_forward(prog, E.pde_desc("burgers", 1, (float(cv[0]),)), xd, td)
    assert torch.equal(r, r_v), "inverse-call and by-value residuals differ"
    if size == "two_units":
        L, dnu, _, gw = I._oracle("burgers", spec, sd, x, t, (nu,))
        e_l = rel_err(float(s) / n, L, label=f"inverse N={n} loss", tol=TOL)
        e_c = abs(float(cg[0]) - dnu) / abs(dnu)
        print(f"inverse N={n}: loss {e_l:.2e}, d loss / d nu {float(cg[0])!r} vs {dnu!r} ({e_c:.2e})")
        assert e_l <= TOL
        assert e_c <= TOL
        _check_grads(prog, names, flat, gw, f"inverse N={n}", TOL, TENSOR_TOL)
        _check_biases(prog, names, flat, gw, spec, f"inverse N={n}")


@pytest.mark.parametrize("n", [17, 96])
def test_bias_of_a_frozen_weight(n, dev):
    """Layer 1 has no weight gradient to form (a null dW in the descriptor) and still owes its bias gradient: the fixed
    units test the pointers once, ahead of the unit loop."""
    from hip_helpers import program_from_spec

    spec = _images_spec(NET)
    o = _oracle(spec, ("burgers", 1), SEED[NET] + 160, n, True)
    prog, names = program_from_spec(spec, o["sd"], dev)
    weights = [k for k in names if k.endswith("weight")]
    assert len(weights) == 4, names
    frozen = weights[1]
    prog.trainable[names.index(frozen)] = False
    _routed_to_u16(prog, n)
    pde = o["pde"]
    _takes_the_fixed_unit(prog, pde, n)
    x, t = o["x"].to(dev), o["t"].to(dev)
    r, s, flat = _loss_grad(prog, dev, pde, x, t, n)
    want = {k: v for k, v in o["gL"].items() if k != frozen}
    _check_grads(prog, names, flat, want, f"N={n} frozen {frozen}", TOL, TENSOR_TOL)
    _check_biases(prog, names, flat, want, spec, f"N={n} frozen {frozen}")
    assert rel_err(float(s) / n, float(o["L"]), label=f"N={n} frozen loss", tol=TOL) <= TOL
    _same_bits((r, s, flat), _generic(prog, lambda: _loss_grad(prog, dev, pde, x, t, n)), names, prog, spec, f"N={n} frozen")
    r2, s2, flat2 = _loss_grad(prog, dev, pde, x, t, n)
    assert torch.equal(flat, flat2) and torch.equal(s, s2) and torch.equal(r, r2), "two launches differ"


def _family_spec(fam):
    """The headline shape with the family's activation: four Linears, that is 64 Fourier features and three MFMA layers
    (test_unit16_kernel_gpu._spec has two).  `sin` exists only as the SIREN network, whose encoding is a first Linear."""
    import oracle as O
    from test_unit16_kernel_gpu import _spec as _kernel_spec

    if fam == "sin":
        return _kernel_spec("sin")
    return O.ArchSpec("fourier", hidden_dim=128, num_layers=4, mapping_size=32, scale=2.0, activation=fam)


@pytest.mark.parametrize("fam", ["tanh", "sin", "gelu", "sigmoid", "relu"])
def test_families(fam, dev):
    """Every activation family at 32 points on the headline shape: fused, forward-only and inverse launches of
    jet_u16mf_<family> / jet_u16mfc_<family> against the generic units, bit for bit, and against the fp64 oracle.  Fixed
    units exist for tanh, gelu and relu (csrc/Makefile: FACTS).  sigmoid keeps jet_u16m_3: its fixed unit rounded the
    layer-0 bias gradient to other bits in this very test and is not built.  `sin` is the SIREN network: it misses the
    shape and takes jet_u16m_1.  For those two the flag changes nothing."""
    from hip_helpers import program_from_spec
    from pinnrl_amd import engine as E

    import test_inverse_fused_gpu as I

    n = 32
    spec = _family_spec(fam)
    o = _oracle(spec, ("burgers", 1), 171, n, True)
    prog, names = program_from_spec(spec, o["sd"], dev)
    pde = o["pde"]
    if fam in ("sin", "sigmoid"):
        from pinnrl_amd import _lib

        assert _unit(prog, pde, n) == f"jet_u16m_{_lib.ACT[fam]}" == _generic(prog, lambda: _unit(prog, pde, n))
    else:
        _takes_the_fixed_unit(prog, pde, n, fam)
    x, t = o["x"].to(dev), o["t"].to(dev)
    tol = RELU_TOL if fam == "relu" else TOL
    r, s, flat = _loss_grad(prog, dev, pde, x, t, n)
    e_r = rel_l2(r.cpu(), o["r"], label=f"{fam} residual", tol=tol)
    e_l = rel_err(float(s) / n, float(o["L"]), label=f"{fam} loss", tol=tol)
    print(f"{fam}: residual rel l2 {e_r:.2e}, loss rel err {e_l:.2e}")
    assert e_r <= tol
    assert e_l <= tol
    _check_grads(prog, names, flat, o["gL"], f"{fam} loss", tol, TENSOR_TOL)
    _same_bits((r, s, flat), _generic(prog, lambda: _loss_grad(prog, dev, pde, x, t, n)), names, prog, spec, fam)
    r_f, _ = E.residual_forward(prog, _pde_desc(pde), x, t)
    assert torch.equal(r_f, r), "forward-only and fused residuals differ"
    r_fg, _ = _generic(prog, lambda: E.residual_forward(prog, _pde_desc(pde), x, t))
    assert torch.equal(r_fg, r), "forward-only residuals of the generic unit differ"
    # the inverse call: jet_u16mfc_<family> against jet_u16mc_<family>
    pd = I._pd("burgers")
    assert E.inverse_kernel_name(prog, pd, n) == "jet_kernel_u16"
    cv = I._coef_values((float(pde.parameters["nu"]),), dev)
    got = _inverse_launch(prog, pd, cv, x, t, n, dev)
    want = _generic(prog, lambda: _inverse_launch(prog, pd, cv, x, t, n, dev))
    assert torch.isfinite(got[3]).all() and torch.isfinite(got[2]).all()
    assert torch.equal(got[2], want[2]), f"{fam}: d loss / d nu {float(got[2][0])!r} != {float(want[2][0])!r}"
    _same_bits((got[0], got[1], got[3]), (want[0], want[1], want[3]), names, prog, spec, f"{fam} inverse")
    r_v, _ = E.residual_forward(prog, E.pde_desc("burgers", 1, (float(cv[0]),)), x, t)
    assert torch.equal(got[0], r_v), "inverse-call and by-value residuals differ"


@pytest.mark.parametrize("fam", ["gelu", "relu"])
def test_other_fixed_families_at_the_ragged_size(fam, dev):
    """Three full units per workgroup and a ragged packed round, as for tanh above: jet_u16mf_<family> and
    jet_u16mfc_<family> against their generic siblings, bit for bit (no oracle at this size)."""
    import oracle as O
    from hip_helpers import program_from_spec
    from pinnrl_amd import engine as E
    from test_inverse_fused_gpu import _coef_values, _pd, _points

    n, _ = _three_units_and_a_ragged_round(dev)
    spec = _family_spec(fam)
    sd = O.init_state_dict(spec, seed=190)
    x, t = (v.to(dev) for v in _points("burgers", n, 191))
    prog, names = program_from_spec(spec, sd, dev)
    pde = O.PdeSpec(name="burgers", parameters={"nu": 0.02})
    _takes_the_fixed_unit(prog, pde, n, fam)
    r, s, flat = _loss_grad(prog, dev, pde, x, t, n)
    assert torch.isfinite(flat).all() and torch.isfinite(s).all() and torch.isfinite(r).all()
    _same_bits((r, s, flat), _generic(prog, lambda: _loss_grad(prog, dev, pde, x, t, n)), names, prog, spec, f"{fam} N={n}")
    r_f, _ = E.residual_forward(prog, _pde_desc(pde), x, t)
    assert torch.equal(r_f, r), "forward-only and fused residuals differ"
    pd, cv = _pd("burgers"), _coef_values((0.02,), dev)
    got = _inverse_launch(prog, pd, cv, x, t, n, dev)
    want = _generic(prog, lambda: _inverse_launch(prog, pd, cv, x, t, n, dev))
    assert torch.equal(got[2], want[2]), f"{fam}: d loss / d nu {float(got[2][0])!r} != {float(want[2][0])!r}"
    _same_bits((got[0], got[1], got[3]), (want[0], want[1], want[3]), names, prog, spec, f"{fam} inverse N={n}")


NEAR_MISSES = ["width_64", "two_layers", "mapping_16", "first_linear"]


def _near_miss(case):
    import oracle as O

    return {
        "width_64": O.ArchSpec("fourier", hidden_dim=64, num_layers=4, mapping_size=32, scale=2.0),
        "two_layers": _images_spec("fourier_2"),
        "mapping_16": O.ArchSpec("fourier", hidden_dim=128, num_layers=4, mapping_size=16, scale=2.0),
        "first_linear": _images_spec("linear_3_narrow"),
    }[case]


@pytest.mark.parametrize("case", NEAR_MISSES)
def test_near_miss_shapes_keep_their_units(case, dev):
    from hip_helpers import program_from_spec
    from pinnrl_amd import engine as E

    n = 33
    spec = _near_miss(case)
    o = _oracle(spec, ("burgers", 1), 180 + NEAR_MISSES.index(case), n, True)
    prog, names = program_from_spec(spec, o["sd"], dev)
    pde = o["pde"]
    unit = _unit(prog, pde, n)
    assert not unit.startswith("jet_u16mf"), unit
    assert _generic(prog, lambda: _unit(prog, pde, n)) == unit
    assert unit == {"width_64": "jet_kernel_wide", "two_layers": "jet_u16m_0", "mapping_16": "jet_u16m_0",
                    "first_linear": "jet_u16m_0"}[case], unit
    x, t = o["x"].to(dev), o["t"].to(dev)
    r, s, flat = _loss_grad(prog, dev, pde, x, t, n)
    e_r = rel_l2(r.cpu(), o["r"], label=f"{case} residual", tol=TOL)
    e_l = rel_err(float(s) / n, float(o["L"]), label=f"{case} loss", tol=TOL)
    print(f"{case}: residual rel l2 {e_r:.2e}, loss rel err {e_l:.2e}")
    assert e_r <= TOL
    assert e_l <= TOL
    _check_grads(prog, names, flat, o["gL"], f"{case} loss", TOL, TENSOR_TOL)
    r_g, s_g, flat_g = _generic(prog, lambda: _loss_grad(prog, dev, pde, x, t, n))
    assert torch.equal(r, r_g) and torch.equal(s, s_g) and torch.equal(flat, flat_g), f"{case}: the flag changed an unrouted call"
    r_f, _ = E.residual_forward(prog, _pde_desc(pde), x, t)
    assert torch.equal(r_f, r), "forward-only and fused residuals differ"
