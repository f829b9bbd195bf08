"""GPU: the merged units of the 16-point fused kernel (jet_u16m_<family>, jet_u16mc_<family>) fetch a unit's coordinates
with one load per lane of wave 0, requested in the unit before the one that stores them (jet_kernel_u16.h; DESIGN.md
§4.1).  The hidden layers' bias gradients keep their column sums in LDS (summing them in the dW GEMM's operand registers
was measured and dropped); they are asserted by name here all the same, at sizes where the unit
loop and the packed round both contribute.

What can go wrong, and the size that shows it:

* 1 point: the packed round alone: every request of the unit loop is masked;
* 17 points: one unit and a one-point packed round: the unit's request for a next unit is masked, the round reads its
  own buffer;
* 32 points: one workgroup, two units (the coordinates of the second are the ones requested in the prologue);
* 96 points: three workgroups;
* three full units per workgroup and a ragged packed round: the two-ahead request wraps the double buffer, and the
  request past the workgroup's last unit is masked.  The four-stream units (PINN_FLAG_PLAIN_STREAMS) keep the earlier
  fetch, so they check the point order independently;
* a frozen hidden weight whose bias is trained (reachable through NetProgram's `trainable`): that layer skips its dW
  GEMM and still owes its bias gradient.  This case runs code the coordinate change does not touch; it is here because
  nothing else in the suite covers it.

Helpers and bars of test_merged_keep_gpu.py / test_unit16_kernel_gpu.py: 1e-5 against the fp64 oracle (1e-4 per
tensor), 2e-6 against the four-stream units.
"""

import pytest
import torch

from conftest import rel_err, rel_l2
from test_merged_keep_gpu import SEED, _three_units_and_a_ragged_round
from test_merged_stream_gpu import _plain
from test_unit16_images_gpu import _routed_to_u16, _well_conditioned
from test_unit16_images_gpu import _spec as _images_spec
from test_unit16_kernel_gpu import AB_TOL, TENSOR_TOL, TOL, _loss_grad
from test_wide_variants_gpu import _check_grads, _oracle, _pde_desc

pytestmark = pytest.mark.gpu

NETS = ["fourier_1", "fourier_2", "fourier_3", "linear_2", "linear_3_narrow"]
SEEDS = dict(SEED, linear_3_narrow=85)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _hidden_biases(names, spec):
    """Names of the bias vectors of the MFMA layers: every Linear bias but the output layer's (and but the first
    Linear's where that one is the encoding)."""
    biases = [k for k in names if k.endswith("bias")]
    return biases[(0 if spec.architecture == "fourier" else 1):-1]


def _check_biases(prog, names, flat, want, spec, what):
    from pinnrl_amd import engine as E

    by_name = {k: g for k, g in zip(names, E.split_flat_grad(prog, flat)) if g is not None}
    keys = _hidden_biases(names, spec)
    assert keys, names
    for k in keys:
        e = rel_l2(by_name[k].cpu(), want[k], label=f"{what} bias {k}", tol=TENSOR_TOL)
        print(f"{what}: {k}: {e:.2e}")
        assert e <= TENSOR_TOL, f"{what}: {k}: {e:.2e}"


def test_build_facts():
    from pinnrl_amd import _lib

    info = _lib.build_info()
    for unit in ("jet_u16m_0", "jet_u16mc_0"):
        assert f"{unit}:" not in info, info
        assert f"nopack {unit} " not in info, info


@pytest.mark.parametrize("n", [1, 17, 32, 96])
@pytest.mark.parametrize("net", NETS)
def test_small_sizes(net, n, dev):
    from hip_helpers import program_from_spec
    from pinnrl_amd import _lib
    from pinnrl_amd import engine as E

    spec = _images_spec(net)
    o = _well_conditioned(spec, SEEDS[net] + 30, n) if n == 1 else _oracle(spec, ("burgers", 1), SEEDS[net] + 30, n, True)
    prog, names = program_from_spec(spec, o["sd"], dev)
    _routed_to_u16(prog, n)
    grid = _lib.kernel_for(prog, n, 1, 2, 1)["grid"]
    plan = _lib.u16_tail_plan(n, grid)[:2]
    assert (grid, plan) == {1: (1, (0, 1)), 17: (1, (1, 1)), 32: (1, (2, 0)), 96: (3, (2, 0))}[n], (grid, plan)
    pde = o["pde"]
    x, t = o["x"].to(dev), o["t"].to(dev)
    r, s, flat = _loss_grad(prog, dev, pde, x, t, n)
    e_r = rel_l2(r.cpu(), o["r"], label=f"{net} N={n} residual", tol=TOL)
    e_l = rel_err(float(s) / n, float(o["L"]), label=f"{net} N={n} loss", tol=TOL)
    print(f"{net} N={n}: residual rel l2 {e_r:.2e}, loss rel err {e_l:.2e}")
    assert e_r <= TOL
    assert e_l <= TOL
    _check_grads(prog, names, flat, o["gL"], f"{net} N={n} loss", TOL, TENSOR_TOL)
    _check_biases(prog, names, flat, o["gL"], spec, f"{net} N={n}")
    r_f, _ = E.residual_forward(prog, _pde_desc(pde), x, t)
    assert torch.equal(r_f, r), "forward-only and fused residuals differ"
    r2, s2, flat2 = _loss_grad(prog, dev, pde, x, t, n)
    assert torch.equal(flat, flat2) and torch.equal(s, s2) and torch.equal(r, r2), "two launches differ"
    if n > 1:  # (the two stream sets may well round a single residual to the same bits)
        r_p, _, _ = _plain(prog, lambda: _loss_grad(prog, dev, pde, x, t, n))
        assert not torch.equal(r_p, r), "the call did not take the merged unit"


@pytest.mark.parametrize("net", ["fourier_3", "fourier_2", "linear_2"])
def test_three_units_then_a_ragged_packed_round(net, dev):
    import oracle as O
    from hip_helpers import program_from_spec
    from pinnrl_amd import _lib
    from pinnrl_amd import engine as E
    from test_inverse_fused_gpu import _points

    n, g = _three_units_and_a_ragged_round(dev)
    spec = _images_spec(net)
    sd = O.init_state_dict(spec, seed=SEEDS[net] + 40)
    x, t = (v.to(dev) for v in _points("burgers", n, SEEDS[net] + 41))
    prog, names = program_from_spec(spec, sd, dev)
    _routed_to_u16(prog, n)
    assert _lib.kernel_for(prog, n, 1, 2, 1)["grid"] == g
    pde = O.PdeSpec(name="burgers", parameters={"nu": 0.02})
    r, s, flat = _loss_grad(prog, dev, pde, x, t, n)
    assert torch.isfinite(flat).all() and torch.isfinite(s).all() and torch.isfinite(r).all()
    r4, s4, flat4 = _plain(prog, lambda: _loss_grad(prog, dev, pde, x, t, n))
    assert not torch.equal(r4, r), "the call did not take the merged unit"
    e_g = rel_l2(flat.cpu(), flat4.cpu(), label=f"{net} N={n} merged grad vs four streams", tol=AB_TOL)
    e_l = rel_err(float(s), float(s4), label=f"{net} N={n} merged loss vs four streams", tol=AB_TOL)
    # Point for point: both are fp32 evaluations of the same residual within TOL of fp64 relative to its size, so a pair
    # differs by at most 2 TOL of the largest residual; a point that took another point's coordinates differs by O(1).
    e_p = float((r - r4).abs().max() / r4.abs().max())
    print(f"{net} N={n}: gradient rel l2 {e_g:.2e}, loss rel err {e_l:.2e}, residual max point error {e_p:.2e} against the four-stream unit")
    assert e_g <= AB_TOL
    assert e_l <= AB_TOL
    assert e_p <= 2 * TOL
    by, by4 = (dict(zip(names, E.split_flat_grad(prog, f))) for f in (flat, flat4))
    for k in _hidden_biases(names, spec):
        e_b = rel_l2(by[k].cpu(), by4[k].cpu(), label=f"{net} N={n} bias {k} vs four streams", tol=AB_TOL)
        print(f"{net} N={n}: {k}: {e_b:.2e}")
        assert e_b <= AB_TOL
    r_f, _ = E.residual_forward(prog, _pde_desc(pde), x, t)
    assert torch.equal(r_f, r), "forward-only and fused residuals differ"
    r2, s2, flat2 = _loss_grad(prog, dev, pde, x, t, n)
    assert torch.equal(flat, flat2) and torch.equal(s, s2) and torch.equal(r, r2), "two launches differ"


@pytest.mark.parametrize("n", [17, 96])
def test_bias_of_a_frozen_weight(n, dev):
    """Layer 1 of three MFMA layers has no weight gradient to form and skips its dW GEMM; its bias gradient, and those of
    layers 0 and 2, are still due."""
    from hip_helpers import program_from_spec

    net = "fourier_3"
    spec = _images_spec(net)
    o = _oracle(spec, ("burgers", 1), SEEDS[net] + 50, n, True)
    prog, names = program_from_spec(spec, o["sd"], dev)
    weights = [k for k in names if k.endswith("weight")]
    assert len(weights) == 4, names
    frozen = weights[1]
    prog.trainable[names.index(frozen)] = False
    _routed_to_u16(prog, n)
    pde = o["pde"]
    x, t = o["x"].to(dev), o["t"].to(dev)
    r, s, flat = _loss_grad(prog, dev, pde, x, t, n)
    want = {k: v for k, v in o["gL"].items() if k != frozen}
    _check_grads(prog, names, flat, want, f"{net} N={n} frozen {frozen}", TOL, TENSOR_TOL)
    _check_biases(prog, names, flat, want, spec, f"{net} N={n} frozen {frozen}")
    e_l = rel_err(float(s) / n, float(o["L"]), label=f"{net} N={n} frozen loss", tol=TOL)
    assert e_l <= TOL
    r2, s2, flat2 = _loss_grad(prog, dev, pde, x, t, n)
    assert torch.equal(flat, flat2) and torch.equal(s, s2) and torch.equal(r, r2), "two launches differ"


@pytest.mark.parametrize("net", ["fourier_3", "fourier_2"])
def test_inverse_call_two_full_units(net, dev):
    """jet_u16mc_<family> over two full units of one workgroup: weight gradient, bias vectors by name and d loss / d nu."""
    import oracle as O
    from hip_helpers import program_from_spec
    from pinnrl_amd import engine as E

    import test_inverse_fused_gpu as I

    n, nu = 32, 0.02
    spec = _images_spec(net)
    sd = O.init_state_dict(spec, seed=SEEDS[net] + 60)
    x, t = I._points("burgers", n, SEEDS[net] + 61)
    L, dnu, _, gw = I._oracle("burgers", spec, sd, x, t, (nu,))
    prog, names = program_from_spec(spec, sd, dev)
    pd = I._pd("burgers")
    assert E.inverse_kernel_name(prog, pd, n) == "jet_kernel_u16"
    cv = I._coef_values((nu,), dev)
    xd, td = x.to(dev), t.to(dev)
    s, cg, flat = I._launch(prog, pd, cv, xd, td, 1.0 / n, dev)
    assert torch.isfinite(flat).all() and torch.isfinite(cg).all() and torch.isfinite(s).all()
    e_l = rel_err(float(s) / n, L, label=f"inverse {net} N={n} loss", tol=TOL)
    e_c = abs(float(cg[0]) - dnu) / abs(dnu)
    print(f"inverse {net} N={n}: loss {e_l:.2e}, d loss / d nu {float(cg[0])!r} vs {dnu!r} ({e_c:.2e})")
    assert e_l <= TOL
    assert e_c <= TOL
    _check_grads(prog, names, flat, gw, f"inverse {net} N={n}", TOL, TENSOR_TOL)
    _check_biases(prog, names, flat, gw, spec, f"inverse {net} N={n}")
    got2 = I._launch(prog, pd, cv, xd, td, 1.0 / n, dev)
    assert all(torch.equal(a, b) for a, b in zip((s, cg, flat), got2)), "two launches differ"
    r_i, _ = E.residual_loss_grad_inverse(prog, pd, cv, xd, td, 1.0 / n, E.new_flat_grad(prog, dev),
                                          torch.zeros(4, dtype=torch.float32, device=dev), want_residual=True)
    r_v, _ = E.residual_forward(prog, E.pde_desc("burgers", 1, (float(cv[0]),)), xd, td)
    assert torch.equal(r_i, r_v), "inverse-call and by-value residuals differ"


def test_inverse_call_three_units_then_a_ragged_packed_round(dev):
    """The merged COEF unit against the four-stream COEF unit of the same build, two MFMA layers."""
    import oracle as O
    from hip_helpers import program_from_spec
    from pinnrl_amd import _lib
    from pinnrl_amd import engine as E

    import test_inverse_fused_gpu as I

    assert "jet_u16c_1_2_0:" not in _lib.build_info(), "the four-stream tanh COEF unit of the 16-point kernel is not routed to"
    n, g = _three_units_and_a_ragged_round(dev)
    nu = 0.02
    spec = _images_spec("fourier_2")
    sd = O.init_state_dict(spec, seed=97)
    x, t = (v.to(dev) for v in I._points("burgers", n, 98))
    prog, names = program_from_spec(spec, sd, dev)
    pd = I._pd("burgers")
    assert E.inverse_kernel_name(prog, pd, n) == "jet_kernel_u16"
    cv = I._coef_values((nu,), dev)

    def launch():
        I._poison(prog, pd, dev, n)
        flat = E.new_flat_grad(prog, dev)
        cg = torch.zeros(4, dtype=torch.float32, device=dev)
        r, s = E.residual_loss_grad_inverse(prog, pd, cv, x, t, 1.0 / n, flat, cg, want_residual=True)
        torch.cuda.synchronize()
        return r.clone(), s.clone(), cg.clone(), flat.clone()

    r, s, cg, flat = launch()
    assert torch.isfinite(flat).all() and torch.isfinite(cg).all() and torch.isfinite(s).all()
    r4, s4, cg4, flat4 = _plain(prog, launch)
    assert not torch.equal(r4, r), "the call did not take the merged unit"
    e_g = rel_l2(flat.cpu(), flat4.cpu(), label=f"inverse N={n} merged grad vs four streams", tol=AB_TOL)
    e_l = rel_err(float(s), float(s4), label=f"inverse N={n} merged loss vs four streams", tol=AB_TOL)
    e_c = rel_err(float(cg[0]), float(cg4[0]), label=f"inverse N={n} merged d loss / d nu vs four streams", tol=AB_TOL)
    print(f"inverse N={n}: gradient {e_g:.2e}, loss {e_l:.2e}, d loss / d nu {e_c:.2e} against the four-stream COEF unit")
    assert e_g <= AB_TOL
    assert e_l <= AB_TOL
    assert e_c <= AB_TOL
    by, by4 = (dict(zip(names, E.split_flat_grad(prog, f))) for f in (flat, flat4))
    for k in _hidden_biases(names, spec):
        e_b = rel_l2(by[k].cpu(), by4[k].cpu(), label=f"inverse N={n} bias {k} vs four streams", tol=AB_TOL)
        assert e_b <= AB_TOL
    assert all(torch.equal(a, b) for a, b in zip((r, s, cg, flat), launch())), "two launches differ"
    r_v, _ = E.residual_forward(prog, E.pde_desc("burgers", 1, (float(cv[0]),)), x, t)
    assert torch.equal(r, r_v), "inverse-call and by-value residuals differ"
