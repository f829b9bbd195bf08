"""GPU: the merged units of the 16-point fused kernel (jet_u16m_<family>, jet_u16mc_<family>) keep the forward sweep's
activations in LDS and store every zbar over the record it was computed from (jet_kernel_u16.h, KEEP).

A unit now reads images that the unit before it, in the same workgroup, has left behind: the activations of one parity
stay in X, of the other in A2, the adjoints in the record images and S.  The existing merged-stream tests run at most one
full unit per workgroup, so these run several:

* 32 points (one workgroup, two full units, no packed round) and 96 (three workgroups of two units) against the fp64
  oracle, for one to three MFMA layers behind Fourier features and behind a first Linear;
* three full units per workgroup and then a ragged packed round of two groups (16 g 3 + 4 g 2 - 3 points on g compute
  units: 14 333 on 256), the merged unit against the four-stream unit of the same build (PINN_FLAG_PLAIN_STREAMS), which
  still replays its activations;
* the inverse call (jet_u16mc_<family>) at both sizes.

Helpers and bars of test_merged_stream_gpu.py / test_unit16_kernel_gpu.py: 1e-5 against the fp64 oracle (1e-4 per
tensor), 2e-6 against the four-stream units.
"""

import pytest
import torch

from conftest import rel_err, rel_l2
from test_merged_stream_gpu import _plain
from test_unit16_images_gpu import _routed_to_u16
from test_unit16_images_gpu import _spec as _images_spec
from test_unit16_kernel_gpu import AB_TOL, TENSOR_TOL, TOL, _loss_grad
from test_wide_variants_gpu import _check_grads, _oracle, _pde_desc

pytestmark = pytest.mark.gpu

NETS = ["fourier_1", "fourier_2", "fourier_3", "linear_2"]
SEED = {"fourier_1": 81, "fourier_2": 82, "fourier_3": 83, "linear_2": 84}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _three_units_and_a_ragged_round(dev):
    """(N, g): three full rounds on the device's g compute units, then two four-point groups per workgroup, the last
    one three points short."""
    from pinnrl_amd import _lib

    g = torch.cuda.get_device_properties(dev).multi_processor_count
    n = 16 * g * 3 + 4 * g * 2 - 3
    rounds, groups, first_tail = _lib.u16_tail_plan(n, g)
    assert (rounds, groups, first_tail) == (3, 2, 48 * g), (rounds, groups, first_tail)
    return n, g


def test_build_facts():
    from pinnrl_amd import _lib

    info = _lib.build_info()
    for unit in ("jet_u16m_0", "jet_u16mc_0"):
        assert f"{unit}:" not in info, info
        assert f"nopack {unit} " not in info, info


@pytest.mark.parametrize("n", [32, 96])
@pytest.mark.parametrize("net", NETS)
def test_two_full_units_per_workgroup(net, n, dev):
    from hip_helpers import program_from_spec
    from pinnrl_amd import _lib
    from pinnrl_amd import engine as E

    spec = _images_spec(net)
    o = _oracle(spec, ("burgers", 1), SEED[net], n, True)
    prog, names = program_from_spec(spec, o["sd"], dev)
    _routed_to_u16(prog, n)
    grid = _lib.kernel_for(prog, n, 1, 2, 1)["grid"]
    assert grid == n // 32 and _lib.u16_tail_plan(n, grid)[:2] == (2, 0), "two full units per workgroup, no packed round"
    pde = o["pde"]
    x, t = o["x"].to(dev), o["t"].to(dev)
    r, s, flat = _loss_grad(prog, dev, pde, x, t, n)
    e_r = rel_l2(r.cpu(), o["r"], label=f"{net} N={n} residual", tol=TOL)
    e_l = rel_err(float(s) / n, float(o["L"]), label=f"{net} N={n} loss", tol=TOL)
    print(f"{net} N={n}: residual rel l2 {e_r:.2e}, loss rel err {e_l:.2e}")
    assert e_r <= TOL
    assert e_l <= TOL
    _check_grads(prog, names, flat, o["gL"], f"{net} N={n} loss", TOL, TENSOR_TOL)
    r_f, _ = E.residual_forward(prog, _pde_desc(pde), x, t)
    assert torch.equal(r_f, r), "forward-only and fused residuals differ"
    r2, s2, flat2 = _loss_grad(prog, dev, pde, x, t, n)
    assert torch.equal(flat, flat2) and torch.equal(s, s2) and torch.equal(r, r2), "two launches differ"
    r_p, _, _ = _plain(prog, lambda: _loss_grad(prog, dev, pde, x, t, n))
    assert not torch.equal(r_p, r), "the call did not take the merged unit"


@pytest.mark.parametrize("net", ["fourier_3", "fourier_2"])
def test_three_units_then_a_ragged_packed_round(net, dev):
    import oracle as O
    from hip_helpers import program_from_spec
    from pinnrl_amd import _lib
    from test_inverse_fused_gpu import _points

    n, g = _three_units_and_a_ragged_round(dev)
    spec = _images_spec(net)
    sd = O.init_state_dict(spec, seed=SEED[net] + 10)
    x, t = (v.to(dev) for v in _points("burgers", n, SEED[net] + 11))
    prog, names = program_from_spec(spec, sd, dev)
    _routed_to_u16(prog, n)
    assert _lib.kernel_for(prog, n, 1, 2, 1)["grid"] == g
    pde = O.PdeSpec(name="burgers", parameters={"nu": 0.02})
    r, s, flat = _loss_grad(prog, dev, pde, x, t, n)  # (poisons the workspace first)
    assert torch.isfinite(flat).all() and torch.isfinite(s).all() and torch.isfinite(r).all()
    r4, s4, flat4 = _plain(prog, lambda: _loss_grad(prog, dev, pde, x, t, n))
    assert not torch.equal(r4, r), "the call did not take the merged unit"
    e_g = rel_l2(flat.cpu(), flat4.cpu(), label=f"{net} N={n} merged grad vs four streams", tol=AB_TOL)
    e_l = rel_err(float(s), float(s4), label=f"{net} N={n} merged loss vs four streams", tol=AB_TOL)
    print(f"{net} N={n}: gradient rel l2 {e_g:.2e}, loss rel err {e_l:.2e} against the four-stream unit")
    assert e_g <= AB_TOL
    assert e_l <= AB_TOL
    r2, s2, flat2 = _loss_grad(prog, dev, pde, x, t, n)
    assert torch.equal(flat, flat2) and torch.equal(s, s2) and torch.equal(r, r2), "two launches differ"


@pytest.mark.parametrize("net", ["fourier_3", "linear_2"])
def test_inverse_call_two_full_units(net, dev):
    """d loss / d nu of the merged COEF unit over two full units of one workgroup; its residual has the bits of the
    by-value call."""
    import oracle as O
    from hip_helpers import program_from_spec
    from pinnrl_amd import engine as E

    import test_inverse_fused_gpu as I

    n, nu = 32, 0.02
    spec = _images_spec(net)
    sd = O.init_state_dict(spec, seed=SEED[net] + 20)
    x, t = I._points("burgers", n, SEED[net] + 21)
    L, dnu, _, gw = I._oracle("burgers", spec, sd, x, t, (nu,))
    prog, names_all = program_from_spec(spec, sd, dev)
    pd = I._pd("burgers")
    assert E.inverse_kernel_name(prog, pd, n) == "jet_kernel_u16"
    cv = I._coef_values((nu,), dev)
    xd, td = x.to(dev), t.to(dev)
    s, cg, flat = I._launch(prog, pd, cv, xd, td, 1.0 / n, dev)
    assert torch.isfinite(flat).all() and torch.isfinite(cg).all() and torch.isfinite(s).all()
    e_l = rel_err(float(s) / n, L, label=f"inverse {net} N={n} loss", tol=TOL)
    e_c = abs(float(cg[0]) - dnu) / abs(dnu)
    by_name = {k: g for k, g in zip(names_all, E.split_flat_grad(prog, flat)) if g is not None}
    e_g = rel_l2(torch.cat([by_name[k].flatten().cpu() for k in gw]), torch.cat([gw[k].flatten() for k in gw]),
                 label=f"inverse {net} N={n} weight gradient", tol=TOL)
    print(f"inverse {net} N={n}: loss {e_l:.2e}, d loss / d nu {float(cg[0])!r} vs {dnu!r} ({e_c:.2e}), gradient {e_g:.2e}")
    assert e_l <= TOL
    assert e_c <= TOL
    assert e_g <= TOL
    assert float(cg[1]) == 0.0 and float(cg[2]) == 0.0 and float(cg[3]) == 0.0
    got2 = I._launch(prog, pd, cv, xd, td, 1.0 / n, dev)
    assert all(torch.equal(a, b) for a, b in zip((s, cg, flat), got2)), "two launches differ"
    r_i, _ = E.residual_loss_grad_inverse(prog, pd, cv, xd, td, 1.0 / n, E.new_flat_grad(prog, dev),
                                          torch.zeros(4, dtype=torch.float32, device=dev), want_residual=True)
    r_v, _ = E.residual_forward(prog, E.pde_desc("burgers", 1, (float(cv[0]),)), xd, td)
    assert torch.equal(r_i, r_v), "inverse-call and by-value residuals differ"


def test_inverse_call_three_units_then_a_ragged_packed_round(dev):
    """The merged COEF unit against the four-stream COEF unit of the same build."""
    import oracle as O
    from hip_helpers import program_from_spec
    from pinnrl_amd import _lib
    from pinnrl_amd import engine as E

    import test_inverse_fused_gpu as I

    assert "jet_u16c_1_2_0:" not in _lib.build_info(), "the four-stream tanh COEF unit of the 16-point kernel is not routed to"
    n, g = _three_units_and_a_ragged_round(dev)
    nu = 0.02
    spec = _images_spec("fourier_3")
    sd = O.init_state_dict(spec, seed=95)
    x, t = (v.to(dev) for v in I._points("burgers", n, 96))
    prog, _ = program_from_spec(spec, sd, dev)
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
    assert all(torch.equal(a, b) for a, b in zip((r, s, cg, flat), launch())), "two launches differ"
    r_v, _ = E.residual_forward(prog, E.pde_desc("burgers", 1, (float(cv[0]),)), x, t)
    assert torch.equal(r, r_v), "inverse-call and by-value residuals differ"
