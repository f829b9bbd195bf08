"""GPU: layer counts, encodings and LDS slots of the 16-point fused kernel (jet_kernel_u16.h).

The kernel keeps its activations, the tape, the running dw_out / loss / db_out sums and the PDE coefficients in LDS, and
which image holds what in the reverse sweep depends on the number of MFMA layers.  These cases run networks with 1, 2 and
3 MFMA layers that the kernel accepts (image height 128, the first MFMA layer reads 64 features): behind 64 Fourier
features and behind a plain first Linear of width 64 (whose gradient is the kernel's encoding-backward pass), one of
them with a 64-wide layer between two 128-wide ones, in which waves 4-7 own no rows.  Point counts: a single point, a ragged second unit (17), and 4 900 (two units
per workgroup).

Every case must be routed to `jet_kernel_u16`; one that is not is an error, not a skip.  Checked: loss, residual and
gradient <= 1e-5 against the fp64 oracle; the forward-only launch's residual bit-identical to the fused launch's; two
launches bit-identical.  The same for one inverse call (COEF unit: coefficients and the running coefficient-gradient
sums live in the row pad of image X), d loss / d nu included.  The workspace is filled with NaN before every reverse
launch."""

import pytest
import torch

from conftest import rel_err, rel_l2
from test_wide_variants_gpu import _check_grads, _oracle, _pde_desc, _poison

pytestmark = pytest.mark.gpu

TOL = 1e-5
TENSOR_TOL = 1e-4  # single tensors (some have a handful of entries), as in test_unit16_kernel_gpu
POINTS = [1, 17, 4_900]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _spec(name):
    import oracle as O

    return {
        # Fourier: 2 * 32 = 64 features, then num_layers - 1 MFMA layers of width 128
        "fourier_1": O.ArchSpec("fourier", hidden_dim=128, num_layers=2, mapping_size=32, scale=2.0),
        "fourier_2": O.ArchSpec("fourier", hidden_dim=128, num_layers=3, mapping_size=32, scale=2.0),
        "fourier_3": O.ArchSpec("fourier", hidden_dim=128, num_layers=4, mapping_size=32, scale=2.0),
        # plain first Linear 2 -> 64 (the encoding), then the MFMA layers
        "linear_1": O.ArchSpec("feedforward", hidden_dims=[64, 128], num_layers=2),
        "linear_2": O.ArchSpec("feedforward", hidden_dims=[64, 128, 128], num_layers=3),
        "linear_3_narrow": O.ArchSpec("feedforward", hidden_dims=[64, 128, 64, 128], num_layers=4),  # 64->128->64->128
    }[name]


MFMA_LAYERS = {"fourier_1": 1, "fourier_2": 2, "fourier_3": 3, "linear_1": 1, "linear_2": 2, "linear_3_narrow": 3}


def _routed_to_u16(prog, n):
    from pinnrl_amd import _lib

    assert "jet_u16_1_2_0:" not in _lib.build_info(), "the tanh (1, 2) unit of the 16-point kernel is not routed to"
    name = _lib.kernel_name(prog, n, 1, 2, 1)
    assert name == "jet_kernel_u16", f"reverse launch takes {name}"
    name = _lib.kernel_name(prog, n, 1, 2, 0)
    assert name == "jet_kernel_u16", f"forward-only launch takes {name}"


def _loss_grad(prog, dev, pde, x, t, n):
    from pinnrl_amd import engine as E

    _poison(prog, dev, n, 1, 2)
    flat = E.new_flat_grad(prog, dev)
    r, s = E.residual_loss_grad(prog, _pde_desc(pde), x, t, 1.0 / n, flat, want_residual=True)
    torch.cuda.synchronize()
    return r.clone(), s.clone(), flat.clone()


def _well_conditioned(spec, seed, n):
    """The fp64 results of the case.  With a single point the relative error of the residual is the relative error of
    one number, and how large fp32 rounding makes it depends on the point: on cancellation between the terms of
    r = u_t + u u_x - nu u_xx (condition number kappa = (|u_t| + |u u_x| + |nu u_xx|) / |r|, 1 to 3 without
    cancellation) and on cancellation inside the network's own sums.  A point where either is large tests the point,
    not the kernel.  So the single-point case takes the first seed (seed, seed + 100, ...) at which kappa <= 4 and the
    oracle's own code, run in fp32 on the CPU, is within a quarter of the bar of its fp64 result; the kernel's results
    play no part in the choice, and the bar stays 1e-5.  Over 17 or 4 900 points the norm is dominated by the large
    residuals and the seed is taken as it is."""
    import oracle as O

    for k in range(16):
        o = _oracle(spec, ("burgers", 1), seed + 100 * k, n, True)
        if n > 1:
            return o
        u, u_t, u_x, u_xx = (float(j[0]) for j in o["jets"])
        r64 = float(o["r"].flatten()[0])
        kappa = (abs(u_t) + abs(u * u_x) + abs(float(o["pde"].parameters["nu"]) * u_xx)) / abs(r64)
        p32 = {name: v.float() for name, v in o["sd"].items()}
        r32 = float(O.compute_residual(o["pde"], lambda inp: O.network_forward(spec, p32, inp), o["x"].float(), o["t"].float()).detach().flatten()[0])
        e32 = abs(r32 - r64) / abs(r64)
        print(f"seed {seed + 100 * k}: single point, kappa {kappa:.2f}, fp32 oracle against fp64 {e32:.2e}")
        if kappa <= 4.0 and e32 <= TOL / 4:
            return o
    raise AssertionError("no well-conditioned single point in 16 seeds")


@pytest.mark.parametrize("n", POINTS)
@pytest.mark.parametrize("net", list(MFMA_LAYERS))
def test_layer_counts_and_encodings(net, n, dev):
    from hip_helpers import program_from_spec
    from pinnrl_amd import engine as E

    spec = _spec(net)
    o = _well_conditioned(spec, 40 + MFMA_LAYERS[net], n)
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
    r_f2, _ = E.residual_forward(prog, _pde_desc(pde), x, t)  # (its loss sum is added atomically: not compared)
    assert torch.equal(r_f, r_f2), "two forward-only launches differ"


@pytest.mark.parametrize("n", POINTS)
def test_inverse_call_keeps_its_row_pad_slots(n, dev):
    """The COEF unit on the headline shape (three MFMA layers behind 64 Fourier features)."""
    import oracle as O
    from hip_helpers import program_from_spec
    from pinnrl_amd import _lib
    from pinnrl_amd import engine as E
    from test_inverse_fused_gpu import _coef_values, _pd, _points
    from test_inverse_fused_gpu import _oracle as _inverse_oracle

    nu = 0.02
    spec = _spec("fourier_3")
    sd = O.init_state_dict(spec, seed=51)
    x, t = _points("burgers", n, 52)
    L, dnu, _, gw = _inverse_oracle("burgers", spec, sd, x, t, (nu,))
    prog, names_all = program_from_spec(spec, sd, dev)
    pd = _pd("burgers")  # pde->coef holds garbage: the coefficients come from the device array
    assert "jet_u16c_1_2_0:" not in _lib.build_info(), "the tanh (1, 2) COEF unit of the 16-point kernel is not routed to"
    assert E.inverse_kernel_name(prog, pd, n) == "jet_kernel_u16"
    xd, td = x.to(dev), t.to(dev)
    cv = _coef_values((nu,), dev)

    def launch():
        from test_inverse_fused_gpu import _poison as _poison_inverse

        _poison_inverse(prog, pd, dev, n)
        flat = E.new_flat_grad(prog, dev)
        cg = torch.zeros(4, dtype=torch.float32, device=dev)
        r, s = E.residual_loss_grad_inverse(prog, pd, cv, xd, td, 1.0 / n, flat, cg, want_residual=True)
        torch.cuda.synchronize()
        return r.clone(), s.clone(), cg.clone(), flat.clone()

    r, s, cg, flat = launch()
    assert torch.isfinite(flat).all() and torch.isfinite(cg).all() and torch.isfinite(s).all()
    e_l = rel_err(float(s) / n, L, label=f"inverse N={n} loss", tol=TOL)
    e_c = abs(float(cg[0]) - dnu) / abs(dnu)
    by_name = {k: g for k, g in zip(names_all, E.split_flat_grad(prog, flat)) if g is not None}
    e_g = rel_l2(torch.cat([by_name[k].flatten().cpu() for k in gw]), torch.cat([gw[k].flatten() for k in gw]),
                 label=f"inverse N={n} weight gradient", tol=TOL)
    # the residual of the same points with nu by value (fp64 oracle, then the forward-only launch)
    pde = O.PdeSpec(name="burgers", dimension=1, domain=((-1.0, 1.0),), parameters={"nu": float(torch.tensor(nu, dtype=torch.float32))})
    params = {k: v.double() for k, v in sd.items()}
    r_want = O.compute_residual(pde, lambda z: O.network_forward(spec, params, z), x.double(), t.double()).detach()
    e_r = rel_l2(r.cpu(), r_want, label=f"inverse N={n} residual", tol=TOL)
    print(f"inverse N={n}: loss {e_l:.2e}, d loss / d nu {float(cg[0])!r} vs {dnu!r} ({e_c:.2e}), gradient {e_g:.2e}, residual {e_r:.2e}")
    assert e_l <= TOL
    assert e_c <= TOL
    assert e_g <= TOL
    assert e_r <= TOL
    assert float(cg[1]) == 0.0 and float(cg[2]) == 0.0 and float(cg[3]) == 0.0
    r2, s2, cg2, flat2 = launch()
    assert torch.equal(r, r2) and torch.equal(s, s2) and torch.equal(cg, cg2) and torch.equal(flat, flat2), "two launches differ"
    r_f, _ = E.residual_forward(prog, E.pde_desc("burgers", 1, (nu,)), xd, td)
    assert torch.equal(r_f, r), "forward-only and inverse-call residuals differ"
