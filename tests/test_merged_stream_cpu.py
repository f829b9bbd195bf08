"""CPU: the merged stream set (u, u_t - nu u_xx, u_x) of the Burgers residual against the four-stream model, in fp64.

`merged_model.py` restates the rules of the merged device functions of `csrc/jet_device.h`; here its residual, loss,
weight gradient and d loss / d nu (activation partials and the Fourier features' own term) are compared with
`jet_model.py` on four streams.  The two are the same mathematics summed in another order, so the bar is 1e-12.
Also: the A/B flag constant of the header and of `_lib`.
"""

import os
import re

import pytest
import torch

import jet_model as J
import merged_model as M

TOL = 1e-12
ACTS = [("tanh", 0.0), ("sin", 1.5), ("gelu", 0.0), ("sigmoid", 0.0), ("relu", 0.0)]


def _program(enc, width, act, par, seed):
    import oracle as O

    if enc == "fourier":
        spec = O.ArchSpec("fourier", hidden_dim=width, num_layers=4, mapping_size=16, scale=2.0)
    else:
        spec = O.ArchSpec("feedforward", hidden_dims=[width, width, width], num_layers=3)
    sd = {k: v.double() for k, v in O.init_state_dict(spec, seed=seed).items()}
    prog = J.mlp_program(spec, sd)
    prog["hidden"] = [(W, b, act, par, nm) for W, b, _, _, nm in prog["hidden"]]
    return prog


def _rel(a, b):
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("act,par", ACTS)
@pytest.mark.parametrize("width", [32, 128])
@pytest.mark.parametrize("enc", ["fourier", "linear"])
def test_merged_equals_four_streams(enc, width, act, par):
    torch.manual_seed(7)
    n = 23
    inp = torch.cat([torch.rand(n, 1, dtype=torch.float64) * 2 - 1, torch.rand(n, 1, dtype=torch.float64)], 1)
    prog = _program(enc, width, act, par, 11)
    for nu in (0.01 / torch.pi, 0.02):
        r4, l4, g4, dnu4 = M.burgers_loss_grad_plain(prog, inp, nu)
        r3, l3, g3, dnu3 = M.burgers_loss_grad(prog, inp, nu)
        assert _rel(r3, r4) <= TOL
        assert abs(float(l3 - l4)) <= TOL * abs(float(l4))
        assert set(g3) == set(g4)
        for k in g4:
            assert _rel(g3[k], g4[k]) <= TOL, k
        if act == "relu" and enc == "linear":  # piecewise-linear network of the coordinates: u_xx = 0 identically
            assert float(dnu4) == 0.0 and float(dnu3) == 0.0
        else:
            assert abs(float(dnu3 - dnu4)) <= TOL * abs(float(dnu4)), (float(dnu3), float(dnu4))


def test_coefficient_cotangent_is_the_derivative_of_the_loss():
    """d loss / d nu of the merged adjoint against a central difference of the four-stream loss."""
    torch.manual_seed(3)
    inp = torch.cat([torch.rand(19, 1, dtype=torch.float64) * 2 - 1, torch.rand(19, 1, dtype=torch.float64)], 1)
    prog = _program("fourier", 32, "tanh", 0.0, 5)
    nu, h = 0.02, 1e-6
    _, _, _, dnu = M.burgers_loss_grad(prog, inp, nu)
    lp = M.burgers_loss_grad_plain(prog, inp, nu + h)[1]
    lm = M.burgers_loss_grad_plain(prog, inp, nu - h)[1]
    assert abs(float(dnu) - float(lp - lm) / (2 * h)) <= 1e-7 * abs(float(dnu))


def test_flag_constant_and_abi_version():
    from pinnrl_amd import _lib

    here = os.path.dirname(os.path.abspath(__file__))
    hdr = open(os.path.join(here, "..", "include", "pinn_jet.h")).read()
    assert int(re.search(r"#define PINN_FLAG_PLAIN_STREAMS (\d+)", hdr).group(1)) == 16 == _lib.PINN_FLAG_PLAIN_STREAMS
    assert int(re.search(r"#define PINN_ABI_VERSION (\d+)", hdr).group(1)) == 2 == _lib.PINN_ABI_VERSION
    others = [_lib.PINN_FLAG_LAYER_NORM, _lib.PINN_FLAG_DETERMINISTIC, _lib.PINN_FLAG_LAYER_MAJOR, _lib.PINN_FLAG_WIDE_TILE32]
    assert all(_lib.PINN_FLAG_PLAIN_STREAMS & f == 0 for f in others)
