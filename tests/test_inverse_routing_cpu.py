"""CPU test (no GPU): routing and workspace sizing of `pinn_residual_loss_grad_inverse` (inverse problems: PDE coefficients
read from a device array at launch time, coefficient cotangents from the same launch).

The queries make the decisions the call makes (pinn_abi.hip: inverse_route = use_wide / use_u16 with the COEF units
`jet_widec_*` / `jet_u16c_*` in place of the plain ones): descriptors of the plain-MLP family take the fused tile-major
kernels, a stream set without a COEF unit and every other descriptor take the layer-major engine."""

import ctypes

import pytest

import pinnrl_amd  # noqa: F401
from pinnrl_amd import _lib
from pinnrl_amd import engine as E


def _net(arch, widths, act="tanh", input_dim=2, mapping_size=0, **kw):
    """Descriptor only: the queries read no tensor."""
    return E.NetProgram(arch, act, input_dim, list(widths) + [1], [], [], mapping_size=mapping_size,
                        omega_0=5.0 if arch == "siren" else 0.0, **kw)


def _headline():
    return _net("fourier", [128] * 3, mapping_size=32)  # fourier 4x128: 64 Fourier features, three MFMA layers


def _pd(kind, coef=(0.02, 0.05)):
    return E.pde_desc(kind, 1, list(coef))


def _name(prog, kind, N=4900):
    return E.inverse_kernel_name(prog, _pd(kind), N)


def _inv_bytes(prog, kind, N):
    return _lib.load().pinn_inverse_workspace_bytes(ctypes.byref(prog.desc), ctypes.byref(_pd(kind)), N)


def _lm_bytes(prog, kind, N):
    """Size of the layer-major engine for the PDE's stream set, from a flagged copy of the descriptor."""
    nt, nx = E.pde_streams(_pd(kind))
    d = _lib.PinnNetDesc.from_buffer_copy(bytes(prog.desc))
    d.flags |= _lib.PINN_FLAG_LAYER_MAJOR
    return _lib.load().pinn_workspace_bytes(ctypes.byref(d), N, nt, nx, 1)


def test_the_three_symbols_are_exported():
    lib = _lib.load()
    for sym in ("pinn_residual_loss_grad_inverse", "pinn_inverse_workspace_bytes", "pinn_inverse_kernel_name"):
        assert sym in _lib.EXPORTS
        assert getattr(lib, sym) is not None


def test_headline_network_takes_the_16_point_unit():
    prog = _headline()
    # a 16-point COEF unit that pinn_build_info() lists (scratch, or the default MFMA form) is not routed to
    want = "jet_kernel_wide" if "jet_u16c_1_2_0:" in _lib.build_info() else "jet_kernel_u16"
    assert _name(prog, "burgers") == want
    prog.desc.flags |= _lib.PINN_FLAG_WIDE_TILE32
    assert _name(prog, "burgers") == "jet_kernel_wide"


def test_mlp_family_takes_the_32_point_unit():
    ff64 = _net("feedforward", [64] * 3)
    for kind in ("heat", "wave", "cahn_hilliard", "convection", "allen_cahn", "black_scholes", "pendulum", "heat_laplacian"):
        assert _name(ff64, kind) == "jet_kernel_wide", kind


@pytest.mark.parametrize("kind", ["wave", "cahn_hilliard"])
def test_k_ge_5_at_width_128_is_layer_major(kind):
    """Two K >= 5 images at height 128 exceed the LDS (as test_kernel_routing_cpu.py::test_k_ge_5_backward)."""
    assert _name(_net("feedforward", [128] * 3), kind) == "layer_major"
    assert _name(_net("feedforward", [64] * 3), kind) == "jet_kernel_wide"


def test_layer_major_descriptors_and_sets_without_a_coef_unit():
    assert _name(_headline(), "kdv") == "layer_major"                 # (1, 3): no COEF unit
    assert _name(_net("feedforward", [64] * 3), "kdv") == "layer_major"
    for prog in (_net("resnet", [64] * 5, num_blocks=2), _net("attention", [64], num_blocks=1),
                 _net("feedforward", [64] * 3, layer_norm=True), _net("feedforward", [160] * 3)):
        assert _name(prog, "burgers") == "layer_major", prog.arch
    flagged = _headline()
    flagged.set_layer_major(True)
    assert _name(flagged, "burgers") == "layer_major"
    # a 2-D descriptor runs stream set (1, 0): no COEF unit
    prog2 = _net("feedforward", [64] * 3, input_dim=3)
    assert E.inverse_kernel_name(prog2, E.pde_desc("burgers", 2, [0.02]), 100) == "layer_major"


@pytest.mark.parametrize("N", [1, 16, 17, 4900, 49729])
def test_slab_row_did_not_grow(N):
    """The two coefficient sums sit in the padding of the loss-sum slot: same workspace as the forward-mode call."""
    prog = _headline()
    want = _lib.load().pinn_workspace_bytes(ctypes.byref(prog.desc), N, 1, 2, 1)
    assert want > 0
    assert _inv_bytes(prog, "burgers", N) == want
    prog.set_deterministic(True)
    assert _inv_bytes(prog, "burgers", N) == _lib.load().pinn_workspace_bytes(ctypes.byref(prog.desc), N, 1, 2, 1)


@pytest.mark.parametrize("N", [17, 4900])
def test_layer_major_routes_are_sized_for_the_layer_major_engine(N):
    cases = [(_headline(), "kdv"), (_net("feedforward", [128] * 3), "wave"), (_net("feedforward", [128] * 3), "cahn_hilliard"),
             (_net("resnet", [64] * 5, num_blocks=2), "burgers"), (_net("attention", [64], num_blocks=1), "heat")]
    for prog, kind in cases:
        assert _name(prog, kind, N) == "layer_major"
        got = _inv_bytes(prog, kind, N)
        assert got == _lm_bytes(prog, kind, N) and got > 0, (prog.arch, kind)
    flagged = _headline()
    flagged.set_layer_major(True)
    assert _inv_bytes(flagged, "burgers", N) == _lib.load().pinn_workspace_bytes(ctypes.byref(flagged.desc), N, 1, 2, 1)


def test_bad_queries_are_refused():
    prog = _headline()
    with pytest.raises(_lib.JetLibraryError):
        _name(prog, "burgers", N=0)
    assert _inv_bytes(prog, "burgers", 0) == 0
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    assert lib.pinn_inverse_kernel_name(ctypes.byref(prog.desc), None, 10, buf, len(buf)) != 0
    assert lib.pinn_inverse_kernel_name(ctypes.byref(prog.desc), ctypes.byref(_pd("burgers")), 10, None, 0) != 0


def test_existing_queries_keep_their_behaviour():
    """pinn_kernel_name / pinn_workspace_bytes do not know about the COEF units; backward = 3 stays an error."""
    prog = _headline()
    assert _lib.kernel_name(prog, 4900, 1, 2, 1) == "jet_kernel_u16"
    with pytest.raises(_lib.JetLibraryError):
        _lib.kernel_for(prog, 4900, 1, 2, 3)
