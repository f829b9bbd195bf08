"""CPU test (no GPU): which reverse launches take the 16-point fused kernel (jet_kernel_u16.h).

`pinn_kernel_name` names the kernel a call takes; `pinn_kernel_for` keeps reporting the fused engine's fields as before
(engine, hmax, na0, grid, flush), and so does `pinn_workspace_bytes`."""

import pytest

import pinnrl_amd  # noqa: F401
from pinnrl_amd import _lib
from pinnrl_amd import engine as E

CUS = 256


def _net(arch, widths, act="tanh", input_dim=2, mapping_size=0, **kw):
    return E.NetProgram(arch, act, input_dim, list(widths) + [1], [], [], mapping_size=mapping_size,
                        omega_0=5.0 if arch == "siren" else 0.0, **kw)


def _headline():
    """bench.py's network: fourier 4 x 128 behind 32 Fourier frequencies (64 features), three MFMA layers."""
    return _net("fourier", [128, 128, 128], mapping_size=32)


def _u16_built(nt, nx, fam):
    return f"jet_u16_{nt}_{nx}_{_lib.ACT[fam]}:" not in _lib.build_info()


def _name(prog, nt, nx, bwd, N=49_729):
    return _lib.kernel_name(prog, N, nt, nx, bwd)


def test_headline_takes_the_16_point_kernel():
    assert _u16_built(1, 2, "tanh"), _lib.build_info()
    assert _name(_headline(), 1, 2, 1) == "jet_kernel_u16"


@pytest.mark.parametrize("nt,nx", [(0, 0), (1, 0), (1, 1), (1, 2), (2, 0)])
@pytest.mark.parametrize("fam", ["tanh", "sin", "gelu", "sigmoid", "relu"])
def test_stream_sets_and_families(nt, nx, fam):
    prog = _net("siren", [64, 128, 128]) if fam == "sin" else _net("fourier", [128, 128, 128], act=fam, mapping_size=32)
    want = "jet_kernel_u16" if _u16_built(nt, nx, fam) else "jet_kernel_wide"
    assert _name(prog, nt, nx, 1) == want


def test_opt_out_flag_keeps_the_32_point_kernel():
    prog = _headline()
    prog.desc.flags |= _lib.PINN_FLAG_WIDE_TILE32
    assert _name(prog, 1, 2, 1) == "jet_kernel_wide"


def test_forward_only_calls_of_the_same_network_take_it_too():
    """Forward-only launches of a descriptor whose reverse launches take the 16-point kernel run its forward code, so
    that per-point results do not depend on whether the call has a reverse sweep; the flag opts both out."""
    prog = _headline()
    assert _name(prog, 1, 2, 0) == "jet_kernel_u16"
    prog.desc.flags |= _lib.PINN_FLAG_WIDE_TILE32
    assert _name(prog, 1, 2, 0) == "jet_kernel_wide"


@pytest.mark.parametrize("case", ["forward_k5", "four_layers", "k5", "first_layer_128", "height_64", "backward_inputs"])
def test_other_calls_keep_their_kernel(case):
    prog, nt, nx, bwd, want = _headline(), 1, 2, 1, "jet_kernel_wide"
    if case == "forward_k5":
        nt, nx, bwd = 1, 3, 0
    elif case == "four_layers":
        prog = _net("fourier", [128] * 4, mapping_size=32)
    elif case == "k5":
        nt, nx, want = 1, 3, "layer_major"  # K = 5 reverse sweep at height 128 takes the layer-major engine, as before
    elif case == "first_layer_128":
        prog = _net("feedforward", [128] * 3)
    elif case == "height_64":
        prog = _net("fourier", [64] * 3, mapping_size=16)
    elif case == "backward_inputs":
        bwd, want = 2, "layer_major"
    assert _name(prog, nt, nx, bwd) == want


@pytest.mark.parametrize("N", [1, 16, 17, 4_900, 49_729])
def test_workspace_size_does_not_depend_on_the_kernel(N):
    """pinn_workspace_bytes reports the 32-point kernel's tape + slab whichever kernel runs, so that
    PINN_FLAG_WIDE_TILE32 can be toggled on one workspace; the 16-point launch itself uses only the slab."""
    prog = _headline()
    grid = min(CUS, (N + 31) // 32)
    pad = lambda n: (n + 3) // 4 * 4  # noqa: E731
    stride = sum(pad(n) for n in [128 * 64, 128, 128 * 128, 128, 128 * 128, 128, 128, 1, 1])
    tape = 4 * 4 * 16 * 256 * 4 * grid  # (3 layers + encoding) x K = 4 x 16 registers x 256 threads x 4 B
    assert _lib.load().pinn_workspace_bytes(_ref(prog), N, 1, 2, 1) == tape + 4 * stride * grid
    prog.desc.flags |= _lib.PINN_FLAG_WIDE_TILE32
    assert _lib.load().pinn_workspace_bytes(_ref(prog), N, 1, 2, 1) == tape + 4 * stride * grid


def _ref(prog):
    import ctypes

    return ctypes.byref(prog.desc)


def test_kernel_for_fields_are_unchanged():
    """The query's fields for a 16-point launch are those of the fused engine's 32-point variant it replaces."""
    prog = _headline()
    u = _lib.kernel_for(prog, 49_729, 1, 2, 1)
    prog.desc.flags |= _lib.PINN_FLAG_WIDE_TILE32
    t = _lib.kernel_for(prog, 49_729, 1, 2, 1)
    assert u == t
    assert (u["engine"], u["hmax"], u["na0"], u["grid"], u["flush"]) == ("tile_major", 128, 2, CUS, "store")
