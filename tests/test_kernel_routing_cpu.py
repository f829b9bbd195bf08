"""CPU test (no GPU): which kernel a call takes, as `pinn_kernel_for` reports it.

The query makes the same decisions as the launch path (pinn_abi.hip: use_wide, wide_grid, wide_flush and
jet_kernel_wide.h: jet_wide_variant), so these tables pin the routing of every descriptor class to the fused tile-major
kernel's compiled variants (image height `hmax`, first-layer k-tiles `na0`) or to the layer-major engine.  Without a
device the CU count falls back to 256 (MI355X), which sizes the grid."""

import pytest

import pinnrl_amd  # noqa: F401
from pinnrl_amd import _lib
from pinnrl_amd import engine as E

SETS = [(0, 0), (1, 0), (1, 1), (1, 2), (1, 3), (1, 4), (2, 0), (2, 2)]
CUS = 256


def _net(arch, widths, act="tanh", input_dim=2, mapping_size=0, **kw):
    """Descriptor only: the query reads no tensor."""
    return E.NetProgram(arch, act, input_dim, list(widths) + [1], [], [], mapping_size=mapping_size,
                        omega_0=5.0 if arch == "siren" else 0.0, **kw)


def _route(prog, nt, nx, backward, N=100):
    return _lib.kernel_for(prog, N, nt, nx, backward)


@pytest.mark.parametrize("nt,nx", SETS)
@pytest.mark.parametrize("width", [32, 64, 96, 128])
def test_stream_sets_and_widths(nt, nx, width):
    K = 1 + nt + nx
    prog = _net("feedforward", [width] * 3)
    f = _route(prog, nt, nx, 0)
    assert f["engine"] == "tile_major" and (f["time_order"], f["space_order"], f["backward"]) == (nt, nx, 0)
    assert (f["hmax"], f["na0"]) == ((64, 2) if width <= 64 else (128, 4))
    assert f["act_family"] == _lib.ACT["tanh"]
    b = _route(prog, nt, nx, 1)
    if width <= 64:
        assert b["engine"] == "tile_major" and (b["hmax"], b["na0"], b["backward"]) == (64, 2, 1)
    elif K >= 5:  # the reverse sweep's two K-stream images at height 128 exceed the 160 KB of LDS
        assert b["engine"] == "layer_major" and b["hmax"] == -1
    else:  # first MFMA layer's input is the 96 / 128-wide first hidden layer: > 64
        assert b["engine"] == "tile_major" and (b["hmax"], b["na0"]) == (128, 4)


@pytest.mark.parametrize("depth,engine", [(11, "tile_major"), (12, "layer_major")])
def test_k4_backward_at_128_fills_the_lds_at_11_layers(depth, engine):
    """K = 4, width 128, reverse sweep: 11 MFMA layers use exactly 163 840 bytes of LDS; 12 do not fit."""
    prog = _net("feedforward", [128] * (depth + 1))  # first Linear (the encoding) + `depth` MFMA layers
    b = _route(prog, 1, 2, 1)
    assert b["engine"] == engine
    if engine == "tile_major":
        assert (b["hmax"], b["na0"]) == (128, 4)
    assert _route(prog, 1, 2, 0)["engine"] == "tile_major"  # one image only: the forward fits either way
    fprog = _net("fourier", [128] * depth, mapping_size=16)
    assert _route(fprog, 1, 2, 1)["engine"] == engine
    assert _route(fprog, 2, 0, 1)["engine"] == "tile_major"  # K = 3: the images are smaller


@pytest.mark.parametrize("nt,nx", [(1, 3), (2, 2), (1, 4)])
def test_k_ge_5_backward(nt, nx):
    for arch, widths, ms in [("fourier", [128] * 3, 32), ("feedforward", [128] * 3, 0), ("siren", [64, 128, 128], 0)]:
        assert _route(_net(arch, widths, mapping_size=ms), nt, nx, 1)["engine"] == "layer_major"
    for arch, widths, ms in [("fourier", [64] * 3, 16), ("feedforward", [64] * 3, 0), ("siren", [64] * 3, 0)]:
        b = _route(_net(arch, widths, mapping_size=ms), nt, nx, 1)
        assert b["engine"] == "tile_major" and (b["hmax"], b["na0"]) == (64, 2)


def test_first_layer_k_tiles():
    """na0 of the backward variant at height 128: 2 when the first MFMA layer reads <= 64 features, else 4."""
    cases = [(_net("fourier", [128] * 3, mapping_size=32), 2),   # 64 Fourier features -> 128 (the headline network)
             (_net("fourier", [128] * 3, mapping_size=64), 4),   # 128 features
             (_net("fourier", [128] * 3, mapping_size=16), 2),   # 32 features
             (_net("feedforward", [64, 128, 128]), 2),
             (_net("feedforward", [128, 128, 128]), 4),
             (_net("siren", [64, 128, 128], act="sin"), 2)]
    for prog, na0 in cases:
        b = _route(prog, 1, 2, 1)
        assert b["engine"] == "tile_major" and (b["hmax"], b["na0"]) == (128, na0)
        f = _route(prog, 1, 2, 0)
        assert (f["hmax"], f["na0"]) == (128, 4)  # forward: one variant at height 128
    # 32 Fourier features into width 64: the image height is 64 and so is the variant
    b = _route(_net("fourier", [64] * 3, mapping_size=16), 1, 2, 1)
    assert (b["hmax"], b["na0"]) == (64, 2)
    # 128 Fourier features into width 64: the feature image sets the height
    b = _route(_net("fourier", [64] * 3, mapping_size=64), 1, 2, 1)
    assert (b["hmax"], b["na0"]) == (128, 4)


def test_layer_major_descriptors():
    lm = [_net("feedforward", [160] * 3), _net("feedforward", [33] * 3), _net("fourier", [128] * 3, mapping_size=80),
          _net("feedforward", [64] * 3, layer_norm=True), _net("resnet", [64] * 5, num_blocks=2),
          _net("attention", [64], num_blocks=1)]
    flagged = _net("fourier", [128] * 3, mapping_size=32)
    flagged.set_layer_major(True)
    lm.append(flagged)
    for prog in lm:
        for backward in (0, 1, 2):
            r = _route(prog, 1, 2, backward)
            assert r["engine"] == "layer_major", (prog.arch, backward)
            assert (r["hmax"], r["na0"], r["grid"], r["act_family"]) == (-1, -1, -1, -1)
            assert r["flush"] is None and not r["default_mfma_form"]


@pytest.mark.parametrize("nt,nx", SETS)
def test_input_cotangents_are_always_layer_major(nt, nx):
    prog = _net("fourier", [64] * 3, mapping_size=16)
    assert _route(prog, nt, nx, 1)["engine"] == "tile_major"
    assert _route(prog, nt, nx, 2)["engine"] == "layer_major"


def test_activation_families():
    """leaky_relu and identity run the relu unit; siren the sin unit."""
    for act, fam in [("tanh", "tanh"), ("gelu", "gelu"), ("sigmoid", "sigmoid"), ("relu", "relu"),
                     ("leaky_relu", "relu"), ("identity", "relu")]:
        for prog in (_net("feedforward", [64] * 3, act=act), _net("fourier", [64] * 3, act=act, mapping_size=16)):
            assert _route(prog, 1, 2, 1)["act_family"] == _lib.ACT[fam]
    assert _route(_net("siren", [64] * 3, act="sin"), 1, 2, 1)["act_family"] == _lib.ACT["sin"]
    # a single hidden layer (no MFMA layer): the first Linear's activation picks the unit
    assert _route(_net("feedforward", [64], act="gelu"), 1, 2, 1)["act_family"] == _lib.ACT["gelu"]


@pytest.mark.parametrize("N", [1, 32, 33, 8 * 32, 8 * 32 + 1, 256 * 32, 256 * 32 + 1, 49729])
def test_grid_is_min_of_cus_and_tiles(N):
    prog = _net("fourier", [128] * 3, mapping_size=32)
    tiles = (N + 31) // 32
    for backward in (0, 1):
        assert _route(prog, 1, 2, backward, N=N)["grid"] == min(CUS, tiles)


def test_flush_forms():
    """n_layers <= 3 (every MFMA layer keeps its dW tiles in registers): store flush; deeper networks: direct atomics for
    a grid of <= 8 workgroups, the two-level flush above that; PINN_FLAG_DETERMINISTIC: the slab (store flush kept)."""
    shallow = _net("fourier", [128] * 2, mapping_size=32)   # n_layers 2
    three = _net("fourier", [128] * 3, mapping_size=32)     # n_layers 3
    deep = _net("fourier", [128] * 4, mapping_size=32)      # n_layers 4
    ff_deep = _net("feedforward", [64] * 5)                 # first Linear + n_layers 4
    for prog in (shallow, three):
        for N in (10, 8 * 32 + 1, 16401):
            assert _route(prog, 1, 2, 1, N=N)["flush"] == "store"
    for prog in (deep, ff_deep):
        assert _route(prog, 1, 2, 1, N=8 * 32)["flush"] == "direct"     # 8 tiles
        assert _route(prog, 1, 2, 1, N=8 * 32 + 1)["flush"] == "two_level"
        assert _route(prog, 1, 2, 1, N=16401)["flush"] == "two_level"
        prog.set_deterministic(True)
        for N in (10, 8 * 32 + 1, 16401):
            assert _route(prog, 1, 2, 1, N=N)["flush"] == "deterministic"
            assert _route(prog, 1, 2, 0, N=N)["flush"] == "deterministic"  # the loss sum of a forward launch
        prog.set_deterministic(False)
        assert _route(prog, 1, 2, 0, N=16401)["flush"] == "direct"
    three.set_deterministic(True)
    assert _route(three, 1, 2, 1, N=16401)["flush"] == "store"


def test_query_agrees_with_workspace_sizing():
    """pinn_workspace_bytes sizes the engine the query names: zero scratch for a forward tile-major call, none of the
    layer-major engine's packed records."""
    import ctypes

    lib = _lib.load()
    for prog in (_net("fourier", [128] * 3, mapping_size=32), _net("feedforward", [64] * 3)):
        assert _route(prog, 1, 2, 0)["engine"] == "tile_major"
        assert lib.pinn_workspace_bytes(ctypes.byref(prog.desc), 4000, 1, 2, 0) == 0
        prog.set_layer_major(True)
        assert lib.pinn_workspace_bytes(ctypes.byref(prog.desc), 4000, 1, 2, 0) > 0
        prog.set_layer_major(False)


def test_bad_queries_are_refused():
    prog = _net("feedforward", [64] * 3)
    with pytest.raises(ValueError):
        _route(prog, 3, 0, 0)
    with pytest.raises(NotImplementedError):
        _route(prog, 2, 1, 0)  # stream set (2, 1) is not compiled
    with pytest.raises(_lib.JetLibraryError):
        _route(prog, 1, 2, 0, N=0)
    with pytest.raises(_lib.JetLibraryError):
        _route(prog, 1, 2, 3)
