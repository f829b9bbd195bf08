"""CPU tests (no GPU) of the autoencoder architecture: the parameter container against the reference's theta_0 and
state_dict layout (fixtures of tools/make_autoencoder_golden.py), the fp64 node model (tests/autoencoder_model.py, the
executable specification of the engine's program) against the fixtures, and the C ABI's descriptor handling."""
import ctypes

import pytest
import torch

import autoencoder_model as AM
from conftest import rel_l2
import pinnrl_amd  # noqa: F401
from pinnrl_amd import _lib
from pinnrl_amd import engine as E
from pinnrl_amd.neural_networks import AutoEncoder, PINNModel

CPU = torch.device("cpu")
SETS = [(0, 0), (1, 0), (1, 1), (1, 2), (1, 3), (1, 4), (2, 0), (2, 2)]


@pytest.fixture(scope="module", params=AM.CASES)
def case(request):
    return AM.load_fixture(request.param)


def _desc(hidden, latent, layer_norm=True, act="relu", num_blocks=None, widths=None):
    """Descriptor only: the queries read no tensor."""
    w = widths if widths is not None else list(hidden) + [latent] + list(hidden)[::-1] + [1]
    return E.NetProgram("autoencoder", act, 2, w, [], [], num_blocks=len(hidden) if num_blocks is None else num_blocks,
                        layer_norm=layer_norm)


def test_theta0_and_state_dict_layout_match_the_reference(case):
    meta, sd, a = case
    torch.manual_seed(meta["seed"])
    model = PINNModel(AM.model_config(meta, CPU), device=CPU)
    assert isinstance(model.model, AutoEncoder)
    got = AM.perturb({k: v.detach() for k, v in model.state_dict().items()}, meta["perturb"]["seed"], meta["perturb"]["scale"])
    assert list(got) == meta["sd_keys"] == list(sd)
    for k in sd:
        assert got[k].shape == sd[k].shape and torch.equal(got[k], sd[k]), k
    assert model.count_parameters() == sum(v.numel() for v in sd.values())
    assert model.count_parameters() == a["grad64_exact"].shape[0] == a["grad64"].shape[0]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(torch.zeros(4, 2))


def test_program_spec_is_the_abi_encoding(case):
    meta, sd, a = case
    m = meta["model"]
    model = PINNModel(AM.model_config(meta, CPU), device=CPU)
    prog = model.program()
    d, n = prog.desc, len(m["hidden_dims"])
    assert (d.arch, d.num_blocks, d.num_linear) == (_lib.ARCH["autoencoder"], n, 2 * n + 2) and _lib.ARCH["autoencoder"] == 5
    assert [d.widths[i] for i in range(d.num_linear)] == m["hidden_dims"] + [m["latent_dim"]] + m["hidden_dims"][::-1] + [1]
    assert bool(d.flags & _lib.PINN_FLAG_LAYER_NORM) == m["layer_norm"] and d.activation == _lib.ACT[m["activation"]]
    assert prog.num_tensors == len(sd) == _lib.load().pinn_num_tensors(ctypes.byref(d))
    assert ["model." + k for k in prog.names] == meta["sd_keys"] and all(prog.trainable)
    # flops_per_point walks the widths: 2 * sum(in * out) over the 2 n + 2 Linears
    dims = [m["input_dim"]] + [d.widths[i] for i in range(d.num_linear)]
    assert prog.flops_per_point() == 2 * sum(i * o for i, o in zip(dims[:-1], dims[1:]))


def test_node_model_reproduces_the_fixture(case):
    meta, sd, a = case
    jets, r, loss, flat = AM.node_model_outputs(meta, sd, torch.from_numpy(a["x"]), torch.from_numpy(a["t"]))
    K = 1 + sum(meta["streams"])
    assert a["jets64"].shape == (K, meta["n_points"])
    for s in range(K):
        assert rel_l2(jets[s], a["jets64"][s]) <= 1e-12, s
    assert rel_l2(r, a["residual64_exact"]) <= 1e-12
    assert abs(loss - float(a["loss64_exact"])) <= 1e-12 * abs(float(a["loss64_exact"]))
    assert rel_l2(flat, a["grad64_exact"]) <= 1e-12
    # the reference's own gradient is exact only without LayerNorm (torch's fused layer_norm, differentiated three times)
    d = rel_l2(a["grad64"], a["grad64_exact"])
    assert d == pytest.approx(meta["grad64_vs_exact"]["total"], rel=1e-9, abs=1e-300)
    assert (d > 1e-4) == meta["model"]["layer_norm"]


@pytest.mark.parametrize("layer_norm", [True, False])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_num_tensors(n, layer_norm):
    prog = _desc([40, 33, 64][:n], 16, layer_norm)
    assert _lib.load().pinn_num_tensors(ctypes.byref(prog.desc)) == (8 * n + 4 if layer_norm else 4 * n + 4)
    # the module list of the container has exactly that many entries in its state_dict
    net = AutoEncoder({"input_dim": 2, "hidden_dims": [40, 33, 64][:n], "latent_dim": 16, "layer_norm": layer_norm, "output_dim": 1})
    assert len(net.state_dict()) == (8 * n + 4 if layer_norm else 4 * n + 4)
    lin, lns = AM.linear_names(n, layer_norm, prefix="")
    want = []
    for a, b in zip(lin, lns):
        want += [a + ".weight", a + ".bias"] + ([b + ".weight", b + ".bias"] if b else [])
    assert list(net.state_dict()) == want


@pytest.mark.parametrize("nt,nx", SETS)
def test_always_the_layer_major_engine(nt, nx):
    lib = _lib.load()
    for prog in (_desc([124, 248, 124], 64), _desc([32, 64], 16, act="tanh"), _desc([64], 32, False, act="tanh"),
                 _desc([128, 128], 128, False, act="tanh")):  # the last two: widths the tile-major kernels would take in an MLP
        for backward in (0, 1, 2):
            info = _lib.kernel_for(prog, 1000, nt, nx, backward)
            assert info["engine"] == "layer_major" and info["hmax"] == -1
            assert _lib.kernel_name(prog, 1000, nt, nx, backward) == "layer_major"
            assert lib.pinn_workspace_bytes(ctypes.byref(prog.desc), 1000, nt, nx, backward) > 0
    for kind in ("burgers", "kdv", "allen_cahn"):
        pd = E.pde_desc(kind, 1, [0.1])
        prog = _desc([128, 128], 128, False, act="tanh")
        assert E.inverse_kernel_name(prog, pd, 1000) == "layer_major"
        assert lib.pinn_inverse_workspace_bytes(ctypes.byref(prog.desc), ctypes.byref(pd), 1000) > 0


def test_bad_descriptors_are_refused_with_the_documented_codes():
    lib = _lib.load()

    def rc_of(prog):
        rc = lib.pinn_num_tensors(ctypes.byref(prog.desc))
        info = _lib.PinnKernelInfo()
        assert lib.pinn_kernel_for(ctypes.byref(prog.desc), 100, 1, 2, 1, ctypes.byref(info)) == rc
        assert lib.pinn_workspace_bytes(ctypes.byref(prog.desc), 100, 1, 2, 1) == 0
        return rc, lib.pinn_last_error()

    BAD_DESC, UNSUPPORTED = -1, -2
    assert rc_of(_desc([32, 64], 16, num_blocks=3))[0] == BAD_DESC          # num_linear = 6, 2 n + 2 = 8
    assert rc_of(_desc([32, 64], 16, num_blocks=1))[0] == BAD_DESC
    assert rc_of(_desc([32, 64], 16, num_blocks=-1))[0] == BAD_DESC
    rc, msg = rc_of(_desc([], 16))                                         # n = 0: Linear(2, 16), Linear(16, 1)
    assert rc == UNSUPPORTED and b"linear" in msg
    assert rc_of(_desc([32], 16, widths=[32, 16, 32, 2]))[0] == UNSUPPORTED   # output_dim must be 1
    assert rc_of(_desc([32], 16, widths=[32, 0, 32, 1]))[0] == UNSUPPORTED    # latent width outside [1, 1024]
    assert rc_of(_desc([32], 16, widths=[32, 16, 1025, 1]))[0] == UNSUPPORTED
    ok = _desc([11] * 11, 5)                                                # PINN_MAX_LINEAR = 24 caps n at 11
    assert lib.pinn_num_tensors(ctypes.byref(ok.desc)) == 92
    with pytest.raises(NotImplementedError, match="24 Linear"):
        _desc([11] * 12, 5)


def test_short_weight_table_is_refused_before_any_entry_is_read():
    lib = _lib.load()
    prog = _desc([32, 64], 16)
    n = lib.pinn_num_tensors(ctypes.byref(prog.desc))
    assert n == 20
    bogus = (ctypes.c_void_p * 3)(1, 2, 3)  # must never be read
    outs = (ctypes.c_void_p * 2)(8, 8)
    for bad_n in (3, n - 1, n + 1, 0):
        rc = lib.pinn_jet_forward(ctypes.byref(prog.desc), bogus, bad_n, 16, 16, 5, 1, 0, outs, None, 0, None)
        assert rc == -1 and b"entries" in lib.pinn_last_error(), (bad_n, rc, lib.pinn_last_error())


def _cfg(**over):
    meta = {"model": dict(input_dim=2, hidden_dims=[32, 64], latent_dim=16, activation="tanh", layer_norm=True, dropout=0.0,
                          output_dim=1)}
    meta["model"].update(over)
    if not meta["model"]["hidden_dims"]:
        cfg = AM.model_config({"model": dict(meta["model"], hidden_dims=[1])}, CPU)
        cfg.model.hidden_dims = []
        return cfg
    return AM.model_config(meta, CPU)


def test_dropout_and_the_purely_linear_model_raise():
    model = PINNModel(_cfg(dropout=0.1), device=CPU)
    assert any(isinstance(mod, torch.nn.Dropout) for mod in model.model.encoder)  # the container follows the reference
    with pytest.raises(NotImplementedError, match="dropout"):
        model.program()
    linear = PINNModel(_cfg(hidden_dims=[]), device=CPU)
    assert len(linear.state_dict()) == 4
    with pytest.raises(NotImplementedError, match="purely linear"):
        linear.program()


def test_latent_dim_left_unset_raises_like_the_reference():
    """ModelConfig.latent_dim is None unless set; config.get("latent_dim", 16) returns that None, and nn.Linear refuses it."""
    cfg = _cfg()
    cfg.model.latent_dim = None
    with pytest.raises(TypeError):
        PINNModel(cfg, device=CPU)
    net = AutoEncoder({"input_dim": 2, "output_dim": 1})  # a plain dict without the keys does reach the defaults
    assert (net.latent_dim, net.hidden_dims) == (16, [32, 64])


def test_encode_and_decode_are_the_module_loops():
    torch.manual_seed(0)
    net = AutoEncoder({"input_dim": 2, "hidden_dims": [8, 12], "latent_dim": 5, "activation": "tanh", "output_dim": 1})
    inp = torch.rand(7, 2)
    z = net.encode(inp)
    assert z.shape == (7, 5) and net.decode(z).shape == (7, 1)
    h = inp
    for mod in list(net.encoder) + list(net.decoder):
        h = mod(h)
    assert torch.equal(net.decode(z), h)
