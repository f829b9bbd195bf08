"""Component launches of a multi-output network (`component=` of engine.jets_forward / jets_backward / jets_backward_inputs)
against fp64.

Output k of a C-output network is the one-output network whose output layer is row k of the output weight and entry k of
the output bias, so the truth needs no new model: tests/jet_model.py on that one-output network (and, along axis 1, on its
column-swapped form, as tests/test_axis_jets_gpu.py does).  input_dim 3, C = 3; feedforward of width 30 (rows of the output
weight are then only 4-byte aligned), feedforward with LayerNorm, fourier, resnet; N in {1, 33, 513}; the set (1, 2) on axis 0
and the set (0, 2) on axis 1.  Bars and the per-point measure are those of tests/test_axis_jets_gpu.py: 1e-5 for u and the
weight gradient, 2e-5 for a derivative stream and the input cotangents (5e-5 with LayerNorm), per-point quantities scaled
by their root mean square over the 513-point population.  The rows != k of the output layer's gradient slots keep a
sentinel bit for bit."""

import dataclasses

import pytest
import torch

import jet_model as JM
from conftest import rel_l2
from hip_helpers import check_tensors, program_from_spec
from test_axis_jets_gpu import TOL, _AxisView, _reference

pytestmark = pytest.mark.gpu

C = 3
DIN = 3
POINTS = (1, 33, 513)
LAUNCHES = ((0, 1, 2), (1, 0, 2))  # (axis, nt, nx)
FAMILIES = [("feedforward", 30), ("feedforward_ln", 32), ("fourier", 32), ("resnet", 32)]
SENTINEL = 12345.678


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _network(family, width, seed=11):
    """(spec with C outputs, its fp32 state_dict, the one-output spec, the first-layer key, the two output-layer keys)."""
    import autoencoder_model as AM
    import oracle as O

    arch = "feedforward" if family.startswith("feedforward") else family
    spec = O.ArchSpec(arch, input_dim=DIN, hidden_dim=width, num_layers=3 if arch == "fourier" else 2, activation="tanh",
                      mapping_size=12, scale=1.5, num_blocks=2 if arch == "resnet" else None, layer_norm=family == "feedforward_ln",
                      output_dim=C)
    sd = AM.perturb(O.init_state_dict(spec, seed=seed), seed + 1, 0.2)
    first = {"feedforward": "model.layers.0.weight", "fourier": "model.fourier.B", "resnet": "model.input_layer.weight"}[arch]
    keys = list(sd)
    assert sd[keys[-2]].shape == (C, width) and sd[keys[-1]].shape == (C,)
    return spec, sd, dataclasses.replace(spec, output_dim=1), first, (keys[-2], keys[-1])


def _component(sd, out_keys, k):
    """The one-output network that is output k."""
    one = dict(sd)
    one[out_keys[0]] = sd[out_keys[0]][k : k + 1].clone()
    one[out_keys[1]] = sd[out_keys[1]][k : k + 1].clone()
    return one


def _population(nt, nx, seed, n=POINTS[-1]):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, DIN - 1, generator=g) * 2 - 1
    t = torch.rand(n, 1, generator=g)
    return x, t, torch.randn(1 + nt + nx, n, generator=g)


@pytest.mark.parametrize("family,width", FAMILIES)
def test_component_jets_gradients_and_input_cotangents(family, width, dev):
    from pinnrl_amd import _lib
    from pinnrl_amd import engine as E

    spec, sd, spec1, first, out_keys = _network(family, width)
    prog, _ = program_from_spec(spec, sd, dev)
    assert prog.n_outputs == C and prog.desc.widths[prog.desc.num_linear - 1] == 1
    ln = family in ("feedforward_ln", "resnet")
    tol_u, tol_s, tol_g = TOL, (5e-5 if ln else 2 * TOL), TOL
    trainable = [k for k in sd if not k.endswith("fourier.B")]
    build64 = lambda s: JM.net_program(spec1, s)  # noqa: E731
    worst = {"u": 0.0, "stream": 0.0, "grad": 0.0, "xg": 0.0, "tg": 0.0}
    npop = POINTS[-1]
    for a, nt, nx in LAUNCHES:
        K = 1 + nt + nx
        xp, tp, cp = _population(nt, nx, seed=100 * a + 10 * nt + nx)
        for k in range(C):
            one = _component(sd, out_keys, k)
            pop = _reference(build64, one, first, DIN, a, xp, tp, cp, nt, nx)
            rms = {"jets": [float(pop[0][s].norm()) / npop ** 0.5 for s in range(K)], "xg": float(pop[2].norm()) / npop ** 0.5,
                   "tg": float(pop[3].norm()) / npop ** 0.5}

            def scaled(got, want, scale, N):
                return float((got.double() - want).norm()) / (N ** 0.5 * scale)

            for N in POINTS:
                x, t, cot = xp[:N], tp[:N], cp[:, :N].contiguous()
                jets64, grads64, xg64, tg64 = pop if N == npop else _reference(build64, one, first, DIN, a, x, t, cot, nt, nx)
                xd, td, cd = x.to(dev), t.to(dev), cot.to(dev)
                where = f"{family}/{width} component {k} axis={a} set=({nt},{nx}) N={N}"
                assert _lib.kernel_name(_AxisView(E._launch_desc(prog, a, None, k)), N, nt, nx, 1) == "layer_major"
                jets = E.jets_forward(prog, xd, td, nt, nx, axis=a, component=k).cpu()
                assert jets.shape == (K, N)
                for s in range(K):
                    e = scaled(jets[s], jets64[s], rms["jets"][s], N)
                    worst["u" if s == 0 else "stream"] = max(worst["u" if s == 0 else "stream"], e)
                    assert e <= (tol_u if s == 0 else tol_s), f"{where}: jet stream {s}: {e:.2e}"
                # the gradient: every tensor; of the output layer row k, the other rows keep the sentinel bit for bit
                for runner in ("backward", "backward_inputs"):
                    flat = E.new_flat_grad(prog, dev)
                    by = dict(zip(sd, E.split_flat_grad(prog, flat)))
                    for j in range(C):
                        if j != k:
                            by[out_keys[0]][j].fill_(SENTINEL)
                            by[out_keys[1]][j].fill_(SENTINEL)
                    if runner == "backward":
                        E.jets_backward(prog, xd, td, nt, nx, cd, flat, axis=a, component=k)
                    else:
                        xg, tg = E.jets_backward_inputs(prog, xd, td, nt, nx, cd, flat, True, True, axis=a, component=k)
                        e_x, e_t = scaled(xg.cpu(), xg64, rms["xg"], N), scaled(tg.cpu(), tg64, rms["tg"], N)
                        worst["xg"], worst["tg"] = max(worst["xg"], e_x), max(worst["tg"], e_t)
                        assert e_x <= tol_s and e_t <= tol_s, f"{where}: x_grad {e_x:.2e}, t_grad {e_t:.2e}"
                    got = {n_: g.detach().cpu() for n_, g in by.items() if g is not None}
                    for j in range(C):
                        if j != k:
                            assert torch.equal(got[out_keys[0]][j], torch.full((width,), SENTINEL)), f"{where}: dW_out row {j} was written"
                            assert float(got[out_keys[1]][j]) == torch.tensor(SENTINEL).item(), f"{where}: db_out entry {j} was written"
                    got[out_keys[0]] = got[out_keys[0]][k : k + 1]
                    got[out_keys[1]] = got[out_keys[1]][k : k + 1]
                    for n_ in trainable:  # parameters no jet depends on: zero
                        grads64.setdefault(n_, torch.zeros_like(one[n_], dtype=torch.float64))
                    want = {n_: grads64[n_] for n_ in trainable}
                    e = rel_l2(torch.cat([got[n_].flatten() for n_ in trainable]), torch.cat([want[n_].flatten() for n_ in trainable]),
                               label="component weight gradient", tol=tol_g)
                    worst["grad"] = max(worst["grad"], e)
                    assert e <= tol_g, f"{where}: weight gradient ({runner}): {e:.2e}"
                    check_tensors(got, want, f"{where} ({runner})")
    print(f"{family}/{width}: worst " + ", ".join(f"{n_} {v:.2e}" for n_, v in worst.items()))


def test_component_out_of_range_raises_before_the_library(dev, monkeypatch):
    from pinnrl_amd import _lib
    from pinnrl_amd import engine as E

    spec, sd, _, _, _ = _network("feedforward", 30)
    prog, _ = program_from_spec(spec, sd, dev)
    x, t = torch.zeros(4, 2, device=dev), torch.zeros(4, 1, device=dev)
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was called"))
    for k in (-1, C):
        with pytest.raises(ValueError, match="component"):
            E.jets_forward(prog, x, t, 0, 0, component=k)
        with pytest.raises(ValueError, match="component"):
            E.jets_backward(prog, x, t, 0, 0, torch.zeros(1, 4, device=dev), torch.zeros(8, device=dev), component=k)
        with pytest.raises(ValueError, match="component"):
            E.jets_backward_inputs(prog, x, t, 0, 0, torch.zeros(1, 4, device=dev), None, True, True, component=k)


def _model(dev, arch="feedforward", output_dim=C, width=30):
    from pinnrl_amd.config import Config, ModelConfig
    from pinnrl_amd.neural_networks import PINNModel

    cfg = Config.__new__(Config)
    cfg.device = torch.device("cpu")
    cfg.model = ModelConfig(input_dim=DIN, hidden_dim=width, output_dim=output_dim, num_layers=2, activation="tanh", architecture=arch)
    cfg.model.hidden_dims, cfg.model.dropout, cfg.model.layer_norm = [width, width], 0.0, False
    torch.manual_seed(5)
    return PINNModel(cfg, device=torch.device("cpu")).to(dev)


def test_model_forward_is_n_by_c_and_differentiable(dev):
    from pinnrl_amd import engine as E

    model = _model(dev)
    g = torch.Generator().manual_seed(2)
    inp = torch.rand(33, DIN, generator=g).to(dev).requires_grad_(True)
    w = torch.randn(33, C, generator=g).to(dev)
    out = model(inp)
    assert out.shape == (33, C) and out.requires_grad
    prog = model.program()
    x, t = inp.detach()[:, :-1], inp.detach()[:, -1:]
    for k in range(C):
        assert torch.equal(out[:, k].detach(), E.jets_forward(prog, x, t, 0, 0, component=k)[0])
        assert torch.equal(model.jets(x, t, 1, 2, component=k).detach(), E.jets_forward(prog, x, t, 1, 2, component=k))
    (out * w).sum().backward()
    flat = E.new_flat_grad(prog, dev)
    ig = torch.zeros(33, DIN, device=dev)
    for k in range(C):
        xg, tg = E.jets_backward_inputs(prog, x, t, 0, 0, w[:, k].reshape(1, -1).contiguous(), flat, True, True, component=k)
        ig += torch.cat([xg, tg], 1)
    for p, want in zip(prog.tensors, E.split_flat_grad(prog, flat)):
        assert p.grad is not None and rel_l2(p.grad.cpu(), want.double().cpu()) <= 1e-6
    assert rel_l2(inp.grad.cpu(), ig.double().cpu()) <= 1e-6
    assert float(prog.tensors[-2].grad.abs().min()) > 0.0  # every row of the output weight received its gradient


def test_one_output_program_is_untouched(dev):
    """C = 1: the program's own descriptor (no copy, no flag), the same kernel name, the same bits with and without the argument."""
    import oracle as O
    from pinnrl_amd import _lib
    from pinnrl_amd import engine as E

    spec = O.ArchSpec("feedforward", input_dim=2, hidden_dim=32, num_layers=3, activation="tanh", layer_norm=False)
    prog, _ = program_from_spec(spec, O.init_state_dict(spec, seed=3), dev)
    prog.set_deterministic(True)
    assert prog.n_outputs == 1 and E._launch_desc(prog, 0, None, 0) is prog.desc
    N = 513
    for bwd in (0, 1):
        assert _lib.kernel_name(_AxisView(E._launch_desc(prog)), N, 1, 2, bwd) == _lib.kernel_name(prog, N, 1, 2, bwd) != "layer_major"
    g = torch.Generator().manual_seed(4)
    x, t = (torch.rand(N, 1, generator=g) * 2 - 1).to(dev), torch.rand(N, 1, generator=g).to(dev)
    cot = torch.randn(4, N, generator=g).to(dev)
    assert torch.equal(E.jets_forward(prog, x, t, 1, 2), E.jets_forward(prog, x, t, 1, 2, component=0))
    f0, f1 = E.new_flat_grad(prog, dev), E.new_flat_grad(prog, dev)
    E.jets_backward(prog, x, t, 1, 2, cot, f0)
    E.jets_backward(prog, x, t, 1, 2, cot, f1, component=0)
    assert torch.equal(f0, f1) and float(f0.abs().max()) > 0.0
    with pytest.raises(ValueError, match="component"):
        E.jets_forward(prog, x, t, 1, 2, component=1)
