"""Component launches along a direction (`component=k, direction=d` of engine.jets_forward / jets_backward /
jets_backward_inputs) against fp64: the combination a coupled system with mixed derivatives rests on (`TermPDESystemMixed`:
field k's launch along e_a + e_b).

Both are properties of the launch descriptor and no new model is needed: output k of a C-output network is the one-output
network built from row k of the output layer (tests/test_components_gpu.py), and its jets along a direction are the axis-0 jets
of the exactly sheared network (tests/test_direction_jets_gpu.py's `_reference` on tests/direction_model.py).  C = 3, input_dim 4
(three space axes), feedforward of width 30 (rows of the output weight only 4-byte aligned) and fourier of width 32, the
directions (1, 1, 0) and (0, 1, 1) on the set (0, 2), N in {1, 33, 513}.  Bars and the per-point measure are those of
tests/test_components_gpu.py: 1e-5 for u and the weight gradient, 2e-5 for a derivative stream and the input cotangents,
per-point quantities scaled by their root mean square over the 513-point population.  The rows != k of the output layer's
gradient slots keep a sentinel bit for bit."""

import dataclasses

import pytest
import torch

import jet_model as JM
from conftest import rel_l2
from hip_helpers import check_tensors, program_from_spec
from test_axis_jets_gpu import TOL, _AxisView
from test_components_gpu import SENTINEL, _component
from test_direction_jets_gpu import _reference

pytestmark = pytest.mark.gpu

C = 3
DIN = 4
POINTS = (1, 33, 513)
NT, NX = 0, 2
LINES = ((1, 1, 0), (0, 1, 1))
FAMILIES = [("feedforward", 30), ("fourier", 32)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _network(family, width, seed=13):
    """(spec with C outputs, its fp32 state_dict, the one-output spec, the first-layer key, the two output-layer keys)."""
    import autoencoder_model as AM
    import oracle as O

    spec = O.ArchSpec(family, input_dim=DIN, hidden_dim=width, num_layers=3 if family == "fourier" else 2, activation="tanh",
                      mapping_size=12, scale=1.5, layer_norm=False, output_dim=C)
    sd = AM.perturb(O.init_state_dict(spec, seed=seed), seed + 1, 0.2)
    first = {"feedforward": "model.layers.0.weight", "fourier": "model.fourier.B"}[family]
    keys = list(sd)
    assert sd[keys[-2]].shape == (C, width) and sd[keys[-1]].shape == (C,)
    return spec, sd, dataclasses.replace(spec, output_dim=1), first, (keys[-2], keys[-1])


def _population(seed, n=POINTS[-1]):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, DIN - 1, generator=g) * 2 - 1
    t = torch.rand(n, 1, generator=g)
    return x, t, torch.randn(1 + NT + NX, n, generator=g)


@pytest.mark.parametrize("family,width", FAMILIES)
def test_component_direction_jets_gradients_and_input_cotangents(family, width, dev):
    from pinnrl_amd import _lib
    from pinnrl_amd import engine as E

    spec, sd, spec1, first, out_keys = _network(family, width)
    prog, _ = program_from_spec(spec, sd, dev)
    assert prog.n_outputs == C and prog.desc.widths[prog.desc.num_linear - 1] == 1
    tol_u, tol_s, tol_g = TOL, 2 * TOL, TOL
    trainable = [k for k in sd if not k.endswith("fourier.B")]
    build64 = lambda s: JM.net_program(spec1, s)  # noqa: E731
    worst = {"u": 0.0, "stream": 0.0, "grad": 0.0, "xg": 0.0, "tg": 0.0}
    npop = POINTS[-1]
    K = 1 + NT + NX
    for line in LINES:
        xp, tp, cp = _population(seed=300 + sum((3 ** c) * v for c, v in enumerate(line)))
        for k in range(C):
            one = _component(sd, out_keys, k)
            pop = _reference(build64, one, first, DIN, line, xp, tp, cp, NX)
            rms = {"jets": [float(pop[0][s].norm()) / npop ** 0.5 for s in range(K)], "xg": float(pop[2].norm()) / npop ** 0.5,
                   "tg": float(pop[3].norm()) / npop ** 0.5}

            def scaled(got, want, scale, N):
                return float((got.double() - want).norm()) / (N ** 0.5 * scale)

            for N in POINTS:
                x, t, cot = xp[:N], tp[:N], cp[:, :N].contiguous()
                jets64, grads64, xg64, tg64 = pop if N == npop else _reference(build64, one, first, DIN, line, x, t, cot, NX)
                xd, td, cd = x.to(dev), t.to(dev), cot.to(dev)
                where = f"{family}/{width} component {k} direction={line} set=({NT},{NX}) N={N}"
                assert _lib.kernel_name(_AxisView(E._launch_desc(prog, 0, line, k)), N, NT, NX, 1) == "layer_major"
                jets = E.jets_forward(prog, xd, td, NT, NX, direction=line, component=k).cpu()
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
                        E.jets_backward(prog, xd, td, NT, NX, cd, flat, direction=line, component=k)
                    else:
                        xg, tg = E.jets_backward_inputs(prog, xd, td, NT, NX, cd, flat, True, True, direction=line, component=k)
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
                               label="component direction weight gradient", tol=tol_g)
                    worst["grad"] = max(worst["grad"], e)
                    assert e <= tol_g, f"{where}: weight gradient ({runner}): {e:.2e}"
                    check_tensors(got, want, f"{where} ({runner})")
    print(f"{family}/{width}: worst " + ", ".join(f"{n_} {v:.2e}" for n_, v in worst.items()))
