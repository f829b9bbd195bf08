"""Jet launches along a direction (PINN_FLAG_SPACE_DIRECTION), and the orders 3 and 4 along a further axis, against the fp64
node model.

The truth is the node model of tests/jet_model.py on the EXACTLY sheared network (tests/direction_model.py in fp64: every
sheared entry is a sum of two or three fp32 numbers, exact in fp64): its axis-0 jets are the exact directional derivatives of
the network as given.  The weight gradient comes from the model's own reverse sweep with the map-gradient columns
un-sheared, the input cotangents from autograd through the shear of the inputs.  An axis is the direction e_a of the same
helpers.  The engine's shear is rounded to fp32 (one add or subtract per entry); measured on the fp64 model that moves every
stream by at most 3.5e-7 relative l2, two orders below the bars, so it has no bar of its own.

Families, widths, bars and the error measure are those of tests/test_axis_jets_gpu.py: 1e-5 for u and the weight gradient, 2e-5
for a derivative stream and the input cotangents, 5e-5 for those of LayerNorm networks; per-point quantities are measured as
|got - want|_2 / (sqrt(N) rms over the 100-point population).  Directions (1,1), (1,-1) at input_dim 3 and (0,1,-1), (1,0,1),
(1,-1,1) at input_dim 4 on the sets (0, 2) and (0, 4); axis 1 at input_dim 3 on (0, 3) and (0, 4); N in {1, 17, 100}."""

import pytest
import torch

import direction_model as DM
import jet_model as JM
from conftest import rel_l2
from test_axis_jets_gpu import FAMILIES, LN_FAMILIES, _AxisView, _network, _population

pytestmark = pytest.mark.gpu

TOL = 1e-5
POINTS = (1, 17, 100)
# (input_dim, line, sets): a line with one non-zero entry is an axis
LINES = ((3, (1, 1), ((0, 2), (0, 4))), (3, (1, -1), ((0, 2), (0, 4))), (4, (0, 1, -1), ((0, 2), (0, 4))),
         (4, (1, 0, 1), ((0, 2), (0, 4))), (4, (1, -1, 1), ((0, 2), (0, 4))), (3, (0, 1), ((0, 3), (0, 4))))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _line_kwargs(line):
    nz = [c for c, v in enumerate(line) if v]
    return {"axis": nz[0]} if len(nz) == 1 else {"direction": line}


def _reference(build64, sd, first, din, line, x, t, cot, NX):
    """fp64 truth on the given points: jets along the line, d<cot, jets>/d(theta), d<cot, jets>/d(x), d<cot, jets>/d(t)."""
    K = 1 + NX
    sd64 = DM.shear_state_dict({k: v.double() for k, v in sd.items()}, first, line)
    inp = torch.cat([x, t], 1).double().requires_grad_(True)
    prog = build64(sd64)
    u, _ = JM.program_forward(prog, DM.shear_inputs(inp, line), 0, NX)  # under autograd: the input cotangents
    pairing = sum((cot[s].double() * u[s][:, 0]).sum() for s in range(K))
    ig, = torch.autograd.grad(pairing, inp)
    with torch.no_grad():  # the node model's own reverse sweep: the weight gradient
        u, tape = JM.program_forward(prog, DM.shear_inputs(inp.detach(), line), 0, NX)
        grads = JM.program_backward(prog, tape, [cot[s].double().unsqueeze(1) for s in range(K)], 0, NX)
    if not first.endswith("fourier.B"):
        grads[first] = DM.unshear_map_grad(grads[first], line)
    return torch.stack([s[:, 0] for s in u]), grads, ig[:, : din - 1], ig[:, din - 1:]


@pytest.mark.parametrize("width", [32, 40])
@pytest.mark.parametrize("family,act", FAMILIES)
def test_jets_gradients_and_input_cotangents_along_a_direction(family, act, width, dev):
    from pinnrl_amd import _lib
    from pinnrl_amd import engine as E

    ln = family in LN_FAMILIES
    tol_u, tol_s, tol_g = TOL, (5e-5 if ln else 2 * TOL), TOL
    worst = {"u": 0.0, "stream": 0.0, "stream4": 0.0, "grad": 0.0, "xg": 0.0, "tg": 0.0}
    for din, line, sets in LINES:
        sd, build64, build_gpu, first = _network(family, act, width, din)
        prog = build_gpu(sd, dev)
        trainable = [k for k in sd if not k.endswith("fourier.B")]
        kw = _line_kwargs(line)
        for NT, NX in sets:
            K = 1 + NX
            xp, tp, cp = _population(din, NT, NX, seed=20000 * din + 100 * NX + sum((3 ** c) * (v % 3) for c, v in enumerate(line)))
            pop = _reference(build64, sd, first, din, line, xp, tp, cp, NX)
            rms = {"jets": [float(pop[0][s].norm()) / 10.0 for s in range(K)], "xg": float(pop[2].norm()) / 10.0,
                   "tg": float(pop[3].norm()) / 10.0}

            def scaled(got, want, scale, N):
                return float((got.double() - want).norm()) / (N ** 0.5 * scale)

            for N in POINTS:
                x, t, cot = xp[:N], tp[:N], cp[:, :N].contiguous()
                jets64, grads64, xg64, tg64 = pop if N == 100 else _reference(build64, sd, first, din, line, x, t, cot, NX)
                xd, td, cd = x.to(dev), t.to(dev), cot.to(dev)
                desc = E._axis_desc(prog, kw.get("axis", 0), kw.get("direction"))
                assert _lib.kernel_name(_AxisView(desc), N, NT, NX, 1) == "layer_major"
                jets = E.jets_forward(prog, xd, td, NT, NX, **kw).cpu()
                assert jets.shape == (K, N)
                where = f"{family}/{act}/{width} din={din} line={line} set=({NT},{NX}) N={N}"
                for s in range(K):
                    e = scaled(jets[s], jets64[s], rms["jets"][s], N)
                    key = "u" if s == 0 else ("stream4" if s == 4 else "stream")
                    worst[key] = max(worst[key], e)
                    assert e <= (tol_u if s == 0 else tol_s), f"{where}: jet stream {s}: {e:.2e}"
                for k in trainable:  # parameters no jet depends on (attention's query and key at sequence length 1): zero
                    grads64.setdefault(k, torch.zeros_like(sd[k], dtype=torch.float64))
                want = torch.cat([grads64[k].flatten() for k in trainable])
                flat = E.new_flat_grad(prog, dev)
                E.jets_backward(prog, xd, td, NT, NX, cd, flat, **kw)
                by = {k: g for k, g in zip(sd, E.split_flat_grad(prog, flat)) if g is not None}
                got = torch.cat([by[k].flatten().cpu() for k in trainable])
                e = rel_l2(got, want, label="direction weight gradient", tol=tol_g)
                worst["grad"] = max(worst["grad"], e)
                assert e <= tol_g, f"{where}: weight gradient: {e:.2e}"
                if not first.endswith("fourier.B"):  # the first Linear on its own: every column, the sheared ones included
                    e1 = rel_l2(by[first].cpu(), grads64[first], label="direction first-Linear gradient", tol=tol_s)
                    assert e1 <= tol_s, f"{where}: first-Linear gradient: {e1:.2e}"
                flat2 = E.new_flat_grad(prog, dev)
                xg, tg = E.jets_backward_inputs(prog, xd, td, NT, NX, cd, flat2, True, True, **kw)
                e_x, e_t = scaled(xg.cpu(), xg64, rms["xg"], N), scaled(tg.cpu(), tg64, rms["tg"], N)
                worst["xg"], worst["tg"] = max(worst["xg"], e_x), max(worst["tg"], e_t)
                assert e_x <= tol_s and e_t <= tol_s, f"{where}: x_grad {e_x:.2e}, t_grad {e_t:.2e}"
                by2 = {k: g for k, g in zip(sd, E.split_flat_grad(prog, flat2)) if g is not None}
                e = rel_l2(torch.cat([by2[k].flatten().cpu() for k in trainable]), want)
                assert e <= tol_g, f"{where}: weight gradient of the input-cotangent call: {e:.2e}"
    print(f"{family}/{act}/{width}: worst " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


@pytest.mark.parametrize("family,act", [("feedforward_ln", "tanh"), ("fourier", "gelu"), ("resnet", "tanh"), ("autoencoder", "gelu")])
def test_deterministic_mode_is_bit_identical_along_a_direction(family, act, dev):
    from pinnrl_amd import engine as E

    din, line, N, NT, NX = 4, (1, -1, 1), 100, 0, 4
    sd, build64, build_gpu, first = _network(family, act, 40, din)
    prog = build_gpu(sd, dev)
    prog.set_deterministic(True)
    g = torch.Generator().manual_seed(3)
    x, t = (torch.rand(N, din - 1, generator=g) * 2 - 1).to(dev), torch.rand(N, 1, generator=g).to(dev)
    cot = torch.randn(1 + NT + NX, N, generator=g).to(dev)
    runs = []
    for _ in range(2):
        flat = E.new_flat_grad(prog, dev)
        E.jets_backward(prog, x, t, NT, NX, cot, flat, direction=line)
        xg, tg = E.jets_backward_inputs(prog, x, t, NT, NX, cot, None, True, True, direction=line)
        runs.append((E.jets_forward(prog, x, t, NT, NX, direction=line), flat, xg, tg))
    for u, v in zip(*runs):
        assert torch.equal(u, v)
    assert float(runs[0][1].abs().max()) > 0.0


def test_the_engine_shears_in_the_stated_rounding_order(dev):
    """The fp32 shear of tests/direction_model.py is the engine's, bit for bit: an axis launch of the fp32-sheared network on
    the fp32-sheared points gives the streams of the direction launch of the network as given, and a refused line is refused."""
    from pinnrl_amd import engine as E

    for din, line in ((3, (1, -1)), (4, (0, 1, -1)), (4, (1, -1, 1))):
        sd, build64, build_gpu, first = _network("feedforward", "tanh", 40, din)
        prog = build_gpu(sd, dev)
        prog.set_layer_major(True)
        g = torch.Generator().manual_seed(5)
        x, t = torch.rand(33, din - 1, generator=g) * 2 - 1, torch.rand(33, 1, generator=g)
        got = E.jets_forward(prog, x.to(dev), t.to(dev), 0, 4, direction=line)
        # the same unit of the same set needs a line too: the sheared network with columns 0 and 1 exchanged once more,
        # launched along axis 1, hands the kernels the very same packed map and coordinates
        swap = (0, 1)
        sheared = build_gpu(DM.shear_state_dict(DM.shear_state_dict(sd, first, line), first, swap), dev)
        xs = DM.shear_inputs(DM.shear_inputs(torch.cat([x, t], 1), line), swap)
        want = E.jets_forward(sheared, xs[:, : din - 1].contiguous().to(dev), xs[:, din - 1:].contiguous().to(dev), 0, 4, axis=1)
        assert torch.equal(got, want), (din, line)
    with pytest.raises(NotImplementedError, match="not compiled"):
        E.jets_forward(prog, x.to(dev), t.to(dev), 1, 2, direction=(1, -1, 1))
    with pytest.raises(ValueError, match="direction"):
        E.jets_forward(prog, x.to(dev), t.to(dev), 0, 2, direction=(1, 0, 0))
