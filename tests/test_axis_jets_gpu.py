"""Jet launches along a further space axis (PINN_FLAG_SPACE_AXIS) against the fp64 node model.

The truth needs no new model: a derivative along axis a equals the axis-0 derivative of the same network with columns 0 and a
swapped in x and in the first Linear (or in the rows of Fourier B).  So tests/jet_model.py::program_forward /
program_backward run on the swapped network, the first Linear's gradient columns are swapped back, and the input
cotangents come from autograd through the same fp64 jets, columns swapped back.

Families: feedforward with and without LayerNorm, fourier, siren, resnet, attention, autoencoder with and without LayerNorm;
depth 2, widths 32 and 40 (a padded width); input_dim 3 with axis 1, input_dim 4 with axes 1 and 2; sets (0, 1), (0, 2), (1, 2);
N in {1, 15, 16, 17, 33, 100}, the edges of the 16-point unit and the 32-point tile.  Activations: tanh and gelu, and sin as
SIREN's sin(omega_0 z) — smooth ones only, so no point is left out.  Bars as tests/test_hip_parity.py and
tests/test_autoencoder_gpu.py hold them: 1e-5 relative l2 for u and the weight gradient, 2e-5 for a derivative stream and the
input cotangents, 5e-5 for those of LayerNorm networks.  Every batch size takes the first N of one 100-point population; the
per-point quantities (streams, input cotangents) are measured as |got - want|_2 / (sqrt(N) rms over the population), which is
the relative l2 error at N = 100 and the same bar per point below it (one point's value can cancel to nearly nothing: at
N = 1 a plain relative error of such a value reached 4e-4 on streams whose population error is 3e-6)."""

import pytest
import torch

import autoencoder_model as AM
import jet_model as JM
from conftest import rel_l2

pytestmark = pytest.mark.gpu

TOL = 1e-5
POINTS = (1, 15, 16, 17, 33, 100)
AXES = ((3, 1), (4, 1), (4, 2))  # (input_dim, axis)
SETS = ((0, 1), (0, 2), (1, 2))
FAMILIES = [("feedforward", "tanh"), ("feedforward", "gelu"), ("feedforward_ln", "tanh"), ("feedforward_ln", "gelu"),
            ("fourier", "tanh"), ("fourier", "gelu"), ("siren", "sin"), ("resnet", "tanh"), ("resnet", "gelu"),
            ("attention", "tanh"), ("attention", "gelu"), ("autoencoder", "tanh"), ("autoencoder", "gelu"),
            ("autoencoder_ln", "tanh"), ("autoencoder_ln", "gelu")]
LN_FAMILIES = ("feedforward_ln", "resnet", "attention", "autoencoder_ln")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _network(family, act, width, din, seed=7):
    """(state_dict fp32 in ABI order, node-model builder(sd64) -> program, NetProgram builder(sd, dev), first-layer key)."""
    import oracle as O
    from hip_helpers import program_from_spec
    from pinnrl_amd import engine as E

    if family.startswith("autoencoder"):
        from pinnrl_amd.neural_networks import AutoEncoder

        ln, hidden, latent = family.endswith("_ln"), [width, width], width // 2 + 1
        torch.manual_seed(seed)
        net = AutoEncoder({"input_dim": din, "hidden_dims": hidden, "latent_dim": latent, "activation": act, "layer_norm": ln,
                           "dropout": 0.0, "output_dim": 1})
        sd = AM.perturb({"model." + k: v.detach().clone() for k, v in net.state_dict().items()}, seed + 1, 0.2)

        def gpu(sd_, dev):
            tensors = [v.to(dev).contiguous() for v in sd_.values()]
            return E.NetProgram("autoencoder", act, din, hidden + [latent] + hidden[::-1] + [1], tensors, [True] * len(tensors),
                                num_blocks=len(hidden), layer_norm=ln)

        return sd, (lambda s: AM.autoencoder_program(s, len(hidden), act, ln)), gpu, "model.encoder.0.weight"
    arch = "feedforward" if family.startswith("feedforward") else family
    spec = O.ArchSpec(arch, input_dim=din, hidden_dim=width, num_layers=3 if arch == "fourier" else 2, activation=act,
                      mapping_size=12, scale=1.5, omega_0=3.0, num_blocks=2 if arch == "resnet" else None,
                      layer_norm=family == "feedforward_ln")
    sd = AM.perturb(O.init_state_dict(spec, seed=seed), seed + 1, 0.2)  # biases and LayerNorm parameters off their initial 0 / 1
    first = {"feedforward": "model.layers.0.weight", "fourier": "model.fourier.B", "siren": "model.layers.0.linear.weight",
             "resnet": "model.input_layer.weight", "attention": "model.input_proj.weight"}[arch]
    return sd, (lambda s: JM.net_program(spec, s)), (lambda sd_, dev: program_from_spec(spec, sd_, dev)[0]), first


class _AxisView:
    """What `_lib.kernel_name` reads of a program, with the descriptor of a launch along an axis."""

    def __init__(self, desc):
        self.desc = desc


def _swap_first(sd, first, a):
    """The network that sees column a where the original sees column 0, and the other way round."""
    out = dict(sd)
    W = sd[first].clone()
    if first.endswith("fourier.B"):
        W[[0, a], :] = sd[first][[a, 0], :]
    else:
        W[:, [0, a]] = sd[first][:, [a, 0]]
    out[first] = W
    return out


def _population(din, NT, NX, seed, n=100):
    """The 100 seeded points and cotangents of one (input_dim, axis, set): every batch size takes its first N of them."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, din - 1, generator=g) * 2 - 1
    t = torch.rand(n, 1, generator=g)
    return x, t, torch.randn(1 + NT + NX, n, generator=g)


def _reference(build64, sd, first, din, a, x, t, cot, NT, NX):
    """fp64 truth on the given points: jets along axis a, d<cot, jets>/d(theta), d<cot, jets>/d(x), d<cot, jets>/d(t)."""
    K = 1 + NT + NX
    sd64 = {k: v.double() for k, v in _swap_first(sd, first, a).items()}
    inp = torch.cat([x, t], 1).double()
    inp_sw = inp.clone()
    inp_sw[:, [0, a]] = inp[:, [a, 0]]
    inp_sw.requires_grad_(True)
    prog = build64(sd64)
    u, _ = JM.program_forward(prog, inp_sw, NT, NX)  # under autograd: the input cotangents
    pairing = sum((cot[s].double() * u[s][:, 0]).sum() for s in range(K))
    ig_sw, = torch.autograd.grad(pairing, inp_sw)
    ig = ig_sw.clone()
    ig[:, [0, a]] = ig_sw[:, [a, 0]]
    with torch.no_grad():  # the node model's own reverse sweep: the weight gradient
        u, tape = JM.program_forward(prog, inp_sw.detach(), NT, NX)
        grads = JM.program_backward(prog, tape, [cot[s].double().unsqueeze(1) for s in range(K)], NT, NX)
    if not first.endswith("fourier.B"):
        gw = grads[first].clone()
        gw[:, [0, a]] = grads[first][:, [a, 0]]
        grads[first] = gw
    return torch.stack([s[:, 0] for s in u]), grads, ig[:, : din - 1], ig[:, din - 1:]


@pytest.mark.parametrize("width", [32, 40])
@pytest.mark.parametrize("family,act", FAMILIES)
def test_jets_gradients_and_input_cotangents_along_an_axis(family, act, width, dev):
    from pinnrl_amd import _lib
    from pinnrl_amd import engine as E

    ln = family in LN_FAMILIES
    tol_u, tol_s, tol_g = TOL, (5e-5 if ln else 2 * TOL), TOL
    worst = {"u": 0.0, "stream": 0.0, "grad": 0.0, "xg": 0.0, "tg": 0.0}
    for din, a in AXES:
        sd, build64, build_gpu, first = _network(family, act, width, din)
        prog = build_gpu(sd, dev)
        trainable = [k for k in sd if not k.endswith("fourier.B")]
        for NT, NX in SETS:
            K = 1 + NT + NX
            xp, tp, cp = _population(din, NT, NX, seed=10000 * din + 1000 * a + 100 * NT + 10 * NX)
            # Per-point outputs (a jet stream, x_grad, t_grad) do not depend on the batch, and a single point's value can cancel
            # to nearly nothing, which no fp32 evaluation resolves relatively.  So their bars are taken as they are meant — a
            # relative l2 error over a population: |got - want|_2 / (sqrt(N) rms), rms the root mean square of that quantity
            # over the 100-point population.  At N = 100 this IS the relative l2 error; below, the same bar per point.
            pop = _reference(build64, sd, first, din, a, xp, tp, cp, NT, NX)
            rms = {"jets": [float(pop[0][s].norm()) / 10.0 for s in range(K)], "xg": float(pop[2].norm()) / 10.0,
                   "tg": float(pop[3].norm()) / 10.0}

            def scaled(got, want, scale, N):
                return float((got.double() - want).norm()) / (N ** 0.5 * scale)

            for N in POINTS:
                x, t, cot = xp[:N], tp[:N], cp[:, :N].contiguous()
                jets64, grads64, xg64, tg64 = pop if N == 100 else _reference(build64, sd, first, din, a, x, t, cot, NT, NX)
                xd, td, cd = x.to(dev), t.to(dev), cot.to(dev)
                assert _lib.kernel_name(_AxisView(E._axis_desc(prog, a)), N, NT, NX, 1) == "layer_major"
                jets = E.jets_forward(prog, xd, td, NT, NX, axis=a).cpu()
                assert jets.shape == (K, N)
                where = f"{family}/{act}/{width} din={din} axis={a} set=({NT},{NX}) N={N}"
                for s in range(K):
                    e = scaled(jets[s], jets64[s], rms["jets"][s], N)
                    worst["u" if s == 0 else "stream"] = max(worst["u" if s == 0 else "stream"], e)
                    assert e <= (tol_u if s == 0 else tol_s), f"{where}: jet stream {s}: {e:.2e}"
                for k in trainable:  # parameters no jet depends on (attention's query and key at sequence length 1): zero
                    grads64.setdefault(k, torch.zeros_like(sd[k], dtype=torch.float64))
                want = torch.cat([grads64[k].flatten() for k in trainable])
                flat = E.new_flat_grad(prog, dev)
                E.jets_backward(prog, xd, td, NT, NX, cd, flat, axis=a)
                by = {k: g for k, g in zip(sd, E.split_flat_grad(prog, flat)) if g is not None}
                got = torch.cat([by[k].flatten().cpu() for k in trainable])
                e = rel_l2(got, want, label="axis weight gradient", tol=tol_g)
                worst["grad"] = max(worst["grad"], e)
                assert e <= tol_g, f"{where}: weight gradient: {e:.2e}"
                if not first.endswith("fourier.B"):  # the first Linear on its own: every column, the seeded ones included
                    e1 = rel_l2(by[first].cpu(), grads64[first], label="axis first-Linear gradient", tol=tol_s)
                    assert e1 <= tol_s, f"{where}: first-Linear gradient: {e1:.2e}"
                flat2 = E.new_flat_grad(prog, dev)
                xg, tg = E.jets_backward_inputs(prog, xd, td, NT, NX, cd, flat2, True, True, axis=a)
                e_x, e_t = scaled(xg.cpu(), xg64, rms["xg"], N), scaled(tg.cpu(), tg64, rms["tg"], N)
                worst["xg"], worst["tg"] = max(worst["xg"], e_x), max(worst["tg"], e_t)
                assert e_x <= tol_s and e_t <= tol_s, f"{where}: x_grad {e_x:.2e}, t_grad {e_t:.2e}"
                by2 = {k: g for k, g in zip(sd, E.split_flat_grad(prog, flat2)) if g is not None}
                e = rel_l2(torch.cat([by2[k].flatten().cpu() for k in trainable]), want)
                assert e <= tol_g, f"{where}: weight gradient of the input-cotangent call: {e:.2e}"
    print(f"{family}/{act}/{width}: worst " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


@pytest.mark.parametrize("family,act", [("feedforward_ln", "tanh"), ("fourier", "gelu"), ("resnet", "tanh"), ("autoencoder", "gelu")])
def test_deterministic_mode_is_bit_identical_along_an_axis(family, act, dev):
    from pinnrl_amd import engine as E

    din, a, N, NT, NX = 4, 2, 100, 1, 2
    sd, build64, build_gpu, first = _network(family, act, 40, din)
    prog = build_gpu(sd, dev)
    prog.set_deterministic(True)
    g = torch.Generator().manual_seed(3)
    x, t = (torch.rand(N, din - 1, generator=g) * 2 - 1).to(dev), torch.rand(N, 1, generator=g).to(dev)
    cot = torch.randn(1 + NT + NX, N, generator=g).to(dev)
    runs = []
    for _ in range(2):
        flat = E.new_flat_grad(prog, dev)
        E.jets_backward(prog, x, t, NT, NX, cot, flat, axis=a)
        xg, tg = E.jets_backward_inputs(prog, x, t, NT, NX, cot, None, True, True, axis=a)
        runs.append((E.jets_forward(prog, x, t, NT, NX, axis=a), flat, xg, tg))
    for u, v in zip(*runs):
        assert torch.equal(u, v)
    assert float(runs[0][1].abs().max()) > 0.0


def test_axis_zero_is_the_call_without_the_argument(dev):
    """axis=0 passes the program's own descriptor: the same launches, the same bits as before the argument existed; and the
    streams of axis 1 differ from those of axis 0 (the flag reaches the kernels)."""
    from pinnrl_amd import engine as E

    sd, build64, build_gpu, first = _network("feedforward", "tanh", 40, 3)
    prog = build_gpu(sd, dev)
    prog.set_layer_major(True)
    g = torch.Generator().manual_seed(5)
    x, t = (torch.rand(33, 2, generator=g) * 2 - 1).to(dev), torch.rand(33, 1, generator=g).to(dev)
    j0, j0b, j1 = E.jets_forward(prog, x, t, 1, 2), E.jets_forward(prog, x, t, 1, 2, axis=0), E.jets_forward(prog, x, t, 1, 2, axis=1)
    assert torch.equal(j0, j0b)
    # u and u_t agree to rounding (the first Linear adds its products in another order), the space streams are other functions
    assert rel_l2(j1[:2].cpu(), j0[:2].cpu()) <= TOL and rel_l2(j1[2:].cpu(), j0[2:].cpu()) > 1e-2
    with pytest.raises(NotImplementedError, match="not compiled"):
        E.jets_forward(prog, x, t, 0, 2)  # the space-only sets need a non-zero axis
    with pytest.raises(ValueError, match="space axis"):
        E.jets_forward(prog, x, t, 0, 2, axis=2)
