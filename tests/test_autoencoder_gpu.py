"""GPU tests of the autoencoder architecture on the layer-major engine: the fixtures of tools/make_autoencoder_golden.py
(held to `grad64_exact`, the gradient with LayerNorm written out), random parameters against the fp64 node model
(tests/autoencoder_model.py) on shapes chosen for the identity node — the first decoder Linear, whose input record IS the
latent Linear's output record — and the Python surface (input gradients, inverse mode, trainer, encode / decode).

Tolerances are those of tests/test_hip_parity.py for the same quantities: 1e-5 relative l2 for u, residual, loss and gradient,
2e-5 on single derivative streams (5e-5 on those of LayerNorm networks), 1e-4 wherever relu's kinks are in play."""
import math
import os
import subprocess
import sys

import pytest
import torch

import autoencoder_model as AM
import jet_model as JM
from conftest import rel_err, rel_l2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_fixtures = {}


def _fixture(tag):
    if tag not in _fixtures:
        _fixtures[tag] = AM.load_fixture(tag)
    return _fixtures[tag]


def _pde(meta, dev, **extra):
    from pinnrl_amd import pdes as P

    p = meta["pde"]
    cls = {"burgers": P.BurgersEquation, "kdv": P.KdVEquation, "allen_cahn": P.AllenCahnEquation}[p["name"]]
    return cls(P.PDEConfig(name=p["name"], domain=[tuple(d) for d in p["domain"]], time_domain=tuple(p["time_domain"]),
                           parameters=dict(p["parameters"]), boundary_conditions={"dirichlet": {"type": "fixed", "value": 0.0}},
                           initial_condition=dict(p["initial_condition"]), exact_solution={}, dimension=1, device=dev, **extra))


def _product(tag, dev):
    from pinnrl_amd.neural_networks import PINNModel

    meta, sd, a = _fixture(tag)
    cfg = AM.model_config(meta, dev)
    model = PINNModel(cfg, device=dev)
    model.load_state_dict({k: v.to(dev) for k, v in sd.items()})
    return cfg, model, _pde(meta, dev), (meta, sd, a)


def _tols(meta):
    """(value stream u, derivative streams, residual / loss / gradient)"""
    m = meta["model"]
    if m["activation"] == "relu":
        return 1e-4, 1e-4, 1e-4
    return TOL, (5e-5 if m["layer_norm"] else 2 * TOL), TOL


# ---------------------------------------------------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", AM.CASES)
def test_fixture_parity(tag, dev):
    """model.jets per stream, compute_residual, the loss and the flat gradient (through loss.backward()) against the fixture."""
    cfg, model, pde, (meta, sd, a) = _product(tag, dev)
    NT, NX = meta["streams"]
    tol_u, tol_jet, tol = _tols(meta)
    x, t = torch.from_numpy(a["x"]).to(dev), torch.from_numpy(a["t"]).to(dev)
    from pinnrl_amd import _lib

    assert _lib.kernel_name(model.program(), x.shape[0], NT, NX, 1) == "layer_major"
    with torch.no_grad():
        jets = model.jets(x, t, NT, NX).cpu()
    assert jets.shape == a["jets64"].shape
    for s in range(jets.shape[0]):
        e = rel_l2(jets[s], a["jets64"][s], label=f"jet stream {s}", tol=tol_u if s == 0 else tol_jet)
        print(f"{tag}: jet stream {s}: {e:.2e}")
        assert e <= (tol_u if s == 0 else tol_jet), f"jet stream {s}: {e:.2e}"
    r = pde.compute_residual(model, x, t)
    assert r.shape == (x.shape[0], 1) and r.requires_grad
    e_r = rel_l2(r.detach().cpu(), a["residual64_exact"], label="residual", tol=tol)
    loss = pde._apply_loss_fn(r)
    e_L = rel_err(float(loss.detach()), float(a["loss64_exact"]), label="loss", tol=tol)
    loss.backward()
    got = torch.cat([p.grad.flatten().cpu() for _, p in model.named_parameters()])
    e_g = rel_l2(got, a["grad64_exact"], label="gradient", tol=tol)
    print(f"{tag}: residual {e_r:.2e}, loss {e_L:.2e}, gradient vs grad64_exact {e_g:.2e}, vs the reference's grad64 "
          f"{rel_l2(got, a['grad64']):.2e} (reference vs exact {meta['grad64_vs_exact']['total']:.2e})")
    assert e_r <= tol and e_L <= tol, (e_r, e_L)
    assert e_g <= tol, f"gradient vs grad64_exact: {e_g:.2e}"
    # witness (as tests/test_hip_parity.py): the distance to the reference's own gradient is torch's fused-LayerNorm error, not ours
    assert rel_l2(got, a["grad64"]) <= 2 * meta["grad64_vs_exact"]["total"] + tol
    u = model(torch.cat([x, t], 1))
    assert u.shape == (x.shape[0], 1) and rel_l2(u.detach().cpu(), a["jets64"][0]) <= tol_u


# ---------------------------------------------------------------------------------------------------------------------
# random parameters against the fp64 node model
# ---------------------------------------------------------------------------------------------------------------------
# name: (hidden_dims, latent_dim, activation, layer_norm)
SHAPES = {
    "latent1": ([33], 1, "tanh", False),          # a one-row GEMM weight, fed and followed by 33-wide layers
    "latent40": ([160], 40, "gelu", True),
    "latent257": ([64], 257, "tanh", True),       # the "bottleneck" wider than its neighbours: 64 -> 257 -> 64
    "n3_fused": ([128, 128, 128], 128, "tanh", True),  # every node a fused-kernel shape: fused launches on both sides of the identity node
}
ORDERS = [(0, 0), (1, 2), (2, 2), (1, 4)]
POINTS = [197, 4099]
_refs = {}


def _random_sd(shape, seed):
    hidden, latent, act, ln = SHAPES[shape]
    from pinnrl_amd.neural_networks import AutoEncoder

    torch.manual_seed(seed)
    net = AutoEncoder({"input_dim": 2, "hidden_dims": hidden, "latent_dim": latent, "activation": act, "layer_norm": ln,
                       "dropout": 0.0, "output_dim": 1})
    sd = {"model." + k: v.detach().clone() for k, v in net.state_dict().items()}
    return AM.perturb(sd, seed + 1, 0.2)


def _program(shape, sd, dev):
    from pinnrl_amd import engine as E

    hidden, latent, act, ln = SHAPES[shape]
    tensors = [v.to(dev).contiguous() for v in sd.values()]
    return E.NetProgram("autoencoder", act, 2, hidden + [latent] + hidden[::-1] + [1], tensors, [True] * len(tensors),
                        num_blocks=len(hidden), layer_norm=ln)


def _reference(shape, N, NT, NX):
    """fp64 node model, computed once per case and shared: points, cotangents, jets and d<cot, jets>/d(theta)."""
    key = (shape, N, NT, NX)
    if key not in _refs:
        hidden, latent, act, ln = SHAPES[shape]
        sd = _random_sd(shape, 11)
        g = torch.Generator().manual_seed(1000 * N + 10 * NT + NX)
        x = torch.rand(N, 1, generator=g) * 2 - 1
        t = torch.rand(N, 1, generator=g)
        K = 1 + NT + NX
        cot = torch.randn(K, N, generator=g)
        prog = AM.autoencoder_program({k: v.double() for k, v in sd.items()}, len(hidden), act, ln)
        u, tape = JM.program_forward(prog, torch.cat([x, t], 1).double(), NT, NX)
        grads = JM.program_backward(prog, tape, [cot[s].double().unsqueeze(1) for s in range(K)], NT, NX)
        _refs[key] = (sd, x, t, cot, torch.stack([s[:, 0] for s in u]), grads)
    return _refs[key]


@pytest.mark.parametrize("NT,NX", ORDERS)
@pytest.mark.parametrize("N", POINTS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_random_parameters_against_the_node_model(shape, N, NT, NX, dev):
    from pinnrl_amd import engine as E

    sd, x, t, cot, jets64, grads64 = _reference(shape, N, NT, NX)
    ln = SHAPES[shape][3]
    prog = _program(shape, sd, dev)
    jets = E.jets_forward(prog, x.to(dev), t.to(dev), NT, NX).cpu()
    for s in range(jets.shape[0]):
        tol = TOL if s == 0 else (5e-5 if ln else 2 * TOL)
        e = rel_l2(jets[s], jets64[s], label=f"jet stream {s}", tol=tol)
        assert e <= tol, f"jet stream {s}: {e:.2e}"
    flat = E.new_flat_grad(prog, dev)
    E.jets_backward(prog, x.to(dev), t.to(dev), NT, NX, cot.to(dev), flat)
    got = torch.cat([g.flatten().cpu() for g in E.split_flat_grad(prog, flat)])
    want = torch.cat([grads64[k].flatten() for k in sd])
    e = rel_l2(got, want, label="gradient", tol=TOL)
    assert e <= TOL, f"weight gradient: {e:.2e}"
    # Per tensor, so that a small tensor cannot hide in the flat norm (the latent bias has `latent` elements).  A cotangent that is
    # lost, doubled or routed to the wrong record is an error of order 1 in that tensor; fp32 sums of N K cancelling terms stay
    # far below 1e-3 of a tensor that carries more than 1e-4 of the whole gradient.
    for (k, v), g in zip(sd.items(), E.split_flat_grad(prog, flat)):
        if float(grads64[k].norm()) > 1e-4 * float(want.norm()):
            assert rel_l2(g.cpu(), grads64[k]) <= 1e-3, (k, rel_l2(g.cpu(), grads64[k]))


@pytest.mark.parametrize("shape", ["latent1", "n3_fused"])
def test_input_cotangents_against_autograd_through_the_node_model(shape, dev):
    """pinn_jet_backward_inputs (want_xg): d<cot, jets>/d(x, t), with and without the weight-gradient table."""
    from pinnrl_amd import engine as E

    NT, NX, N = 1, 2, 197
    sd, x, t, cot, jets64, grads64 = _reference(shape, N, NT, NX)
    hidden, latent, act, ln = SHAPES[shape]
    prog64 = AM.autoencoder_program({k: v.double() for k, v in sd.items()}, len(hidden), act, ln)
    # the node model takes its jets from the input map's streams; differentiate u and u_x by autograd instead
    x64, t64 = x.double().requires_grad_(True), t.double().requires_grad_(True)
    u = JM.program_forward(prog64, torch.cat([x64, t64], 1), 0, 0)[0][0]
    ut = torch.autograd.grad(u.sum(), t64, create_graph=True)[0]
    ux = torch.autograd.grad(u.sum(), x64, create_graph=True)[0]
    uxx = torch.autograd.grad(ux.sum(), x64, create_graph=True)[0]
    c = cot.double()
    pairing = (c[0] * u[:, 0] + c[1] * ut[:, 0] + c[2] * ux[:, 0] + c[3] * uxx[:, 0]).sum()
    xg64, tg64 = torch.autograd.grad(pairing, [x64, t64])
    prog = _program(shape, sd, dev)
    for with_weights in (False, True):
        flat = E.new_flat_grad(prog, dev) if with_weights else None
        xg, tg = E.jets_backward_inputs(prog, x.to(dev), t.to(dev), NT, NX, cot.to(dev), flat, True, True)
        tol = 5e-5 if ln else 2 * TOL
        assert rel_l2(xg.cpu(), xg64) <= tol and rel_l2(tg.cpu(), tg64) <= tol, (rel_l2(xg.cpu(), xg64), rel_l2(tg.cpu(), tg64))
        if with_weights:
            got = torch.cat([g.flatten().cpu() for g in E.split_flat_grad(prog, flat)])
            assert rel_l2(got, torch.cat([grads64[k].flatten() for k in sd])) <= TOL


@pytest.mark.parametrize("shape", ["latent1", "latent257", "n3_fused"])
def test_deterministic_gradients_are_bit_identical(shape, dev):
    from pinnrl_amd import engine as E

    N = 4099
    sd, x, t, cot, jets64, grads64 = _reference(shape, N, 1, 2)
    prog = _program(shape, sd, dev)
    pd = E.pde_desc("burgers", 1, [0.05])
    x, t = x.to(dev), t.to(dev)
    ref = E.new_flat_grad(prog, dev)
    _, s_ref = E.residual_loss_grad(prog, pd, x, t, 1.0 / N, ref)
    prog.set_deterministic(True)
    runs = []
    for _ in range(2):
        flat = E.new_flat_grad(prog, dev)
        _, s = E.residual_loss_grad(prog, pd, x, t, 1.0 / N, flat)
        runs.append((flat.clone(), s.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert rel_l2(runs[0][0].cpu(), ref.cpu()) <= TOL and abs(float(runs[0][1]) - float(s_ref)) <= TOL * abs(float(s_ref))


def test_model_level_deterministic_switch(dev):
    cfg, model, pde, (meta, sd, a) = _product(AM.CASES[0], dev)
    model.set_deterministic(True)
    x, t = torch.from_numpy(a["x"]).to(dev), torch.from_numpy(a["t"]).to(dev)
    grads = []
    for _ in range(2):
        model.zero_grad()
        pde._apply_loss_fn(pde.compute_residual(model, x, t)).backward()
        grads.append(torch.cat([p.grad.flatten() for p in model.parameters()]).clone())
    assert torch.equal(grads[0], grads[1])
    assert rel_l2(grads[0].cpu(), a["grad64_exact"]) <= TOL


# ---------------------------------------------------------------------------------------------------------------------
# both fusion policies
# ---------------------------------------------------------------------------------------------------------------------
def test_the_unfused_policy_in_a_child_process():
    """plan_fusion keeps the latent node's forward GEMM and the first decoder node's reverse GEMM unfused under every
    policy and fuses the nodes around them by default; PINN_LM_FUSED is read once per process, so the fixtures and the shape
    whose every node is a fused-kernel shape run again with everything unfused in a child."""
    e = dict(os.environ, PINN_LM_FUSED="0")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_autoencoder_gpu.py", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "test_fixture_parity or (test_random_parameters and n3_fused and 197) or test_input_cotangents"],
                       cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and " passed" in r.stdout and "deselected" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]


# ---------------------------------------------------------------------------------------------------------------------
# Python surface
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", AM.CASES)
def test_input_gradients_through_autograd(tag, dev):
    cfg, model, pde, (meta, sd, a) = _product(tag, dev)
    NT, NX = meta["streams"]
    tol_u, tol_jet, tol = _tols(meta)
    x = torch.from_numpy(a["x"]).to(dev).requires_grad_(True)
    t = torch.from_numpy(a["t"]).to(dev).requires_grad_(True)
    u = model(torch.cat([x, t], 1))
    ux, ut = torch.autograd.grad(u.sum(), [x, t], create_graph=True)
    assert rel_l2(ut.detach().cpu()[:, 0], a["jets64"][1]) <= tol_jet
    assert rel_l2(ux.detach().cpu()[:, 0], a["jets64"][NT + 1]) <= tol_jet
    uxx = torch.autograd.grad(ux.sum(), x)[0]
    assert rel_l2(uxx.cpu()[:, 0], a["jets64"][NT + 2]) <= tol_jet


def test_encode_and_decode(dev):
    cfg, model, pde, (meta, sd, a) = _product(AM.CASES[0], dev)
    inp = torch.cat([torch.from_numpy(a["x"]), torch.from_numpy(a["t"])], 1).to(dev)
    with torch.no_grad():
        z = model.model.encode(inp)
        assert z.shape == (inp.shape[0], meta["model"]["latent_dim"]) and z.device.type == "cuda"
        out = model.model.decode(z)
        u = model(inp)
    assert out.shape == u.shape == (inp.shape[0], 1)
    assert rel_l2(out.cpu(), u.cpu()) <= TOL  # plain torch modules against the engine
    assert rel_l2(out.cpu(), a["jets64"][0]) <= TOL


def _inverse_reference(meta, sd, x, t, nu0):
    """Burgers with a trainable nu: loss, d/dnu and d/dtheta by autograd through the fp64 node model."""
    m = meta["model"]
    params = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    nu = torch.tensor(nu0, dtype=torch.float64, requires_grad=True)
    prog = AM.autoencoder_program(params, len(m["hidden_dims"]), m["activation"], m["layer_norm"])
    inp = torch.cat([x, t], 1).double()
    u, _ = JM.program_forward(prog, inp, 1, 2)
    r, _ = JM.pde_residual("burgers", {"nu": nu}, u, inp[:, :1], 1, 2)
    L = (r * r).mean()
    g = torch.autograd.grad(L, [nu] + list(params.values()))
    return float(L.detach()), float(g[0]), torch.cat([v.flatten() for v in g[1:]])


def test_inverse_mode_gradients(dev):
    """pinn_residual_loss_grad_inverse (coefficients read from the device) and pinn_residual_loss_grad_coef (by value): the
    head kernel's coefficient reduction on this architecture, against autograd through the fp64 node model."""
    from pinnrl_amd import engine as E

    cfg, model, pde, (meta, sd, a) = _product(AM.CASES[0], dev)
    x, t = torch.from_numpy(a["x"]), torch.from_numpy(a["t"])
    N, nu0 = x.shape[0], 0.07
    nu32 = float(torch.tensor(nu0, dtype=torch.float32))
    L64, dnu64, g64 = _inverse_reference(meta, sd, x, t, nu32)
    prog = model.program()
    pd = E.pde_desc("burgers", 1, [nu32])
    assert E.inverse_kernel_name(prog, pd, N) == "layer_major"
    for entry in ("inverse", "coef"):
        flat, cg = E.new_flat_grad(prog, dev), torch.zeros(2, device=dev)
        if entry == "inverse":
            cv = torch.tensor([nu32, 0.0, 0.0, 0.0], device=dev)
            _, s = E.residual_loss_grad_inverse(prog, E.pde_desc("burgers", 1, [123.0]), cv, x.to(dev), t.to(dev), 1.0 / N, flat, cg)
        else:
            _, s = E.residual_loss_grad(prog, pd, x.to(dev), t.to(dev), 1.0 / N, flat, coef_grads=cg)
        got = torch.cat([g.flatten().cpu() for g in E.split_flat_grad(prog, flat)])
        e = (rel_err(float(s) / N, L64), rel_err(float(cg[0]), dnu64), rel_l2(got, g64))
        print(f"{entry}: loss {e[0]:.2e}, d/dnu {e[1]:.2e}, d/dtheta {e[2]:.2e}")
        assert max(e) <= TOL, (entry, e)
    # and through the Python surface: a trainable nu stays in the graph
    pde_inv = _pde(meta, dev, trainable_parameters=["nu"], parameter_initial_guesses={"nu": nu32})
    model.zero_grad()
    r = pde_inv.compute_residual(model, x.to(dev), t.to(dev))
    (r**2).mean().backward()
    assert rel_err(float(pde_inv.get_parameter("nu").grad), dnu64) <= 1e-4  # the bar of test_inverse_mode_trainable_coefficient
    got = torch.cat([p.grad.flatten().cpu() for _, p in model.named_parameters()])
    assert rel_l2(got, g64) <= TOL


# ---------------------------------------------------------------------------------------------------------------------
# trainer
# ---------------------------------------------------------------------------------------------------------------------
def _trainer(dev, fast_step=None, optimizer="adam", lr=1e-3):
    from pinnrl_amd.config import TrainingConfig
    from pinnrl_amd.training import PDETrainer

    cfg, model, pde, _ = _product(AM.CASES[0], dev)
    cfg.training = TrainingConfig(learning_rate=lr, gradient_clipping=1.0 if optimizer == "adam" else 0.0, optimizer=optimizer)
    if optimizer != "adam":
        cfg.training.lbfgs.max_iter, cfg.training.lbfgs.history_size = 4, 10
    tr = PDETrainer(model, pde, {}, cfg, device=dev, validation_frequency=100, fast_step=fast_step)
    torch.manual_seed(1)
    xb, tb = pde.generate_collocation_points(1000, strategy="uniform")
    tr._sample = lambda n, xb=xb, tb=tb: (xb, tb)
    return model, tr, xb.shape[0]


def _theta(model):
    return torch.cat([p.detach().flatten().cpu() for p in model.parameters()])


def test_three_adam_steps_launch_list_autograd_and_graph(dev):
    """The launch list, make_graphed_step and the autograd step work on programs, not on architectures: three Adam steps
    from the same theta_0 on the same pinned batch end at the same theta (comparison and bar of
    tests/test_api_gpu.py::test_graph_captured_step_for_the_other_configurations)."""
    thetas = {}
    for path in ("autograd", "launch_list", "graph"):
        model, tr, n = _trainer(dev, fast_step=False if path == "autograd" else None)
        if path != "autograd":
            assert tr._manual_step_unsupported() is None, tr._manual_step_unsupported()
            tr._build_flat_state()
        if path == "graph":
            replay, losses = tr.make_graphed_step(n, warmup=1)
            torch.manual_seed(7)
            for _ in range(2):
                replay()
            torch.cuda.synchronize()
            assert math.isfinite(float(losses["total"])) and set(losses) >= {"residual", "boundary", "initial", "total"}
        else:
            x0, t0 = tr._sample(n)
            out = tr.train_step(x0, t0)
            torch.manual_seed(7)
            for _ in range(2):
                x0, t0 = tr._sample(n)
                out = tr.train_step(x0, t0)
            assert math.isfinite(float(out["total"]))
            assert (getattr(tr, "_flat", None) is not None) == (path == "launch_list")
        thetas[path] = _theta(model)
    e_a, e_g = rel_l2(thetas["launch_list"], thetas["autograd"]), rel_l2(thetas["graph"], thetas["launch_list"])
    print(f"theta after three steps: launch list vs autograd {e_a:.2e}, graph vs launch list {e_g:.2e}")
    assert e_a <= 1e-5 and e_g <= 1e-5


def test_one_lbfgs_step_on_the_flat_path(dev):
    model, tr, n = _trainer(dev, fast_step=True, optimizer="lbfgs", lr=0.5)
    assert tr._is_lbfgs and tr._manual_step_unsupported() is None, tr._manual_step_unsupported()
    tr._build_flat_state()
    before = _theta(model)
    x0, t0 = tr._sample(n)
    first = tr.train_step(x0, t0)
    drv = tr._flat["lbfgs"]["driver"]
    assert drv.func_evals > 0 and drv.n_iter > 0
    assert all(math.isfinite(float(v)) for v in first.values()) and not torch.equal(_theta(model), before)
    model_e, tr_e, _ = _trainer(dev, fast_step=False, optimizer="lbfgs", lr=0.5)
    tr_e.train_step(x0, t0)
    e = rel_l2(_theta(model), _theta(model_e))
    print(f"theta after one L-BFGS step, flat path vs eager: {e:.2e}")
    assert e <= 1e-4  # the bar of tests/test_lbfgs_gpu.py::test_lbfgs_train_step_on_the_launch_list
