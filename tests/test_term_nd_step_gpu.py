"""`TermPDEnD` end to end on the GPU: three problems on 2 x 32 networks —

  heat2d     u_t - alpha (u_xx + u_yy), exact exp(-2 alpha pi^2 t) sin(pi x) sin(pi y), Dirichlet faces, fourier
  burgers2d  u_t + u u_x + u u_y - nu (u_xx + u_yy), Dirichlet faces, feedforward (axis 0 on the fused tile-major kernel,
             axis 1 on the layer-major engine)
  heat3d     u_t - alpha (u_xx + u_yy + u_zz), periodic faces, fourier

against torch fp64 autograd through `oracle.network_forward` with the written-out formula (residual, loss terms, d total /
d theta on 200 points: 1e-5, the bar of tests/test_term_pde_gpu.py), and the launch list against the autograd step with the bars
of tests/test_term_step_gpu.py (theta after 1 / 3 / 10 Adam steps 1e-5, one L-BFGS step 1e-4); a captured step replays the
eager launch list bit for bit; the residual-based sampler runs; and 200 Adam steps lower the loss and the error."""

import math

import pytest
import torch

from conftest import rel_err, rel_l2

pytestmark = pytest.mark.gpu

TOL = 1e-5
NPTS = 100
PI = math.pi


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _sines(x):
    return torch.prod(torch.sin(PI * x), dim=1)


def _sines2(x):
    return torch.prod(torch.sin(2 * PI * x), dim=1)


PROBLEMS = {
    "heat2d": dict(dim=2, arch="fourier", params={"alpha": 0.05}, bcs={"dirichlet": {"type": "fixed", "value": 0.0}}, ic=_sines,
                   terms=[(1.0, ("u_t",)), ((-1.0, "alpha"), ("u_xx",)), ((-1.0, "alpha"), ("u_yy",))],
                   exact=lambda x, t: torch.exp(-2 * 0.05 * PI**2 * t[:, 0]) * _sines(x)),
    "burgers2d": dict(dim=2, arch="feedforward", params={"nu": 0.05}, bcs={"dirichlet": {"type": "fixed", "value": 0.0}}, ic=_sines,
                      terms=[(1.0, ("u_t",)), (1.0, ("u", "u_x")), (1.0, ("u", "u_y")), ((-1.0, "nu"), ("u_xx",)),
                             ((-1.0, "nu"), ("u_yy",))], exact=None),
    "heat3d": dict(dim=3, arch="fourier", params={"alpha": 0.02}, bcs={"periodic": {}}, ic=_sines2,
                   terms=[(1.0, ("u_t",)), ((-1.0, "alpha"), ("u_xx",)), ((-1.0, "alpha"), ("u_yy",)), ((-1.0, "alpha"), ("u_zz",))],
                   exact=lambda x, t: torch.exp(-3 * 0.02 * 4 * PI**2 * t[:, 0]) * _sines2(x)),
}


def _spec(name):
    import oracle as O

    p = PROBLEMS[name]
    if p["arch"] == "fourier":
        return O.ArchSpec("fourier", input_dim=p["dim"] + 1, hidden_dim=32, num_layers=3, activation="tanh", mapping_size=8, scale=1.0)
    return O.ArchSpec("feedforward", input_dim=p["dim"] + 1, hidden_dim=32, num_layers=2, activation="tanh")


def _build(name, dev, optimizer="adam", lr=1e-3, sampler="uniform", seed=3):
    """cfg, model (theta_0 from the oracle's initialiser under `seed`), the TermPDEnD, the oracle's ArchSpec and state_dict."""
    import oracle as O
    from pinnrl_amd import pdes as P
    from pinnrl_amd.config import Config, ModelConfig, TrainingConfig
    from pinnrl_amd.neural_networks import PINNModel

    p, spec = PROBLEMS[name], _spec(name)
    cfg = Config.__new__(Config)
    cfg.device = dev
    cfg.model = ModelConfig(input_dim=spec.input_dim, hidden_dim=spec.hidden_dim, output_dim=1, num_layers=spec.num_layers,
                            activation=spec.activation, architecture=spec.architecture)
    cfg.model.mapping_size, cfg.model.scale = spec.mapping_size, spec.scale
    cfg.training = TrainingConfig(learning_rate=lr, gradient_clipping=1.0, optimizer=optimizer)
    cfg.training.collocation_distribution = sampler
    sd = O.init_state_dict(spec, seed=seed)
    model = PINNModel(cfg, device=dev)
    model.load_state_dict({k: v.to(dev) for k, v in sd.items()})
    pc = P.PDEConfig(name=name, domain=[(0.0, 1.0)] * p["dim"], time_domain=(0.0, 0.5), parameters=dict(p["params"]),
                     boundary_conditions=dict(p["bcs"]), initial_condition={}, exact_solution={}, dimension=p["dim"], device=dev,
                     training=cfg.training)
    pde = P.TermPDEnD(pc, p["terms"], p["ic"], exact_solution_fn=p["exact"], boundary_points_per_axis=4, initial_points_per_axis=5)
    return cfg, model, pde, spec, sd


def _theta(model):
    return torch.cat([p.detach().flatten().cpu() for _, p in model.named_parameters()])


def _points(name, n, seed):
    g = torch.Generator().manual_seed(seed)
    dim = PROBLEMS[name]["dim"]
    return torch.rand(n, dim, generator=g), torch.rand(n, 1, generator=g) * 0.5


_fp64 = {}


def _oracle(name, pde):
    """fp64 residual, loss terms, total and d total / d theta by chained autograd.grad through the oracle's network, on 200
    seeded points and the PDE's own fixed boundary / initial points; computed once per problem."""
    import oracle as O

    if name in _fp64:
        return _fp64[name]
    p, spec = PROBLEMS[name], _spec(name)
    sd = O.init_state_dict(spec, seed=3)
    params = {k: v.double().requires_grad_(k != "model.fourier.B") for k, v in sd.items()}
    x32, t32 = _points(name, 200, 17)
    x, t = x32.double().requires_grad_(True), t32.double().requires_grad_(True)
    u = O.network_forward(spec, params, torch.cat([x, t], 1))
    d = lambda y, w: torch.autograd.grad(y, w, torch.ones_like(y), create_graph=True)[0]  # noqa: E731
    u_t, gx = d(u, t), d(u, x)
    first = [gx[:, a : a + 1] for a in range(p["dim"])]
    second = [d(first[a], x)[:, a : a + 1] for a in range(p["dim"])]
    c = list(p["params"].values())[0]
    r = u_t - c * sum(second)
    if name == "burgers2d":
        r = r + u * first[0] + u * first[1]
    res = torch.mean(r**2)
    pts = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in pde._nd_points().items()}
    ub = O.network_forward(spec, params, torch.cat([pts["x"], pts["t"]], 1).double())[:, 0]
    nbc, nf = pts["n_bc"], pts["n_face"]
    if "dirichlet" in p["bcs"]:
        bnd = torch.mean(ub[:nbc] ** 2)
    else:
        bnd = sum(torch.mean((ub[2 * a * nf : 2 * a * nf + nf] - ub[2 * a * nf + nf : 2 * a * nf + 2 * nf]) ** 2) for a in range(p["dim"]))
    ini = torch.mean((ub[nbc:] - pts["u0"].double()) ** 2)
    lw = pde._loss_weights()  # TrainingConfig's: residual, boundary and initial at 1
    total = lw.get("pde", lw.get("residual", 1.0)) * res + lw.get("boundary", 10.0) * bnd + lw.get("initial", 10.0) * ini
    names = [k for k, v in params.items() if v.requires_grad]
    g = torch.autograd.grad(total, [params[k] for k in names])
    _fp64[name] = {"x": x32, "t": t32, "r": r.detach(), "residual": float(res), "boundary": float(bnd), "initial": float(ini),
                   "total": float(total), "names": names, "grad": torch.cat([v.flatten() for v in g])}
    return _fp64[name]


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_residual_losses_and_gradient_match_fp64_autograd(name, dev):
    from pinnrl_amd import engine as E

    cfg, model, pde, spec, sd = _build(name, dev)
    o = _oracle(name, pde)
    x, t = o["x"].to(dev), o["t"].to(dev)
    r = pde.compute_residual(model, x, t)
    assert r.shape == (200, 1) and r.requires_grad
    e_r = rel_l2(r.detach().cpu(), o["r"], label=f"{name}: residual", tol=TOL)
    losses = pde.compute_loss(model, x, t)
    errs = {k: rel_err(float(losses[k].detach()), o[k], label=f"{name}: {k} loss", tol=TOL) for k in ("residual", "boundary", "initial", "total")}
    model.zero_grad()
    losses["total"].backward()
    got = torch.cat([dict(model.named_parameters())[k].grad.flatten().cpu() for k in o["names"]])
    e_g = rel_l2(got, o["grad"], label=f"{name}: d total / d theta", tol=TOL)
    print(f"{name}: residual {e_r:.2e}, losses {', '.join(f'{k} {v:.2e}' for k, v in errs.items())}, gradient {e_g:.2e}")
    assert e_r <= TOL, f"residual: {e_r:.2e}"
    assert all(v <= TOL for v in errs.values()), errs
    assert e_g <= TOL, f"gradient: {e_g:.2e}"
    # the raw chain: residual_loss_grad accumulates the gradients of every axis into one flat buffer
    prog, td = model.program(), pde._pde_desc()
    flat = E.new_flat_grad(prog, dev)
    r2, s2 = E.residual_loss_grad(prog, td, x, t, 1.0 / 200, flat, want_residual=True)
    assert torch.equal(r2, r.detach()) and rel_err(float(s2) / 200, o["residual"]) <= TOL
    # the RAR sampler's probabilities come from the same dispatch (one l1 forward chain)
    pr = pde._residual_sampling_probabilities(model, x, t)
    want = (o["r"].abs().flatten() + 1e-8) / (o["r"].abs().sum() + 200e-8)
    assert rel_l2(pr.cpu(), want) <= TOL


def _batches(pde, n, seed=5):
    torch.manual_seed(seed)
    return [pde._sample_uniform(NPTS) for _ in range(n)]


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_adam_launch_list_matches_the_autograd_step(name, dev):
    from pinnrl_amd.training import PDETrainer

    runs, batches = {}, None
    for key, fast in (("list", None), ("autograd", False)):
        cfg, model, pde, spec, sd = _build(name, dev)
        batches = batches or _batches(pde, 10)
        tr = PDETrainer(model, pde, {}, cfg, device=dev, fast_step=fast)
        if fast is None:
            assert tr._manual_step_unsupported() is None, tr._manual_step_unsupported()
            tr._build_flat_state()
        thetas, losses = {}, []
        for step, (xb, tb) in enumerate(batches, start=1):
            out = tr.train_step(xb, tb)
            losses.append({k: float(out[k].detach()) for k in ("residual", "boundary", "initial", "total")})
            if step in (1, 3, 10):
                thetas[step] = _theta(model)
        assert (getattr(tr, "_flat", None) is not None) == (fast is None)
        runs[key] = (thetas, losses)
    for step in (1, 3, 10):
        e = rel_l2(runs["list"][0][step], runs["autograd"][0][step], label=f"{name}: theta vs autograd, step {step}", tol=TOL)
        print(f"{name} step {step}: theta vs autograd {e:.2e}")
        assert e <= TOL, (step, e)
    for step, (got, want) in enumerate(zip(runs["list"][1], runs["autograd"][1]), start=1):
        for k in got:
            assert abs(got[k] - want[k]) <= 5e-5 * abs(want[k]), (step, k, got[k], want[k])


@pytest.mark.parametrize("name", ["heat2d", "heat3d"])
def test_captured_step_replays_the_eager_launch_list_bit_for_bit(name, dev):
    from pinnrl_amd.training import PDETrainer

    def trainer():
        cfg, model, pde, spec, sd = _build(name, dev)
        model.program().set_deterministic(True)  # fixed-order weight-gradient sums: the launch list is a function of its inputs
        tr = PDETrainer(model, pde, {}, cfg, device=dev)
        assert tr._manual_step_unsupported() is None
        return tr, model, pde

    tr, model, pde = trainer()
    xb, tb = _batches(pde, 1, seed=0)[0]
    tr._build_flat_state()
    side = torch.cuda.Stream(device=dev)
    for _ in range(4):  # the eager launch list with the fork the captured step has
        tr._manual_launches(xb, tb, side=side)
    torch.cuda.synchronize()
    eager, eager_losses = _theta(model), {k: float(v) for k, v in tr._manual_losses().items()}
    tr, model, pde = trainer()
    tr._sample = lambda n, xb=xb, tb=tb: (xb, tb)
    replay, losses = tr.make_graphed_step(NPTS, warmup=1)
    for _ in range(3):
        replay()
    torch.cuda.synchronize()
    assert torch.equal(_theta(model), eager), f"max |d theta| = {float((_theta(model) - eager).abs().max()):.3e}"
    assert {k: float(v) for k, v in losses.items()} == eager_losses
    # and the plain train_step (no fork) agrees to rounding
    tr, model, pde = trainer()
    tr._build_flat_state()
    for _ in range(4):
        tr.train_step(xb, tb)
    assert rel_l2(_theta(model), eager, label=f"{name}: train_step vs forked launch list", tol=TOL) <= TOL


def test_one_lbfgs_step_matches_the_eager_closure(dev):
    from pinnrl_amd.training import PDETrainer

    thetas = []
    for fast in (False, None):
        cfg, model, pde, spec, sd = _build("heat2d", dev, optimizer="lbfgs", lr=0.5)
        cfg.training.gradient_clipping = 0.0
        cfg.training.lbfgs.max_iter, cfg.training.lbfgs.history_size = 4, 10
        tr = PDETrainer(model, pde, {}, cfg, device=dev, fast_step=fast)
        assert tr._is_lbfgs
        if fast is None:
            assert tr._manual_step_unsupported() is None, tr._manual_step_unsupported()
            tr._build_flat_state()
        xb, tb = _batches(pde, 1, seed=9)[0]
        out = tr.train_step(xb, tb)
        assert math.isfinite(float(out["total"]))
        thetas.append(_theta(model))
    e = rel_l2(thetas[1], thetas[0], label="heat2d: theta after one L-BFGS step", tol=1e-4)
    assert e <= 1e-4, f"{e:.2e}"
    assert not torch.equal(thetas[1], _theta(_build("heat2d", dev)[1]))  # the step moved theta


@pytest.mark.parametrize("name", ["burgers2d", "heat3d"])
def test_residual_based_sampler_runs_on_the_launch_list(name, dev):
    from pinnrl_amd.training import PDETrainer

    cfg, model, pde, spec, sd = _build(name, dev, sampler="residual_based")
    tr = PDETrainer(model, pde, {}, cfg, device=dev)
    assert tr._manual_step_unsupported() is None
    tr._build_flat_state()
    torch.manual_seed(1)
    x, t = tr._sample(64)
    dim = PROBLEMS[name]["dim"]
    assert x.shape == (64, dim) and t.shape == (64, 1) and x.is_cuda
    assert float(x.min()) >= 0.0 and float(x.max()) <= 1.0 and float(t.min()) >= 0.0 and float(t.max()) <= 0.5
    out = tr.train_step(x, t)
    assert all(math.isfinite(float(out[k])) for k in ("residual", "boundary", "initial", "total"))


def test_training_lowers_the_loss_and_the_error(dev):
    """200 Adam steps on one batch of 1 024 points (fourier 2 x 32): the total loss on that batch and the error against the
    exact solution on one set of validation points both end below their values at theta_0."""
    from pinnrl_amd.training import PDETrainer

    cfg, model, pde, spec, sd = _build("heat2d", dev, lr=2e-3)
    torch.manual_seed(2)
    xb, tb = pde._sample_uniform(1024)
    assert xb.shape == (1024, 2)

    def measure():
        with torch.no_grad():
            total = float(pde.compute_loss(model, xb, tb)["total"])
        torch.manual_seed(123)  # validate() draws its points: the same ones both times
        return total, pde.validate(model, 1000)["l2_error"]

    loss0, err0 = measure()
    tr = PDETrainer(model, pde, {}, cfg, device=dev)
    assert tr._manual_step_unsupported() is None
    tr._build_flat_state()
    for _ in range(200):
        tr.train_step(xb, tb)
    loss1, err1 = measure()
    print(f"total loss {loss0:.4e} -> {loss1:.4e}; l2_error {err0:.4e} -> {err1:.4e}")
    assert math.isfinite(loss1) and loss1 < loss0 and err1 < err0
