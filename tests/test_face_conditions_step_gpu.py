"""`face_conditions=` end to end on the GPU.  Four problems on 2 x 32 / 3 x 32 networks, 4 boundary points and 5 initial points
per axis:

  neumann2d  2-D heat, every face Neumann 0, fourier; exact exp(-2 alpha pi^2 t) cos(pi x) cos(pi y)
  mixed2d    2-D heat, feedforward, huber loss: x_lo Dirichlet with a callable of (y, t), x_hi Robin (alpha 1, beta 0.5, value
             0.2), y periodic with the derivative
  heat3d     3-D heat, fourier: z_lo Neumann with a callable, z_hi Dirichlet 0, x and y periodic
  cavity     TermPDESystem (u, v, p) in 2-D: u, v Dirichlet 0 by default and no condition on p; u = 1 on y_hi; dp/dn = 0 on
             x_hi; initial condition on u and v — 9 boundary + 2 initial terms, above the 8 of pinn_jet_losses

against torch fp64 autograd through `oracle.network_forward` with the conditions written out (every loss term, the total, d total
/ d theta: 1e-5), the launch list against the autograd step (theta after 1 / 3 / 10 Adam steps 1e-5, one L-BFGS step 1e-4: the
bars of tests/test_term_step_gpu.py), a captured step against the eager launch list bit for bit; 200 Adam steps on neumann2d
lower the loss and the error; `model.jets(..., axis=1)` has exact first-order gradients and refuses second-order ones."""

import math

import pytest
import torch

from conftest import rel_err, rel_l2

pytestmark = pytest.mark.gpu

TOL = 1e-5
NPTS = 128
PI = math.pi
DELTA = 0.05  # huber: both branches occur at theta_0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _cosines(x):
    return torch.prod(torch.cos(PI * x), dim=1)


def _inlet(x, t):  # x_lo of mixed2d: a function of (y, t)
    return torch.sin(PI * x[:, 1]) * (1.0 + t[:, 0])


def _flux(x, t):  # z_lo of heat3d: the outward normal derivative -u_z
    return 0.5 * torch.cos(PI * x[:, 0]) * x[:, 1] - t[:, 0]


def _cavity_ic(x):
    return torch.stack([torch.sin(PI * x[:, 0]) * x[:, 1], -0.5 * torch.sin(PI * x[:, 1]) * x[:, 0]], 1)


HEAT = lambda dim: [(1.0, ("u_t",))] + [((-1.0, "alpha"), (f"u_{ax}{ax}",)) for ax in "xyz"[:dim]]  # noqa: E731
D0 = {"type": "dirichlet", "value": 0.0}
N0 = {"type": "neumann", "value": 0.0}
PROBLEMS = {
    "neumann2d": dict(dim=2, arch="fourier", layers=3, loss="mse", ic=_cosines, faces={"default": N0},
                      exact=lambda x, t: torch.exp(-2 * 0.05 * PI**2 * t[:, 0]) * _cosines(x)),
    "mixed2d": dict(dim=2, arch="feedforward", layers=2, loss="huber", ic=_cosines,
                    faces={"x_lo": {"type": "dirichlet", "value": _inlet}, "x_hi": {"type": "robin", "alpha": 1.0, "beta": 0.5, "value": 0.2},
                           "y": {"type": "periodic", "derivative": True}}),
    "heat3d": dict(dim=3, arch="fourier", layers=2, loss="mse", ic=_cosines,
                   faces={"z_lo": {"type": "neumann", "value": _flux}, "z_hi": D0, "default": {"type": "periodic"}}),
    "cavity": dict(dim=2, arch="fourier", layers=3, loss="mse", ic=_cavity_ic, fields=("u", "v", "p"),
                   faces={"default": {"u": D0, "v": D0, "p": None}, "y_hi": {"u": {"type": "dirichlet", "value": 1.0}}, "x_hi": {"p": N0}},
                   equations=[
                       [(1.0, ("u_t",)), (1.0, ("u", "u_x")), (1.0, ("v", "u_y")), (1.0, ("p_x",)), ((-1.0, "alpha"), ("u_xx",)), ((-1.0, "alpha"), ("u_yy",))],
                       [(1.0, ("v_t",)), (1.0, ("u", "v_x")), (1.0, ("v", "v_y")), (1.0, ("p_y",)), ((-1.0, "alpha"), ("v_xx",)), ((-1.0, "alpha"), ("v_yy",))],
                       [(1.0, ("u_x",)), (1.0, ("v_y",))]]),
}
ALPHA = 0.05


def _spec(name):
    import oracle as O

    p = PROBLEMS[name]
    kw = dict(input_dim=p["dim"] + 1, hidden_dim=32, num_layers=p["layers"], activation="tanh", output_dim=len(p.get("fields", "u")))
    if p["arch"] == "fourier":
        return O.ArchSpec("fourier", mapping_size=8, scale=1.0, **kw)
    return O.ArchSpec("feedforward", **kw)


def _build(name, dev, optimizer="adam", lr=1e-3, seed=3):
    """cfg, model (theta_0 from the oracle's initialiser under `seed`), the PDE with its face conditions."""
    import oracle as O
    from pinnrl_amd import pdes as P
    from pinnrl_amd.config import Config, ModelConfig, TrainingConfig
    from pinnrl_amd.neural_networks import PINNModel

    p, spec = PROBLEMS[name], _spec(name)
    cfg = Config.__new__(Config)
    cfg.device = dev
    cfg.training = TrainingConfig(learning_rate=lr, gradient_clipping=1.0, optimizer=optimizer)
    cfg.training.loss_function, cfg.training.huber_delta = p["loss"], DELTA
    pc = P.PDEConfig(name=name, domain=[(0.0, 1.0)] * p["dim"], time_domain=(0.0, 0.5), parameters={"alpha": ALPHA}, boundary_conditions={},
                     initial_condition={}, exact_solution={}, dimension=p["dim"], device=dev, training=cfg.training)
    if "fields" in p:
        pde = P.TermPDESystem(pc, p["fields"], p["equations"], p["ic"], initial_condition_fields=("u", "v"), boundary_points_per_axis=4,
                              initial_points_per_axis=5, face_conditions=p["faces"])
    else:
        pde = P.TermPDEnD(pc, HEAT(p["dim"]), p["ic"], exact_solution_fn=p.get("exact"), boundary_points_per_axis=4,
                          initial_points_per_axis=5, face_conditions=p["faces"])
    cfg.model = ModelConfig(input_dim=spec.input_dim, hidden_dim=spec.hidden_dim, output_dim=spec.output_dim, num_layers=spec.num_layers,
                            activation=spec.activation, architecture=spec.architecture)
    cfg.model.mapping_size, cfg.model.scale = spec.mapping_size, spec.scale
    model = PINNModel(cfg, device=dev)
    model.load_state_dict({k: v.to(dev) for k, v in O.init_state_dict(spec, seed=seed).items()})
    return cfg, model, pde


def _theta(model):
    return torch.cat([p.detach().flatten().cpu() for _, p in model.named_parameters()])


def _points(name, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, PROBLEMS[name]["dim"], generator=g), torch.rand(n, 1, generator=g) * 0.5


def _fixed_points(pde):
    pts = pde._system_points() if hasattr(pde, "_system_points") else pde._nd_points()
    return {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in pts.items()}


_fp64 = {}


def _oracle(name, pde):
    """fp64 loss terms, total and d total / d theta by autograd through the oracle's network, every condition written out by
    hand on the PDE's own fixed points (face (a, side) is the range [(2a + side) nf, (2a + side + 1) nf)); once per problem."""
    import oracle as O

    if name in _fp64:
        return _fp64[name]
    p, spec = PROBLEMS[name], _spec(name)
    params = {k: v.double().requires_grad_(k != "model.fourier.B") for k, v in O.init_state_dict(spec, seed=3).items()}
    d = lambda y, w: torch.autograd.grad(y, w, torch.ones_like(y), create_graph=True)[0]  # noqa: E731
    if p["loss"] == "huber":
        l = lambda e: torch.nn.functional.huber_loss(e, torch.zeros_like(e), delta=DELTA)  # noqa: E731, E741
    else:
        l = lambda e: torch.mean(e**2)  # noqa: E731, E741
    # the residual on seeded collocation points
    x32, t32 = _points(name, NPTS, 17)
    x, t = x32.double().requires_grad_(True), t32.double().requires_grad_(True)
    out = O.network_forward(spec, params, torch.cat([x, t], 1))
    lap = lambda f: sum(d(d(f, x)[:, a : a + 1], x)[:, a : a + 1] for a in range(p["dim"]))  # noqa: E731
    if name == "cavity":
        u, v, pr = out[:, 0:1], out[:, 1:2], out[:, 2:3]
        gu, gv, gp = d(u, x), d(v, x), d(pr, x)
        r = [d(u, t) + u * gu[:, 0:1] + v * gu[:, 1:2] + gp[:, 0:1] - ALPHA * lap(u),
             d(v, t) + u * gv[:, 0:1] + v * gv[:, 1:2] + gp[:, 1:2] - ALPHA * lap(v), gu[:, 0:1] + gv[:, 1:2]]
        res = sum(l(e) for e in r)
    else:
        res = l(d(out, t) - ALPHA * lap(out))
    # the boundary and initial terms on the fixed points
    pts = _fixed_points(pde)
    xb, tb = pts["x"].double().requires_grad_(True), pts["t"].double()
    ub = O.network_forward(spec, params, torch.cat([xb, tb], 1))
    nbc, nf = pts["n_bc"], pts["n_face"]
    face = lambda a, side: slice((2 * a + side) * nf, (2 * a + side + 1) * nf)  # noqa: E731
    X_LO, X_HI, Y_LO, Y_HI, Z_LO, Z_HI = (face(a, s) for a in range(3) for s in range(2))
    g = d(ub[:, 0:1], xb)  # (n, dim): du/dx_a of the first field
    u0 = ub[:, 0]
    xf, tf = pts["x"], pts["t"]
    if name == "neumann2d":  # du/dn = 0: -u_x on x_lo, +u_x on x_hi, -u_y on y_lo, +u_y on y_hi
        bnd = [l(-g[X_LO, 0]), l(g[X_HI, 0]), l(-g[Y_LO, 1]), l(g[Y_HI, 1])]
    elif name == "mixed2d":
        bnd = [l(u0[X_LO] - _inlet(xf[X_LO], tf[X_LO]).double()), l(u0[X_HI] + 0.5 * g[X_HI, 0] - 0.2),
               l(u0[Y_LO] - u0[Y_HI]), l(g[Y_LO, 1] - g[Y_HI, 1])]
    elif name == "heat3d":
        bnd = [l(u0[X_LO] - u0[X_HI]), l(u0[Y_LO] - u0[Y_HI]), l(-g[Z_LO, 2] - _flux(xf[Z_LO], tf[Z_LO]).double()), l(u0[Z_HI])]
    else:
        v0, p_x = ub[:, 1], d(ub[:, 2:3], xb)[:, 0]
        bnd = [l(u0[X_LO]), l(u0[X_HI]), l(u0[Y_LO]), l(u0[Y_HI] - 1.0), l(v0[X_LO]), l(v0[X_HI]), l(v0[Y_LO]), l(v0[Y_HI]), l(p_x[X_HI])]
    if name == "cavity":
        ini = [l(ub[nbc:, c] - pts["u0"][c].double()) for c in range(2)]
    else:
        ini = [l(u0[nbc:] - pts["u0"].double())]
    lw = pde._loss_weights()
    total = lw.get("pde", lw.get("residual", 1.0)) * res + lw.get("boundary", 10.0) * sum(bnd) + lw.get("initial", 10.0) * sum(ini)
    names = [k for k, v in params.items() if v.requires_grad]
    grad = torch.autograd.grad(total, [params[k] for k in names])
    _fp64[name] = {"x": x32, "t": t32, "residual": float(res), "boundary": float(sum(bnd)), "initial": float(sum(ini)),
                   "terms": [float(v) for v in bnd + ini], "total": float(total), "names": names,
                   "grad": torch.cat([v.flatten() for v in grad])}
    return _fp64[name]


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_losses_and_gradient_match_fp64_autograd(name, dev):
    """`compute_loss` under autograd, then the launch list on the same points: every term of the pinn_face_losses call, the
    summary and the flat gradient."""
    from pinnrl_amd import engine as E
    from pinnrl_amd.training import PDETrainer

    cfg, model, pde = _build(name, dev)
    o = _oracle(name, pde)
    x, t = o["x"].to(dev), o["t"].to(dev)
    losses = pde.compute_loss(model, x, t)
    errs = {k: rel_err(float(losses[k].detach()), o[k], label=f"{name}: {k} loss", tol=TOL) for k in ("residual", "boundary", "initial", "total")}
    model.zero_grad()
    losses["total"].backward()
    got = torch.cat([dict(model.named_parameters())[k].grad.flatten().cpu() for k in o["names"]])
    e_g = rel_l2(got, o["grad"], label=f"{name}: d total / d theta (autograd)", tol=TOL)
    print(f"{name}: autograd losses {', '.join(f'{k} {v:.2e}' for k, v in errs.items())}, gradient {e_g:.2e}")
    assert all(v <= TOL for v in errs.values()), errs
    assert e_g <= TOL, f"gradient: {e_g:.2e}"
    # the launch list
    tr = PDETrainer(model, pde, {}, cfg, device=dev)
    assert tr._manual_step_unsupported() is None, tr._manual_step_unsupported()
    tr._build_flat_state()
    F, prog = tr._flat, model.program()
    ch = tr._chain(NPTS)
    assert len(o["terms"]) == ch["term_losses"].numel() and ch["n_bc"] == len(o["terms"]) - (2 if name == "cavity" else 1)
    tr._loss_grad_launches(x, t, F, prog, pde._pde_desc(), ch)
    torch.cuda.synchronize()
    e_terms = [rel_err(float(a), b, label=f"{name}: loss term {k}", tol=TOL) for k, (a, b) in enumerate(zip(ch["term_losses"].cpu(), o["terms"]))]
    summ = dict(zip(("residual", "boundary", "initial", "total"), F["summary"].cpu().tolist()))
    e_sum = {k: rel_err(summ[k], o[k], label=f"{name}: {k} (launch list)", tol=TOL) for k in summ}
    by_name = {"model." + k: v for k, v in zip(prog.names, E.split_flat_grad(prog, F["grad"][: F["n"]]))}  # the inner network's names
    flat = torch.cat([by_name[k].flatten().cpu() for k in o["names"]])
    e_f = rel_l2(flat, o["grad"], label=f"{name}: d total / d theta (launch list)", tol=TOL)
    print(f"{name}: launch list terms {max(e_terms):.2e}, summary {max(e_sum.values()):.2e}, gradient {e_f:.2e}")
    assert max(e_terms) <= TOL, e_terms
    assert all(v <= TOL for v in e_sum.values()), e_sum
    assert e_f <= TOL, f"gradient: {e_f:.2e}"


def _batches(pde, n, seed=5):
    torch.manual_seed(seed)
    return [pde._sample_uniform(NPTS) for _ in range(n)]


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_adam_launch_list_matches_the_autograd_step(name, dev):
    from pinnrl_amd.training import PDETrainer

    runs, batches = {}, None
    for key, fast in (("list", None), ("autograd", False)):
        cfg, model, pde = _build(name, dev)
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


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_one_lbfgs_step_matches_the_eager_closure(name, dev):
    from pinnrl_amd.training import PDETrainer

    thetas = []
    for fast in (False, None):
        cfg, model, pde = _build(name, dev, optimizer="lbfgs", lr=0.5)
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
    e = rel_l2(thetas[1], thetas[0], label=f"{name}: theta after one L-BFGS step", tol=1e-4)
    print(f"{name}: theta after one L-BFGS step {e:.2e}")
    assert e <= 1e-4, f"{e:.2e}"
    assert not torch.equal(thetas[1], _theta(_build(name, dev)[1]))  # the step moved theta


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_captured_step_replays_the_eager_launch_list_bit_for_bit(name, dev):
    from pinnrl_amd.training import PDETrainer

    def trainer():
        cfg, model, pde = _build(name, dev)
        model.set_deterministic(True)  # fixed-order weight-gradient sums, kept when the flat state rebuilds the program
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
    assert not torch.equal(eager, _theta(_build(name, dev)[1]))  # the steps moved theta


def test_training_lowers_the_loss_and_the_error(dev):
    """200 Adam steps on one batch of 1 024 points, all faces insulated: the total loss on that batch and the error against the
    exact solution on one set of validation points both end below their values at theta_0."""
    from pinnrl_amd.training import PDETrainer

    cfg, model, pde = _build("neumann2d", dev, lr=2e-3)
    torch.manual_seed(2)
    xb, tb = pde._sample_uniform(1024)

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


def test_jets_along_an_axis_are_differentiable_once(dev):
    """`model.jets(x, t, 0, 1, axis=1)` = [u, u_y]: d<c, jets>/d(theta, x, t) against fp64 autograd; a second derivative raises."""
    import oracle as O

    cfg, model, pde = _build("mixed2d", dev)
    spec = _spec("mixed2d")
    x32, t32 = _points("mixed2d", 97, 23)
    g = torch.Generator().manual_seed(4)
    c32 = torch.randn(2, 97, generator=g)
    x, t = x32.to(dev).requires_grad_(True), t32.to(dev).requires_grad_(True)
    J = model.jets(x, t, 0, 1, axis=1)
    assert J.shape == (2, 97) and J.requires_grad
    params = [p for _, p in model.named_parameters()]
    grads = torch.autograd.grad((J * c32.to(dev)).sum(), [x, t] + params, create_graph=True)
    # fp64
    sd = {k: v.double().requires_grad_(True) for k, v in O.init_state_dict(spec, seed=3).items()}
    xd, td = x32.double().requires_grad_(True), t32.double().requires_grad_(True)
    u = O.network_forward(spec, sd, torch.cat([xd, td], 1))
    u_y = torch.autograd.grad(u.sum(), xd, create_graph=True)[0][:, 1]
    names = [k for k, _ in model.named_parameters()]
    want = torch.autograd.grad((torch.stack([u[:, 0], u_y]) * c32.double()).sum(), [xd, td] + [sd[k] for k in names])
    assert rel_l2(J.detach().cpu(), torch.stack([u[:, 0], u_y]).detach(), label="jets along axis 1", tol=TOL) <= TOL
    for what, a, b in (("x", grads[0], want[0]), ("t", grads[1], want[1]),
                       ("theta", torch.cat([v.flatten() for v in grads[2:]]), torch.cat([v.flatten() for v in want[2:]]))):
        e = rel_l2(a.detach().cpu(), b, label=f"d<c, jets along axis 1>/d{what}", tol=TOL)
        print(f"d<c, jets>/d{what}: {e:.2e}")
        assert e <= TOL, (what, e)
    # parameters alone (the branch without input cotangents)
    J2 = model.jets(x32.to(dev), t32.to(dev), 0, 1, axis=1)
    gp = torch.autograd.grad((J2 * c32.to(dev)).sum(), params)
    assert rel_l2(torch.cat([v.flatten() for v in gp]).cpu(), torch.cat([v.flatten() for v in want[2:]])) <= TOL
    for first in (grads[0], grads[1], grads[2]):
        with pytest.raises(NotImplementedError, match="not differentiable again"):
            torch.autograd.grad(first.sum(), [x], allow_unused=True)
