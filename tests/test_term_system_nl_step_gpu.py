"""Nonlinear functions of the unknowns in system residuals end to end on the GPU: three problems on 3 x 32 feedforward networks,
200 points, time_domain (0, 0.5), built like tests/test_term_system_fn_step_gpu.py —

  bratu1d   u_t - u_xx - lam e^(2 + u / 2) = 0 in 1-D, one field (`TermPDESystem`), one EXP; Dirichlet ends
  monod2d   u_t - D (u_xx + u_yy) + R u / (K + u) = 0 in 2-D, one field, Monod kinetics through RECIP with shift K = 2; Dirichlet faces
  euler     compressible flow along x in primitive variables (rho, u, p) on a 2-D box (`TermPDESystemMixed`):
            rho_t + u rho_x + rho u_x,  u_t + u u_x + p_x / (2 + rho) - nu u_xy,  p_t + u p_x + gamma p u_x - q e^(1.5 - Ea / (2 + rho)):
            ir = 1 / (2 + rho) and the nested Arrhenius-type source exp(1.5 - Ea ir); `face_conditions`: Dirichlet on x for all
            fields, Neumann on y for u, Dirichlet on y_lo only for p, nothing on y for rho

against torch fp64 autograd through `oracle.network_forward` with the formulas written out in torch (the oracle asserts that
every argument of a nonlinear function is >= 0.5): the (N, E) residuals, the four losses and d total / d theta at 1e-5 (the bar of
tests/test_term_system_fn_step_gpu.py); three Adam steps of the launch list against the autograd step at that bar; a captured step
that replays the eager launch list bit for bit; one L-BFGS step against the eager closure at that test's 1e-4; and a shift
rewritten in place in `pde.nl_values` between steps: the eager step and the replay both follow it."""

import math

import pytest
import torch

from conftest import rel_err, rel_l2

pytestmark = pytest.mark.gpu

TOL = 1e-5
NPTS = 200
PI = math.pi
PARAMS = {"lam": 0.7, "D": 0.05, "R": 0.9, "K": 2.0, "gamma": 1.4, "Ea": 0.8, "nu": 0.02, "q": 0.3}
D0 = {"type": "dirichlet", "value": 0.0}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


EULER = [[(1.0, ("rho_t",)), (1.0, ("u", "rho_x")), (1.0, ("rho", "u_x"))],
         [(1.0, ("u_t",)), (1.0, ("u", "u_x")), (1.0, ("ir", "p_x")), ((-1.0, "nu"), ("u_xy",))],
         [(1.0, ("p_t",)), (1.0, ("u", "p_x")), ((1.0, "gamma"), ("p", "u_x")), ((-1.0, "q"), ("arr",))]]
PROBLEMS = {
    "bratu1d": dict(dim=1, fields=("u",), mixed=False, equations=[[(1.0, ("u_t",)), (-1.0, ("u_xx",)), ((-1.0, "lam"), ("eu",))]],
                    nonlinear={"eu": ("exp", "u", {"shift": 2.0, "scale": 0.5})}, bcs={"dirichlet": {"type": "fixed", "value": 0.0}},
                    faces=None, ic=lambda x: torch.sin(PI * x[:, :1])),
    "monod2d": dict(dim=2, fields=("u",), mixed=False,
                    equations=[[(1.0, ("u_t",)), ((-1.0, "D"), ("u_xx",)), ((-1.0, "D"), ("u_yy",)), ((1.0, "R"), ("u", "m"))]],
                    nonlinear={"m": ("recip", "u", {"shift": "K"})}, bcs={"dirichlet": {"type": "fixed", "value": 0.0}}, faces=None,
                    ic=lambda x: (torch.sin(PI * x[:, 0]) * torch.sin(PI * x[:, 1])).unsqueeze(1)),
    "euler": dict(dim=2, fields=("rho", "u", "p"), mixed=True, equations=EULER,
                  nonlinear={"ir": ("recip", "rho", {"shift": 2.0}), "arr": ("exp", "ir", {"shift": 1.5, "scale": (-1.0, "Ea")})}, bcs={},
                  faces={"x": D0, "y": {"rho": None, "u": {"type": "neumann", "value": 0.1}, "p": D0}, "y_hi": {"p": None}},
                  ic=lambda x: torch.stack([0.2 * torch.sin(PI * x[:, 0]), torch.sin(PI * x[:, 0]) * x[:, 1], 0.5 * torch.cos(PI * x[:, 0])], 1)),
}
LAUNCHES = {"bratu1d": 1, "monod2d": 2, "euler": 5}  # a nonlinear function adds no network launch (u of euler: x, y and the pair)


def _spec(name):
    import oracle as O

    p = PROBLEMS[name]
    return O.ArchSpec("feedforward", input_dim=p["dim"] + 1, hidden_dim=32, num_layers=3, activation="tanh", output_dim=len(p["fields"]))


def _build(name, dev, optimizer="adam", lr=1e-3, seed=3):
    """cfg, model (theta_0 from the oracle's initialiser under `seed`), the PDE, the oracle's ArchSpec."""
    import oracle as O
    from pinnrl_amd import pdes as P
    from pinnrl_amd.config import Config, ModelConfig, TrainingConfig
    from pinnrl_amd.neural_networks import PINNModel

    p, spec = PROBLEMS[name], _spec(name)
    dim = p["dim"]
    cfg = Config.__new__(Config)
    cfg.device = dev
    cfg.training = TrainingConfig(learning_rate=lr, gradient_clipping=1.0, optimizer=optimizer)
    pc = P.PDEConfig(name=name, domain=[(0.0, 1.0)] * dim, time_domain=(0.0, 0.5), parameters=dict(PARAMS), boundary_conditions=dict(p["bcs"]),
                     initial_condition={}, exact_solution={}, dimension=dim, device=dev, training=cfg.training)
    cls = P.TermPDESystemMixed if p["mixed"] else P.TermPDESystem
    pde = cls(pc, p["fields"], p["equations"], p["ic"], boundary_points_per_axis=4, initial_points_per_axis=5, face_conditions=p["faces"],
              nonlinear=p["nonlinear"])
    assert pc.output_dim == len(p["fields"])
    cfg.model = ModelConfig(input_dim=spec.input_dim, hidden_dim=spec.hidden_dim, output_dim=pc.output_dim, num_layers=spec.num_layers,
                            activation=spec.activation, architecture=spec.architecture)
    cfg.model.mapping_size, cfg.model.scale = spec.mapping_size, spec.scale
    model = PINNModel(cfg, device=dev)
    model.load_state_dict({k: v.to(dev) for k, v in O.init_state_dict(spec, seed=seed).items()})
    return cfg, model, pde, spec


def _theta(model):
    return torch.cat([p.detach().flatten().cpu() for _, p in model.named_parameters()])


def _points(name, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, PROBLEMS[name]["dim"], generator=g), torch.rand(n, 1, generator=g) * 0.5


_fp64 = {}


def _oracle(name, pde):
    """Residuals (N, E), loss terms, total and d total / d theta by chained fp64 autograd.grad through the oracle's network on
    200 seeded points and the system's own fixed points, once per problem."""
    import oracle as O

    if name in _fp64:
        return _fp64[name]
    p, spec = PROBLEMS[name], _spec(name)
    dim, C = p["dim"], len(p["fields"])
    f64 = torch.float64
    params = {k: v.to(f64).requires_grad_(True) for k, v in O.init_state_dict(spec, seed=3).items()}
    x32, t32 = _points(name, NPTS, 17)
    x, t = x32.to(f64).requires_grad_(True), t32.to(f64).requires_grad_(True)
    out = O.network_forward(spec, params, torch.cat([x, t], 1))
    d = lambda y, w: torch.autograd.grad(y, w, torch.ones_like(y), create_graph=True)[0]  # noqa: E731
    g = [d(out[:, c : c + 1], x) for c in range(C)]                                        # g[c][:, a] = d_a of field c
    h = [[d(g[c][:, a : a + 1], x) for a in range(dim)] for c in range(C)]                 # h[c][a][:, b] = d_b d_a of field c
    ut = [d(out[:, c : c + 1], t) for c in range(C)]
    P_ = PARAMS
    if name == "bratu1d":
        args = [2.0 + 0.5 * out[:, 0:1]]
        r = [ut[0] - h[0][0][:, 0:1] - P_["lam"] * torch.exp(args[0])]
    elif name == "monod2d":
        args = [P_["K"] + out[:, 0:1]]
        r = [ut[0] - P_["D"] * (h[0][0][:, 0:1] + h[0][1][:, 1:2]) + P_["R"] * out[:, 0:1] / args[0]]
    else:
        rho, u, pr = out[:, 0:1], out[:, 1:2], out[:, 2:3]
        args = [2.0 + rho]
        ir = 1.0 / args[0]
        args.append(1.5 - P_["Ea"] * ir)
        r = [ut[0] + u * g[0][:, 0:1] + rho * g[1][:, 0:1],
             ut[1] + u * g[1][:, 0:1] + ir * g[2][:, 0:1] - P_["nu"] * h[1][0][:, 1:2],
             ut[2] + u * g[2][:, 0:1] + P_["gamma"] * pr * g[1][:, 0:1] - P_["q"] * torch.exp(args[1])]
    assert all(float(a.detach().min()) >= 0.5 for a in args), [float(a.detach().min()) for a in args]
    r = torch.cat(r, 1)
    res = sum(torch.mean(r[:, e] ** 2) for e in range(r.shape[1]))
    pts = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in pde._system_points().items()}
    xb, tb = pts["x"].to(f64).requires_grad_(True), pts["t"].to(f64)
    ub = O.network_forward(spec, params, torch.cat([xb, tb], 1))
    nbc, nf = pts["n_bc"], pts["n_face"]
    l = lambda e: torch.mean(e**2)  # noqa: E731, E741
    if p["faces"] is None:
        bnd = sum(l(ub[:nbc, c]) for c in range(C))
    else:  # face (a, side) is the range [(2a + side) nf, (2a + side + 1) nf); d/dn = -d/dy on y_lo, +d/dy on y_hi
        face = lambda a, side: slice((2 * a + side) * nf, (2 * a + side + 1) * nf)  # noqa: E731
        X_LO, X_HI, Y_LO, Y_HI = (face(a, s) for a in range(2) for s in range(2))
        u_y = d(ub[:, 1:2], xb)[:, 1]
        rho0, u0, p0 = ub[:, 0], ub[:, 1], ub[:, 2]
        bnd = sum([l(rho0[X_LO]), l(rho0[X_HI]), l(u0[X_LO]), l(u0[X_HI]), l(-u_y[Y_LO] - 0.1), l(u_y[Y_HI] - 0.1), l(p0[X_LO]), l(p0[X_HI]),
                   l(p0[Y_LO])])
    ini = sum(l(ub[nbc:, c] - pts["u0"][c].to(f64)) for c in range(C))
    lw = pde._loss_weights() or {}
    total = lw.get("pde", lw.get("residual", 1.0)) * res + lw.get("boundary", 10.0) * bnd + lw.get("initial", 10.0) * ini
    names = list(params)
    res_grad = torch.autograd.grad(res, [params[k] for k in names], retain_graph=True, allow_unused=True)
    res_grad = [torch.zeros_like(params[k]) if v is None else v for k, v in zip(names, res_grad)]
    grad = torch.autograd.grad(total, [params[k] for k in names])
    cat = lambda gs: torch.cat([v.flatten() for v in gs]).double()  # noqa: E731
    _fp64[name] = {"x": x32, "t": t32, "r": r.detach(), "residual": float(res.detach()), "boundary": float(bnd.detach()),
                   "initial": float(ini.detach()), "total": float(total.detach()), "names": names, "grad": cat(grad), "res_grad": cat(res_grad)}
    return _fp64[name]


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_residuals_losses_and_gradient_match_fp64_autograd(name, dev):
    from pinnrl_amd import engine as E

    cfg, model, pde, spec = _build(name, dev)
    o = _oracle(name, pde)
    x, t = o["x"].to(dev), o["t"].to(dev)
    n_eq = pde.n_equations
    r = pde.compute_residual(model, x, t)
    assert r.shape == (NPTS, n_eq) and r.requires_grad
    e_r = max(rel_l2(r.detach().cpu()[:, e], o["r"][:, e], label=f"{name}: residual {e}", tol=TOL) for e in range(n_eq))
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
    # the raw chain: residual_loss_grad takes the new entry point
    prog, td = model.program(), pde._pde_desc()
    assert type(td) is E.NlSystemTermDesc and td.nl_values is pde.nl_values and len(td.launches()) == LAUNCHES[name]
    flat = E.new_flat_grad(prog, dev)
    r2, s2 = E.residual_loss_grad(prog, td, x, t, 1.0 / NPTS, flat, want_residual=True)
    assert torch.equal(r2, r.detach()) and rel_err(float(s2) / NPTS, o["residual"]) <= TOL
    by_name = {"model." + k: v for k, v in zip(prog.names, E.split_flat_grad(prog, flat))}
    e_c = rel_l2(torch.cat([by_name[k].flatten().cpu() for k in o["names"]]), o["res_grad"], label=f"{name}: d residual loss / d theta (chain)",
                 tol=TOL)
    print(f"{name}: residual_loss_grad against fp64: {e_c:.2e}")
    assert e_c <= TOL, f"gradient of the residual chain: {e_c:.2e}"
    # the same call with the values given explicitly: the same bits
    r3, _ = E.term_residual_system_nl(td, E._system_jets(prog, td, x, t), None, pde.nl_values, x, t)
    assert torch.equal(r3, r.detach())
    # the backward of the residual tensor in a downstream graph of the caller's
    model.zero_grad()
    wgt = torch.linspace(0.5, 1.5, NPTS * n_eq, device=dev).reshape(NPTS, n_eq)
    (pde.compute_residual(model, x, t) * wgt).sum().backward()
    flat2 = E.new_flat_grad(prog, dev)
    E.residual_backward(prog, td, x, t, wgt, flat2)
    for p_, g_ in zip(prog.tensors, E.split_flat_grad(prog, flat2)):
        if g_ is not None and p_.grad is not None:
            assert rel_l2(p_.grad.cpu(), g_.double().cpu()) <= 1e-6
    flat3 = E.new_flat_grad(prog, dev)
    E.residual_backward(prog, td, x, t, 2.0 * r.detach() / NPTS, flat3)
    assert rel_l2(flat.cpu(), flat3.double().cpu()) <= 1e-6


def _batches(pde, n, seed=5):
    torch.manual_seed(seed)
    return [pde._sample_uniform(NPTS) for _ in range(n)]


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_adam_launch_list_matches_the_autograd_step(name, dev):
    from pinnrl_amd.training import PDETrainer

    runs, batches = {}, None
    for key, fast in (("list", None), ("autograd", False)):
        cfg, model, pde, spec = _build(name, dev)
        batches = batches or _batches(pde, 3)
        tr = PDETrainer(model, pde, {}, cfg, device=dev, fast_step=fast)
        if fast is None:
            assert tr._manual_step_unsupported() is None, tr._manual_step_unsupported()
            tr._build_flat_state()
        thetas, losses = {}, []
        for step, (xb, tb) in enumerate(batches, start=1):
            out = tr.train_step(xb, tb)
            losses.append({k: float(out[k].detach()) for k in ("residual", "boundary", "initial", "total")})
            thetas[step] = _theta(model)
        assert (getattr(tr, "_flat", None) is not None) == (fast is None)
        runs[key] = (thetas, losses)
    for step in (1, 2, 3):
        e = rel_l2(runs["list"][0][step], runs["autograd"][0][step], label=f"{name}: theta vs autograd, step {step}", tol=TOL)
        print(f"{name} step {step}: theta vs autograd {e:.2e}")
        assert e <= TOL, (step, e)
    for step, (got, want) in enumerate(zip(runs["list"][1], runs["autograd"][1]), start=1):
        for k in got:
            assert abs(got[k] - want[k]) <= 5e-5 * abs(want[k]), (step, k, got[k], want[k])


def _graph_trainer(name, dev):
    from pinnrl_amd.training import PDETrainer

    cfg, model, pde, spec = _build(name, dev)
    model.set_deterministic(True)  # fixed-order weight-gradient sums, kept when the flat state rebuilds the program
    tr = PDETrainer(model, pde, {}, cfg, device=dev)
    assert tr._manual_step_unsupported() is None
    return tr, model, pde


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_captured_step_replays_the_eager_launch_list_bit_for_bit(name, dev):
    tr, model, pde = _graph_trainer(name, dev)
    xb, tb = _batches(pde, 1, seed=0)[0]
    tr._build_flat_state()
    side = torch.cuda.Stream(device=dev)
    for _ in range(4):  # the eager launch list with the fork the captured step has
        tr._manual_launches(xb, tb, side=side)
    torch.cuda.synchronize()
    eager, eager_losses = _theta(model), {k: float(v) for k, v in tr._manual_losses().items()}
    tr, model, pde = _graph_trainer(name, dev)
    tr._sample = lambda n, xb=xb, tb=tb: (xb, tb)
    replay, losses = tr.make_graphed_step(NPTS, warmup=1)
    for _ in range(3):
        replay()
    torch.cuda.synchronize()
    assert torch.equal(_theta(model), eager), f"max |d theta| = {float((_theta(model) - eager).abs().max()):.3e}"
    assert {k: float(v) for k, v in losses.items()} == eager_losses
    assert not torch.equal(eager, _theta(_build(name, dev)[1]))  # the steps moved theta


def test_a_shift_rewritten_between_steps_changes_the_eager_step_and_the_replay(dev):
    """The half-saturation K of `monod2d`, the shift of its RECIP, lives in `pde.nl_values[0, 0]`: two steps with K = 2, then it is
    rewritten in place to 3 and two more steps follow.  The eager launch list follows the new value (its theta differs from four
    steps at 2), and the captured step, whose kernel reads the tensor at launch time, replays the same four steps bit for bit."""
    thetas = {}
    for key, second in (("same", 2.0), ("rewritten", 3.0)):
        tr, model, pde = _graph_trainer("monod2d", dev)
        xb, tb = _batches(pde, 1, seed=0)[0]
        tr._build_flat_state()
        assert float(pde.nl_values[0, 0]) == 2.0
        side = torch.cuda.Stream(device=dev)
        for step in range(4):
            if step == 2:
                pde.nl_values[0, 0] = second
            tr._manual_launches(xb, tb, side=side)
        torch.cuda.synchronize()
        thetas[key] = _theta(model)
    assert not torch.equal(thetas["same"], thetas["rewritten"])  # the eager step reads the parameters at every call
    tr, model, pde = _graph_trainer("monod2d", dev)
    tr._sample = lambda n, xb=xb, tb=tb: (xb, tb)
    replay, _ = tr.make_graphed_step(NPTS, warmup=1)
    replay()
    pde.nl_values[0, 0] = 3.0
    replay()
    replay()
    torch.cuda.synchronize()
    assert torch.equal(_theta(model), thetas["rewritten"]), f"max |d theta| = {float((_theta(model) - thetas['rewritten']).abs().max()):.3e}"


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_one_lbfgs_step_matches_the_eager_closure(name, dev):
    from pinnrl_amd.training import PDETrainer

    thetas = []
    for fast in (False, None):
        cfg, model, pde, spec = _build(name, dev, optimizer="lbfgs", lr=0.5)
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
    assert e <= 1e-4, f"{e:.2e}"
    assert not torch.equal(thetas[1], _theta(_build(name, dev)[1]))  # the step moved theta
