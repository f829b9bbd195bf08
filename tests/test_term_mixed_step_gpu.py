"""`TermPDEMixed` end to end on the GPU, width 32, 64 collocation points — three problems:

  aniso2d    u_t - a u_xx - 2 b u_xy - c u_yy            (feedforward; one direction launch on the set (0, 2))
  biheat2d   u_t + kappa (u_xxxx + 2 u_xxyy + u_yyyy)    (fourier; both direction launches on the set (0, 4))
  biheat3d   u_t + kappa Lap^2 u in three dimensions      (feedforward; nine launches)

Part one: residual, loss terms and d total / d theta against nested fp64 autograd of the written-out formula through
`oracle.network_forward` on a CPU copy of the model.  A mixed derivative is a difference of streams that each carry the stream
bar (2e-5, tests/test_axis_jets_gpu.py), so the residual's tolerance is that bar times the amplification of the polarisation
formula, computed from the fp64 reference in the test:
    A_2 = rms((|P_2| + |u_aa| + |u_bb|) / 2) / rms(u_ab),   A_4 = rms((|P_4| + |Q_4| + 2 |u_aaaa| + 2 |u_bbbb|) / 12) / rms(u_aabb)
(the largest over the pairs the problem names).  Loss terms and gradient keep the 1e-5 of tests/test_term_nd_step_gpu.py.
Part two, at that file's bars: theta after 3 Adam steps of the launch list against the autograd step (1e-5), the captured step
against the eager launch list (bit for bit), one L-BFGS step (1e-4), and a residual-based resampling call that runs."""

import math

import pytest
import torch

from conftest import rel_err, rel_l2

pytestmark = pytest.mark.gpu

TOL = 1e-5
STREAM_BAR = 2e-5
NPTS = 64
PI = math.pi
PAIRS = ((0, 1), (0, 2), (1, 2))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _sines(x):
    return torch.prod(torch.sin(PI * x), dim=1)


def _bilaplacian(dim):
    names = ["u_xxxx", "u_yyyy", "u_zzzz"][:dim]
    mixed = ["u_xxyy", "u_xxzz", "u_yyzz"] if dim == 3 else ["u_xxyy"]
    return [(1.0, ("u_t",))] + [((1.0, "kappa"), (n,)) for n in names] + [((2.0, "kappa"), (n,)) for n in mixed]


PROBLEMS = {
    "aniso2d": dict(dim=2, arch="feedforward", params={"a": 0.05, "b": 0.02, "c": 0.08}, order=2,
                    terms=[(1.0, ("u_t",)), ((-1.0, "a"), ("u_xx",)), ((-2.0, "b"), ("u_xy",)), ((-1.0, "c"), ("u_yy",))]),
    "biheat2d": dict(dim=2, arch="fourier", params={"kappa": 0.02}, order=4, terms=_bilaplacian(2)),
    "biheat3d": dict(dim=3, arch="feedforward", params={"kappa": 0.02}, order=4, terms=_bilaplacian(3)),
}
AXES = {"x": 0, "y": 1, "z": 2}


def _spec(name):
    import oracle as O

    p = PROBLEMS[name]
    if p["arch"] == "fourier":
        return O.ArchSpec("fourier", input_dim=p["dim"] + 1, hidden_dim=32, num_layers=3, activation="tanh", mapping_size=8, scale=1.0)
    return O.ArchSpec("feedforward", input_dim=p["dim"] + 1, hidden_dim=32, num_layers=2, activation="tanh")


def _build(name, dev, optimizer="adam", lr=1e-3, sampler="uniform", seed=3):
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
                     boundary_conditions={"dirichlet": {"type": "fixed", "value": 0.0}}, initial_condition={}, exact_solution={},
                     dimension=p["dim"], device=dev, training=cfg.training)
    pde = P.TermPDEMixed(pc, p["terms"], _sines, boundary_points_per_axis=4, initial_points_per_axis=5)
    return cfg, model, pde, spec, sd


def _theta(model):
    return torch.cat([p.detach().flatten().cpu() for _, p in model.named_parameters()])


def _points(name, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, PROBLEMS[name]["dim"], generator=g), torch.rand(n, 1, generator=g) * 0.5


_fp64 = {}


def _oracle(name, pde):
    """fp64 residual, loss terms, total, d total / d theta and the amplification A by nested autograd through the oracle's
    network, on 64 seeded points and the PDE's own fixed boundary / initial points; computed once per problem."""
    import oracle as O

    if name in _fp64:
        return _fp64[name]
    p, spec = PROBLEMS[name], _spec(name)
    dim, k = p["dim"], p["order"]
    sd = O.init_state_dict(spec, seed=3)
    params = {n: v.double().requires_grad_(n != "model.fourier.B") for n, v in sd.items()}
    x32, t32 = _points(name, NPTS, 17)
    x, t = x32.double().requires_grad_(True), t32.double().requires_grad_(True)
    u = O.network_forward(spec, params, torch.cat([x, t], 1))
    d = lambda y, w: torch.autograd.grad(y, w, torch.ones_like(y), create_graph=True)[0]  # noqa: E731
    cache = {}

    def deriv(axes):  # d^n u / dx_axes[0] dx_axes[1] .., nested in the order written
        if axes not in cache:
            cache[axes] = u if not axes else d(deriv(axes[:-1]), x)[:, axes[-1] : axes[-1] + 1]
        return cache[axes]

    def along(direction, n):  # (sum_c d_c d/dx_c)^n u
        y = u
        for _ in range(n):
            y = (d(y, x) * torch.tensor(direction, dtype=torch.float64)).sum(1, keepdim=True)
        return y

    r = d(u, t)
    for coef, factors in p["terms"][1:]:
        c = coef[0] * p["params"][coef[1]]
        r = r + c * deriv(tuple(AXES[ch] for ch in factors[0][2:]))
    amp = 0.0
    rms = lambda v: float(v.norm()) / NPTS ** 0.5  # noqa: E731
    for a, b in PAIRS[: (1 if dim == 2 else 3)]:
        ea, eb = [float(c == a) for c in range(dim)], [float(c == b) for c in range(dim)]
        plus, minus = [i + j for i, j in zip(ea, eb)], [i - j for i, j in zip(ea, eb)]
        A, B, Pk = along(ea, k).detach(), along(eb, k).detach(), along(plus, k).detach()
        if k == 2:
            amp = max(amp, rms((Pk.abs() + A.abs() + B.abs()) / 2) / rms(deriv((a, b)).detach()))
        else:
            Qk = along(minus, k).detach()
            amp = max(amp, rms((Pk.abs() + Qk.abs() + 2 * A.abs() + 2 * B.abs()) / 12) / rms(deriv((a, a, b, b)).detach()))
    res = torch.mean(r**2)
    pts = {n: (v.cpu() if isinstance(v, torch.Tensor) else v) for n, v in pde._nd_points().items()}
    ub = O.network_forward(spec, params, torch.cat([pts["x"], pts["t"]], 1).double())[:, 0]
    nbc = pts["n_bc"]
    bnd, ini = torch.mean(ub[:nbc] ** 2), torch.mean((ub[nbc:] - pts["u0"].double()) ** 2)
    lw = pde._loss_weights()
    total = lw.get("pde", lw.get("residual", 1.0)) * res + lw.get("boundary", 10.0) * bnd + lw.get("initial", 10.0) * ini
    names = [n for n, v in params.items() if v.requires_grad]
    g = torch.autograd.grad(total, [params[n] for n in names])
    _fp64[name] = {"x": x32, "t": t32, "r": r.detach(), "residual": float(res.detach()), "boundary": float(bnd.detach()),
                   "initial": float(ini.detach()), "total": float(total.detach()), "names": names, "grad": torch.cat([v.flatten() for v in g]), "amp": amp}
    return _fp64[name]


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_residual_losses_and_gradient_match_fp64_autograd(name, dev):
    from pinnrl_amd import engine as E

    cfg, model, pde, spec, sd = _build(name, dev)
    o = _oracle(name, pde)
    tol_r = STREAM_BAR * o["amp"]
    x, t = o["x"].to(dev), o["t"].to(dev)
    r = pde.compute_residual(model, x, t)
    assert r.shape == (NPTS, 1) and r.requires_grad
    e_r = rel_l2(r.detach().cpu(), o["r"], label=f"{name}: residual", tol=tol_r)
    losses = pde.compute_loss(model, x, t)
    errs = {k: rel_err(float(losses[k].detach()), o[k], label=f"{name}: {k} loss", tol=TOL) for k in ("residual", "boundary", "initial", "total")}
    model.zero_grad()
    losses["total"].backward()
    got = torch.cat([dict(model.named_parameters())[k].grad.flatten().cpu() for k in o["names"]])
    e_g = rel_l2(got, o["grad"], label=f"{name}: d total / d theta", tol=TOL)
    print(f"{name}: amplification {o['amp']:.2f}, residual {e_r:.2e} (tolerance {tol_r:.2e}), losses "
          f"{', '.join(f'{k} {v:.2e}' for k, v in errs.items())}, gradient {e_g:.2e}")
    assert 1.0 <= o["amp"] < 50.0
    assert e_r <= tol_r, f"residual: {e_r:.2e} > {tol_r:.2e}"
    assert all(v <= TOL for v in errs.values()), errs
    assert e_g <= TOL, f"gradient: {e_g:.2e}"
    # the raw chain: residual_loss_grad accumulates the gradients of every launch into one flat buffer
    prog, td = model.program(), pde._pde_desc()
    assert isinstance(td, E.MixedTermDesc) and len(td.launches()) == {"aniso2d": 3, "biheat2d": 4, "biheat3d": 9}[name]
    flat = E.new_flat_grad(prog, dev)
    r2, s2 = E.residual_loss_grad(prog, td, x, t, 1.0 / NPTS, flat, want_residual=True)
    assert torch.equal(r2, r.detach()) and rel_err(float(s2) / NPTS, o["residual"]) <= TOL
    pr = pde._residual_sampling_probabilities(model, x, t)
    want = (o["r"].abs().flatten() + 1e-8) / (o["r"].abs().sum() + NPTS * 1e-8)
    assert rel_l2(pr.cpu(), want) <= tol_r


def _batches(pde, n, seed=5):
    torch.manual_seed(seed)
    return [pde._sample_uniform(NPTS) for _ in range(n)]


@pytest.mark.parametrize("name", ["aniso2d", "biheat2d"])
def test_adam_launch_list_matches_the_autograd_step(name, dev):
    from pinnrl_amd.training import PDETrainer

    runs, batches = {}, None
    for key, fast in (("list", None), ("autograd", False)):
        cfg, model, pde, spec, sd = _build(name, dev)
        batches = batches or _batches(pde, 3)
        tr = PDETrainer(model, pde, {}, cfg, device=dev, fast_step=fast)
        if fast is None:
            assert tr._manual_step_unsupported() is None, tr._manual_step_unsupported()
            tr._build_flat_state()
        losses = []
        for xb, tb in batches:
            out = tr.train_step(xb, tb)
            losses.append({k: float(out[k].detach()) for k in ("residual", "boundary", "initial", "total")})
        assert (getattr(tr, "_flat", None) is not None) == (fast is None)
        runs[key] = (_theta(model), losses)
    e = rel_l2(runs["list"][0], runs["autograd"][0], label=f"{name}: theta vs autograd, step 3", tol=TOL)
    print(f"{name} step 3: theta vs autograd {e:.2e}")
    assert e <= TOL, e
    for step, (got, want) in enumerate(zip(runs["list"][1], runs["autograd"][1]), start=1):
        for k in got:
            assert abs(got[k] - want[k]) <= 5e-5 * abs(want[k]), (step, k, got[k], want[k])


@pytest.mark.parametrize("name", ["aniso2d", "biheat2d"])
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


def test_one_lbfgs_step_matches_the_eager_closure(dev):
    from pinnrl_amd.training import PDETrainer

    thetas = []
    for fast in (False, None):
        cfg, model, pde, spec, sd = _build("aniso2d", dev, optimizer="lbfgs", lr=0.5)
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
    e = rel_l2(thetas[1], thetas[0], label="aniso2d: theta after one L-BFGS step", tol=1e-4)
    assert e <= 1e-4, f"{e:.2e}"
    assert not torch.equal(thetas[1], _theta(_build("aniso2d", dev)[1]))  # the step moved theta


def test_residual_based_sampler_runs_on_the_launch_list(dev):
    from pinnrl_amd.training import PDETrainer

    cfg, model, pde, spec, sd = _build("biheat2d", dev, sampler="residual_based")
    tr = PDETrainer(model, pde, {}, cfg, device=dev)
    assert tr._manual_step_unsupported() is None
    tr._build_flat_state()
    torch.manual_seed(1)
    x, t = tr._sample(NPTS)
    assert x.shape == (NPTS, 2) and t.shape == (NPTS, 1) and x.is_cuda
    assert float(x.min()) >= 0.0 and float(x.max()) <= 1.0 and float(t.min()) >= 0.0 and float(t.max()) <= 0.5
    out = tr.train_step(x, t)
    assert all(math.isfinite(float(out[k])) for k in ("residual", "boundary", "initial", "total"))
