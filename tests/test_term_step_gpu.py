"""Burgers as a `TermPDE` on the autograd-free step (fourier 3x32, 100 collocation points per batch), with the tolerances
tests/test_api_gpu.py applies to the same comparisons:

  theta after 1 / 3 / 10 launch-list Adam steps vs the autograd step of the same TermPDE        rel-L2 <= 1e-5
  theta after 1 / 3 / 10 launch-list Adam steps vs the launch list of BurgersEquation             rel-L2 <= 1e-5
  loss terms vs BurgersEquation                                                                  5e-5
  one L-BFGS step() vs the autograd step of the same TermPDE                                      1e-4
  one RBW step vs the autograd step of the same TermPDE                                           rel-L2 <= 1e-5
  a graph-captured step vs the eager launch list                                                  1e-5

and, after nu is overwritten in place on the device, a replay equals an eager step of a fresh trainer built with that
nu: the coefficients are read at launch time."""

import math

import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

TAG = "burgers_fourier_3x32"
NPTS = 100
BURGERS = [(1.0, ("u_t",)), (1.0, ("u", "u_x")), ((-1.0, "nu"), ("u_xx",))]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _build(kind, dev, nu=None):
    """cfg, model (the fixture's theta_0), PDE (`term`: Burgers as a TermPDE, `compiled`: BurgersEquation), PdeSpec."""
    import test_api_gpu as api
    from pinnrl_amd import pdes as P

    cfg, model, pde, (spec, ps, sd, a, m) = api.build(TAG, dev)
    if nu is not None:
        pde.config.parameters["nu"] = float(nu)
    if kind == "term":
        c = pde.config
        pde = P.TermPDE(P.PDEConfig(name="burgers as terms", domain=list(c.domain), time_domain=tuple(c.time_domain),
                                    parameters=dict(c.parameters), boundary_conditions=dict(c.boundary_conditions),
                                    initial_condition=dict(c.initial_condition), exact_solution={}, dimension=1, device=dev),
                        BURGERS)
    return cfg, model, pde, ps


def _theta(model):
    return torch.cat([p.detach().flatten().cpu() for _, p in model.named_parameters()])


def _batches(ps, n, seed=5):
    import oracle as O

    torch.manual_seed(seed)
    return [O.sample_uniform(ps, NPTS) for _ in range(n)]


def test_adam_launch_list_matches_autograd_and_the_compiled_kind(dev):
    from pinnrl_amd.training import PDETrainer

    runs = {}
    for key, kind, fast in (("term", "term", None), ("autograd", "term", False), ("compiled", "compiled", None)):
        cfg, model, pde, ps = _build(kind, dev)
        tr = PDETrainer(model, pde, {}, cfg, device=dev, fast_step=fast)
        if fast is None:
            assert tr._manual_step_unsupported() is None, tr._manual_step_unsupported()
            tr._build_flat_state()
        thetas, losses = {}, []
        for step, (xb, tb) in enumerate(_batches(ps, 10), start=1):
            out = tr.train_step(xb.to(dev), tb.to(dev))
            losses.append({k: float(out[k].detach()) for k in ("residual", "boundary", "initial", "total")})
            if step in (1, 3, 10):
                thetas[step] = _theta(model)
        assert (getattr(tr, "_flat", None) is not None) == (fast is None)
        runs[key] = (thetas, losses)
    for step in (1, 3, 10):
        e_a = rel_l2(runs["term"][0][step], runs["autograd"][0][step], label=f"theta vs autograd, step {step}", tol=1e-5)
        e_c = rel_l2(runs["term"][0][step], runs["compiled"][0][step], label=f"theta vs BurgersEquation, step {step}", tol=1e-5)
        print(f"step {step}: theta vs autograd {e_a:.2e}, vs BurgersEquation {e_c:.2e}")
        assert e_a <= 1e-5 and e_c <= 1e-5, (step, e_a, e_c)
    for step, (got, want) in enumerate(zip(runs["term"][1], runs["compiled"][1]), start=1):
        for k in got:
            assert abs(got[k] - want[k]) <= 5e-5 * abs(want[k]), (step, k, got[k], want[k])


def test_one_lbfgs_step_matches_the_autograd_step(dev):
    from pinnrl_amd.config import TrainingConfig
    from pinnrl_amd.training import PDETrainer

    thetas = []
    for fast in (False, None):
        cfg, model, pde, ps = _build("term", dev)
        cfg.training = TrainingConfig(learning_rate=0.5, gradient_clipping=0.0, optimizer="lbfgs")
        cfg.training.lbfgs.max_iter, cfg.training.lbfgs.history_size = 4, 10
        tr = PDETrainer(model, pde, {}, cfg, device=dev, fast_step=fast)
        assert tr._is_lbfgs
        if fast is None:
            assert tr._manual_step_unsupported() is None, tr._manual_step_unsupported()
            tr._build_flat_state()
        xb, tb = _batches(ps, 1, seed=9)[0]
        out = tr.train_step(xb.to(dev), tb.to(dev))
        assert math.isfinite(float(out["total"]))
        thetas.append(_theta(model))
    e = rel_l2(thetas[1], thetas[0], label="theta after one L-BFGS step", tol=1e-4)
    assert e <= 1e-4, f"{e:.2e}"
    assert not torch.equal(thetas[1], _theta(_build("term", dev)[1]))  # the step moved theta


def test_one_rbw_step_matches_the_autograd_step(dev):
    from pinnrl_amd.config import AdaptiveWeightsConfig
    from pinnrl_amd.training import PDETrainer

    thetas = []
    for fast in (False, None):
        cfg, model, pde, ps = _build("term", dev)
        cfg.training.gradient_clipping, cfg.training.learning_rate = 1.0, 1e-3
        cfg.training.adaptive_weights = AdaptiveWeightsConfig(enabled=True, strategy="rbw", alpha=0.9, eps=1e-5,
                                                              initial_weights=[0.5, 0.3, 0.2])
        tr = PDETrainer(model, pde, {}, cfg, device=dev, fast_step=fast)
        if fast is None:
            assert tr._manual_step_unsupported() is None, tr._manual_step_unsupported()
            tr._build_flat_state()
        xb, tb = _batches(ps, 1)[0]
        tr.train_step(xb.to(dev), tb.to(dev))
        thetas.append(_theta(model))
    e = rel_l2(thetas[1], thetas[0], label="theta after one RBW step", tol=1e-5)
    assert e <= 1e-5, f"{e:.2e}"


def test_graph_captured_step_and_a_coefficient_written_on_the_device(dev):
    from pinnrl_amd.training import PDETrainer

    nu2 = 0.05
    # eager launch list: four steps on one pinned batch
    cfg, model, pde, ps = _build("term", dev)
    xb, tb = (v.to(dev) for v in _batches(ps, 1, seed=0)[0])
    tr = PDETrainer(model, pde, {}, cfg, device=dev)
    tr._build_flat_state()
    for _ in range(4):
        tr.train_step(xb, tb)
    eager = _theta(model)
    # captured: one warm-up step, three replays
    cfg, model, pde, ps = _build("term", dev)
    tr = PDETrainer(model, pde, {}, cfg, device=dev)
    tr._sample = lambda n, xb=xb, tb=tb: (xb, tb)
    F = tr._build_flat_state()
    theta0 = F["theta"].clone()
    replay, losses = tr.make_graphed_step(NPTS, warmup=1)
    for _ in range(3):
        replay()
    torch.cuda.synchronize()
    assert math.isfinite(float(losses["total"])) and set(losses) >= {"residual", "boundary", "initial", "total"}
    e = rel_l2(_theta(model), eager, label="graphed vs eager launch list", tol=1e-5)
    assert e <= 1e-5, f"{e:.2e}"
    # back to theta_0 with fresh Adam state, nu overwritten in place on the device: the replay follows it
    with torch.no_grad():
        F["theta"].copy_(theta0)
        for k in ("m", "v", "step"):
            F[k].zero_()
        pde.coef_values[2:3].fill_(-nu2)
    replay()
    torch.cuda.synchronize()
    got, got_res = _theta(model), float(losses["residual"])
    cfg, model, pde2, ps = _build("term", dev, nu=nu2)
    assert float(pde2.coef_values[2]) == pytest.approx(-nu2)
    tr2 = PDETrainer(model, pde2, {}, cfg, device=dev)
    tr2._build_flat_state()
    out = tr2.train_step(xb, tb)
    e = rel_l2(got, _theta(model), label="replay after nu was written vs a fresh trainer", tol=1e-5)
    assert e <= 1e-5, f"{e:.2e}"
    assert abs(got_res - float(out["residual"])) <= 5e-5 * abs(float(out["residual"]))
    # and the step with the old nu is a different one
    cfg, model, pde1, ps = _build("term", dev)
    tr1 = PDETrainer(model, pde1, {}, cfg, device=dev)
    tr1._build_flat_state()
    out1 = tr1.train_step(xb, tb)
    assert abs(float(out1["residual"]) - got_res) > 1e-3 * abs(got_res)


def test_device_spelled_without_an_index(dev):
    """`torch.device("cuda")` (what `config.default_device()` returns): the tensors made on it report cuda:0, and the
    coefficient tensor and the descriptor must still be built once — nothing is rebuilt inside a step, an in-place write
    reaches the captured graph, and the step equals the one of a PDE built on cuda:0."""
    import test_api_gpu as api
    from pinnrl_amd import pdes as P
    from pinnrl_amd.training import PDETrainer

    plain = torch.device("cuda")
    nu2 = 0.05

    def build(device, nu=None):
        cfg, model, pde, (spec, ps, sd, a, m) = api.build(TAG, device)
        c = pde.config
        params = dict(c.parameters)
        if nu is not None:
            params["nu"] = nu
        term = P.TermPDE(P.PDEConfig(name="burgers as terms", domain=list(c.domain), time_domain=tuple(c.time_domain),
                                     parameters=params, boundary_conditions=dict(c.boundary_conditions),
                                     initial_condition=dict(c.initial_condition), exact_solution={}, dimension=1, device=device),
                         BURGERS)
        return cfg, model, term, ps

    cfg, model, pde, ps = build(plain)
    cv, td = pde.coef_values, pde._pde_desc()
    assert cv.is_cuda and pde.coef_values is cv and pde._pde_desc() is td and td.coef_values is cv
    xb, tb = (v.to(dev) for v in _batches(ps, 1, seed=0)[0])
    tr = PDETrainer(model, pde, {}, cfg, device=plain)
    tr._sample = lambda n, xb=xb, tb=tb: (xb, tb)
    assert tr._manual_step_unsupported() is None
    F = tr._build_flat_state()
    theta0 = F["theta"].clone()
    tr.train_step(xb, tb)
    assert pde.coef_values is cv and pde._pde_desc() is td  # a step rebuilt neither
    replay, losses = tr.make_graphed_step(NPTS, warmup=1)
    replay()
    torch.cuda.synchronize()
    assert pde.coef_values is cv and pde._pde_desc() is td
    with torch.no_grad():
        F["theta"].copy_(theta0)
        for k in ("m", "v", "step"):
            F[k].zero_()
        pde.coef_values[2:3].fill_(-nu2)
    assert float(cv[2]) == pytest.approx(-nu2)  # the write went into the tensor the graph reads
    replay()
    torch.cuda.synchronize()
    got, got_res = _theta(model), float(losses["residual"])
    cfg, model, pde2, ps = build(dev, nu=nu2)
    tr2 = PDETrainer(model, pde2, {}, cfg, device=dev)
    tr2._build_flat_state()
    out = tr2.train_step(xb, tb)
    e = rel_l2(got, _theta(model), label="replay on torch.device('cuda') after nu was written vs a fresh trainer", tol=1e-5)
    assert e <= 1e-5, f"{e:.2e}"
    assert abs(got_res - float(out["residual"])) <= 5e-5 * abs(float(out["residual"]))
