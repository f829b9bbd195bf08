"""GPU: HeatEquation's finite-difference smoothness term on the autograd-free step.

HeatEquation 1-D on [0, 2] x [0, 10], periodic boundary, the reference's loss weights {residual 15, boundary 20, initial 10,
smoothness 0.1}; fourier and feedforward 3x32 and one fourier 4x128 (the tile-major units of the default configuration);
1027 points of the uniform sampler (a permuted subset of its 33 x 33 jittered grid, whose outer rows are clamped onto the
domain ends: exact ties of the stencil).

The term is ill-conditioned in fp32 at the reference's eps = 1e-4 (tests/test_smoothness_model_cpu.py prints the figures:
S 3e-5, weight gradient 8e-3 against fp64, 3e-4 against itself with the batch permuted).  Correctness against the fp64 model
(tests/smoothness_model.py) is therefore asserted at eps = 2^-6 — a run-time scalar on the same code path — under the bars
of tests/test_inverse_step_gpu.py; at 1e-4 only what is well-defined there is asserted."""

import functools
import math
import os

import numpy as np
import pytest
import torch

from conftest import load_case, rel_l2

import smoothness_model as SM

pytestmark = pytest.mark.gpu

LO, HI, T_MAX = 0.0, 2.0, 10.0
N = 1027
WEIGHTS = {"residual": 15.0, "boundary": 20.0, "initial": 10.0, "smoothness": 0.1}
CASES = {"fourier_3x32": "burgers_fourier_3x32", "feedforward_3x32": "burgers_feedforward_3x32", "fourier_4x128": "heat_fourier_4x128"}
WIDE = 2.0**-6
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data_modes.npz")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _r32(v):
    return float(np.float32(v))


def _obs():
    a = np.load(GOLD)
    return {k: torch.from_numpy(a["obs_" + k]) for k in ("x", "t", "u")}


def _product(case, dev, eps=WIDE, mode="forward", smoothness=0.1, lr=1e-3, optimizer="adam", deterministic=False, **trainer_kw):
    import pinnrl_amd  # noqa: F401
    from pinnrl_amd import pdes as P
    from pinnrl_amd.config import Config, ModelConfig, TrainingConfig
    from pinnrl_amd.neural_networks import PINNModel
    from pinnrl_amd.training import PDETrainer

    spec, _, sd, _, _ = load_case(CASES[case])
    cfg = Config.__new__(Config)
    cfg.device = dev
    cfg.model = ModelConfig(input_dim=2, hidden_dim=spec.hidden_dim, output_dim=1, num_layers=spec.num_layers, activation=spec.activation,
                            architecture=spec.architecture)
    cfg.model.mapping_size, cfg.model.scale = spec.mapping_size, spec.scale
    model = PINNModel(cfg, device=dev)
    model.load_state_dict({k: v.to(dev) for k, v in sd.items()})
    if deterministic:
        model.set_deterministic(True)
    weights = dict(WEIGHTS, smoothness=smoothness)
    if mode != "forward":
        weights["data"] = 2.5
    tr = TrainingConfig(learning_rate=lr, gradient_clipping=1.0, weight_decay=5e-4, loss_weights=weights, mode=mode, optimizer=optimizer)
    tr.lbfgs.max_iter, tr.lbfgs.history_size = 3, 10
    cfg.training = tr
    cls = type("HeatEps", (P.HeatEquation,), {"_SMOOTHNESS_EPS": eps})  # the term's eps is a class attribute
    trainable = ["alpha"] if mode == "inverse" else []
    obs = _obs() if mode != "forward" else None
    pde = cls(P.PDEConfig(
        name="heat", domain=[(LO, HI)], time_domain=(0.0, T_MAX), parameters={"alpha": 0.01}, boundary_conditions={"periodic": {}},
        initial_condition={"type": "sine", "amplitude": 1.0, "frequency": 2.0}, exact_solution={}, dimension=1, device=dev, training=tr,
        trainable_parameters=trainable, parameter_initial_guesses={"alpha": 0.02} if trainable else {},
        observation_data={k: v.to(dev) for k, v in obs.items()} if obs else None))
    trainer = PDETrainer(model, pde, {}, cfg, device=dev, **trainer_kw)
    return cfg, model, pde, trainer, (spec, sd)


@functools.lru_cache(maxsize=None)
def _batches(count=3):
    """`count` pinned batches of N points (CPU tensors): the uniform sampler's 33 x 33 jittered grid, permuted, first N."""
    from pinnrl_amd import pdes as P

    pde = P.HeatEquation(P.PDEConfig(name="heat", domain=[(LO, HI)], time_domain=(0.0, T_MAX), parameters={"alpha": 0.01},
                                     boundary_conditions={"periodic": {}}, initial_condition={"type": "sine"}, exact_solution={},
                                     dimension=1, device=torch.device("cpu")))
    g = torch.Generator().manual_seed(7)
    torch.manual_seed(7)
    out = []
    for _ in range(count):
        x, t = pde.generate_collocation_points(33 * 33, strategy="uniform")
        keep = torch.randperm(x.shape[0], generator=g)[:N]
        x, t = x[keep].contiguous(), t[keep].contiguous()
        assert x.shape == (N, 1) and int((x == LO).sum()) >= 5 and int((x == HI).sum()) >= 5  # end points occur
        out.append((x, t))
    return tuple(out)


def _theta(model):
    return torch.cat([p.detach().flatten().cpu() for _, p in model.named_parameters()])


def _flat_grad_by_parameter(trainer, model):
    from pinnrl_amd import engine as E

    F = trainer._flat
    parts = [g for g in E.split_flat_grad(model.program(), F["grad"][: F["n"]]) if g is not None]
    return torch.cat([g.flatten().cpu() for g in parts])


def _autograd_evaluation(pde, model, x, t):
    """Losses and the gradient by parameter of the autograd step's loss evaluation (no optimiser step)."""
    for p in model.parameters():
        p.grad = None
    losses = pde.compute_loss(model, x, t)
    losses["total"].backward()
    grad = torch.cat([p.grad.flatten().cpu() for _, p in model.named_parameters() if p.requires_grad])
    return {k: float(v.detach()) for k, v in losses.items()}, grad


@functools.lru_cache(maxsize=None)
def _model_step(case, mode):
    """The fp64 model of one loss evaluation at eps = 2^-6 on batch 0 (computed once per case and mode).  The chain (fixed
    boundary / initial / observation points and their terms) is the product's own description of HeatEquation.compute_loss,
    built on the CPU."""
    cfg, model, pde, tr, (spec, sd) = _product(case, torch.device("cpu"), mode=mode)
    x, t = _batches()[0]
    ch = dict(pde._manual_chain(N))
    terms = [(lo, hi, st, pr, None if tg is None else tg.numpy(), w) for lo, hi, st, pr, tg, w in ch["terms"]]
    cx, ct = ch["x"], ch["t"]
    if mode != "forward":  # the data term l(model(obs) - u_obs), weight 2.5: one more range of points, one more term
        obs = _obs()
        lo = cx.shape[0]
        cx, ct = torch.cat([cx, obs["x"]]), torch.cat([ct, obs["t"]])
        terms.append((lo, lo + obs["x"].shape[0], 0, 0, obs["u"].reshape(-1).numpy(), 2.5))
    alpha = _r32(0.02 if mode == "inverse" else 0.01)
    sm = {"eps": WIDE, "weight": _r32(0.1), "lo": LO, "hi": HI}
    losses, grads, dalpha = SM.heat_step(spec, sd, x.numpy(), t.numpy(), alpha, 15.0, cx.numpy(), ct.numpy(), terms, ch["n_bc"], sm,
                                         has_data=mode != "forward")
    names = [k for k in sd if not k.endswith("fourier.B")]
    return losses, torch.cat([grads[k].flatten() for k in names]), dalpha


STEP_CASES = [("fourier_3x32", "forward"), ("fourier_3x32", "inverse"), ("fourier_3x32", "data_augmented"),
              ("feedforward_3x32", "forward"), ("feedforward_3x32", "inverse"), ("feedforward_3x32", "data_augmented"),
              ("fourier_4x128", "forward")]


@pytest.mark.parametrize("case,mode", STEP_CASES)
def test_one_step_against_the_fp64_model(case, mode, dev):
    """eps = 2^-6: {residual, boundary, initial, smoothness, total} within 2e-5 relative and the flat gradient within rel-l2
    2e-5 of the fp64 model (the bar of tests/test_inverse_step_gpu.py for one launch-list step; the fp32 CPU evaluation of the
    same step stands at 1e-6 / 1e-6)."""
    want, want_grad, want_dalpha = _model_step(case, mode)
    cfg, model, pde, tr, _ = _product(case, dev, mode=mode, fast_step=True)
    assert tr._manual_step_unsupported() is None, tr._manual_step_unsupported()
    tr._build_flat_state()
    x, t = (v.to(dev) for v in _batches()[0])
    losses = tr.train_step(x, t)
    torch.cuda.synchronize()
    keys = ("residual", "boundary", "initial", "smoothness", "total") + (("data",) if mode != "forward" else ())
    for k in keys:
        got = float(losses[k])
        print(f"{case}/{mode}/{k}: {got!r} vs {want[k]!r}: rel {abs(got - want[k]) / abs(want[k]):.2e}")
        assert abs(got - want[k]) <= 2e-5 * abs(want[k]), f"{k}: {got} vs {want[k]}"
    e = rel_l2(_flat_grad_by_parameter(tr, model), want_grad)
    print(f"{case}/{mode}: d total / d theta rel l2 {e:.2e}")
    assert e <= 2e-5, f"d total / d theta {e:.2e}"
    if mode == "inverse":  # the term does not depend on the coefficient: its gradient is the residual's
        got = float(tr._flat["coef_grad"][0])
        print(f"{case}/inverse/dalpha: {got!r} vs {want_dalpha!r}")
        assert abs(got - want_dalpha) <= 2e-5 * abs(want_dalpha)


@pytest.mark.parametrize("case", list(CASES))
def test_one_step_at_the_reference_eps_against_the_autograd_step(case, dev):
    """eps = 1e-4.  `smoothness` and `total` within 2e-6 relative of the autograd step's on the same batch: both read
    bit-identical u, only the order of the mean differs ((log2 N + 4) 2^-23 = 1.7e-6).  Gradient: max(2e-5, 4 x control),
    control = rel-l2 between the autograd step's gradients for the batch and for the same batch reversed — the parent's code
    path and its own reassociation noise (x 4: that noise varies from sample to sample).  Measured controls on an MI355X:
    see profiles/smoothness_step.md."""
    cfg, model, pde, tr, _ = _product(case, dev, eps=1e-4)
    x, t = (v.to(dev) for v in _batches()[0])
    eager, eager_grad = _autograd_evaluation(pde, model, x, t)
    _, reversed_grad = _autograd_evaluation(pde, model, x.flip(0).contiguous(), t.flip(0).contiguous())
    control = rel_l2(reversed_grad, eager_grad)
    assert tr._manual_step_unsupported() is None
    tr._build_flat_state()
    losses = tr.train_step(x, t)
    torch.cuda.synchronize()
    for k in ("smoothness", "total"):
        got = float(losses[k])
        print(f"{case}/{k}: {got!r} vs autograd {eager[k]!r}: rel {abs(got - eager[k]) / abs(eager[k]):.2e}")
        assert abs(got - eager[k]) <= 2e-6 * abs(eager[k]), f"{k}: {got} vs {eager[k]}"
    e = rel_l2(_flat_grad_by_parameter(tr, model), eager_grad)
    bar = max(2e-5, 4.0 * control)
    print(f"{case}: d total / d theta vs the autograd step rel l2 {e:.2e}; control (autograd, batch reversed) {control:.2e}; bar {bar:.2e}")
    assert e <= bar, f"d total / d theta {e:.2e} (control {control:.2e}, bar {bar:.2e})"


@pytest.mark.parametrize("case", ["fourier_3x32", "fourier_4x128"])
def test_three_adam_steps_match_the_autograd_step(case, dev):
    """eps = 2^-6, weight decay 5e-4, clipping 1.0, pinned batches, one theta_0: theta within rel-l2 1e-5, losses within 5e-5."""
    _, model_m, _, tr_m, _ = _product(case, dev, fast_step=True)
    _, model_a, _, tr_a, _ = _product(case, dev, fast_step=False)
    assert tr_m._manual_step_unsupported() is None
    tr_m._build_flat_state()
    assert float(tr_m._flat["wd"]) == 5e-4
    for step, (xb, tb) in enumerate(_batches(), start=1):
        x, t = xb.to(dev), tb.to(dev)
        got = tr_m.train_step(x, t)
        want = tr_a.train_step(x, t)
        torch.cuda.synchronize()
        for k in ("residual", "boundary", "initial", "smoothness", "total"):
            g, w = float(got[k]), float(want[k].detach())
            assert abs(g - w) <= 5e-5 * abs(w), f"step {step} {k}: {g} vs {w}"
        e = rel_l2(_theta(model_m), _theta(model_a))
        print(f"{case} step {step}: theta rel l2 {e:.2e}; total {float(got['total'])!r} vs {float(want['total'].detach())!r}")
        assert e <= 1e-5, f"theta after {step} steps: {e:.2e}"
    assert getattr(tr_a, "_flat", None) is None


def test_graph_replay_equals_the_eager_launch_list(dev):
    out = []
    xb, tb = (v.to(dev) for v in _batches()[0])
    for graphed in (False, True):
        _, model, pde, tr, _ = _product("fourier_3x32", dev, lr=2e-3)
        tr._sample = lambda n, xb=xb, tb=tb: (xb, tb)
        if graphed:
            replay, losses = tr.make_graphed_step(N, warmup=1)
            assert "smoothness" in losses and losses["smoothness"].data_ptr() == tr._flat["smooth_loss"].data_ptr()  # a static view
            tr._flat["smooth_loss"].fill_(-1.0)
            for _ in range(3):
                replay()
            torch.cuda.synchronize()
            assert float(losses["smoothness"]) > 0.0  # the replay refreshed it
            assert set(losses) >= {"residual", "boundary", "initial", "smoothness", "total"} and math.isfinite(float(losses["total"]))
            last = {k: float(v) for k, v in losses.items()}
        else:
            tr._build_flat_state()
            for _ in range(4):
                eager = tr.train_step(xb, tb)
        out.append(_theta(model))
    e = rel_l2(out[1], out[0])
    print(f"theta rel l2 {e:.2e}; smoothness {last['smoothness']!r} vs {float(eager['smoothness'])!r}")
    assert e <= 1e-5
    assert abs(last["smoothness"] - float(eager["smoothness"])) <= 5e-5 * abs(float(eager["smoothness"]))


def test_lbfgs_takes_the_launch_list_closure(dev):
    """optimizer = "lbfgs": the first closure loss of one flat step() equals `total` of the Adam-path evaluation at theta_0 bit
    for bit (fixed-order reductions: the deterministic engine flag)."""
    xb, tb = (v.to(dev) for v in _batches()[0])
    _, model_a, pde_a, tr_a, _ = _product("fourier_3x32", dev, deterministic=True)
    tr_a._build_flat_state()
    F = tr_a._flat
    tr_a._loss_grad_launches(xb, tb, F, model_a.program(), pde_a._pde_desc(), tr_a._chain(N))
    torch.cuda.synchronize()
    total0, smooth0 = float(F["summary"][3]), float(F["smooth_loss"][0])
    assert smooth0 > 0.0 and total0 > 0.1 * smooth0

    _, model_l, pde_l, tr_l, _ = _product("fourier_3x32", dev, optimizer="lbfgs", lr=0.5, deterministic=True)
    assert tr_l._is_lbfgs and tr_l._manual_step_unsupported() is None, tr_l._manual_step_unsupported()
    tr_l._build_flat_state()
    theta0 = _theta(model_l)
    backend = tr_l._lbfgs_flat_state()["driver"].backend
    seen = []
    evaluate = backend.evaluate
    backend.evaluate = lambda t: seen.append(evaluate(t)) or seen[-1]
    losses = tr_l.train_step(xb, tb)
    print(f"first closure loss {seen[0]['loss']!r} vs Adam-path total {total0!r}; {len(seen)} evaluations")
    assert seen[0]["loss"] == total0
    assert len(seen) >= 2 and math.isfinite(float(losses["total"])) and "smoothness" in losses
    assert not torch.equal(_theta(model_l), theta0)


def test_train_takes_the_launch_list_and_smoothness_zero_adds_nothing(dev):
    cfg, model, pde, tr, _ = _product("fourier_3x32", dev, eps=1e-4, validation_frequency=5)
    torch.manual_seed(0)
    hist = tr.train(num_epochs=2, batch_size=1024, num_points=2048)
    F = getattr(tr, "_flat", None)
    assert F is not None and "smooth_loss" in F and all("smooth" in ch for ch in F["chains"].values())
    for k in ("train_loss", "residual_loss", "boundary_loss", "initial_loss", "learning_rate"):
        assert len(hist[k]) == 2 and all(math.isfinite(v) for v in hist[k]), k

    cfg, model, pde, tr, _ = _product("fourier_3x32", dev, eps=1e-4, smoothness=0.0, validation_frequency=5)
    torch.manual_seed(0)
    tr.train(num_epochs=1, batch_size=1024, num_points=1024)
    F = tr._flat
    assert F is not None and "smooth_loss" not in F and all("smooth" not in ch for ch in F["chains"].values())
    assert "smoothness" not in tr._manual_losses()
