"""GPU: the autograd-free launch list and the captured graph for `mode in ("inverse", "data_augmented")`.

Set-up as `tests/test_data_modes.py::test_product_data_modes_on_the_gpu` (Burgers / fourier 3x32, observation data, loss
weights {1, 10, 10, 2.5}); `tests/golden/data_modes.npz` holds the REFERENCE's numbers for one evaluation.  The step
itself is checked against the CPU oracle with `torch.optim.Adam` over [theta, nu] and `clip_grad_norm_` over theta only
(pinnrl/training/trainer.py:690-694)."""

import math
import os

import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data_modes.npz")
LW = {"residual": 1.0, "boundary": 10.0, "initial": 10.0, "data": 2.5}
KEYS = ("residual", "boundary", "initial", "data", "total")
NU_TRUE = 0.01 / math.pi


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _load():
    a = dict(np.load(GOLD))
    sd = {k[3:]: torch.from_numpy(v) for k, v in a.items() if k.startswith("sd/")}
    obs = {k: torch.from_numpy(a["obs_" + k]) for k in ("x", "t", "u")}
    return a, sd, obs


def _product(mode, dev, a, sd, obs, trainable=None, lr=1e-3, pde_cls=None, parameters=None, guesses=None, **trainer_kw):
    import pinnrl_amd  # noqa: F401
    from pinnrl_amd import pdes as P
    from pinnrl_amd.config import Config, ModelConfig, TrainingConfig
    from pinnrl_amd.neural_networks import PINNModel
    from pinnrl_amd.training import PDETrainer

    inverse = mode == "inverse"
    if trainable is None:
        trainable = ["nu"] if inverse else []
    cfg = Config.__new__(Config)
    cfg.device = dev
    cfg.model = ModelConfig(input_dim=2, hidden_dim=32, output_dim=1, num_layers=3, activation="tanh", architecture="fourier")
    cfg.model.mapping_size, cfg.model.scale = 16, 4.0
    model = PINNModel(cfg, device=dev)
    model.load_state_dict({k: v.to(dev) for k, v in sd.items()})
    tr = TrainingConfig(learning_rate=lr, gradient_clipping=1.0, loss_weights=dict(LW), mode=mode)
    cfg.training = tr
    if guesses is None:
        guesses = {"nu": float(a["nu_guess"])} if trainable == ["nu"] else {}
    pde = (pde_cls or P.BurgersEquation)(P.PDEConfig(
        name="burgers", domain=[(-1.0, 1.0)], time_domain=(0.0, 1.0), parameters=parameters or {"nu": NU_TRUE},
        boundary_conditions={"dirichlet": {"type": "fixed", "value": 0.0}},
        initial_condition={"type": "sine", "amplitude": -1.0, "frequency": 1.0}, exact_solution={}, dimension=1, device=dev,
        training=tr, trainable_parameters=list(trainable), parameter_initial_guesses=guesses,
        observation_data={k: v.to(dev) for k, v in obs.items()} if obs else None))
    trainer = PDETrainer(model, pde, {}, cfg, device=dev, **trainer_kw)
    return cfg, model, pde, trainer


def _theta(model):
    return torch.cat([p.detach().flatten().cpu() for _, p in model.named_parameters()])


def _flat_grad_by_parameter(trainer, model):
    from pinnrl_amd import engine as E

    F = trainer._flat
    prog = model.program()
    parts = [g for g in E.split_flat_grad(prog, F["grad"][: F["n"]]) if g is not None]
    return torch.cat([g.flatten().cpu() for g in parts])


@pytest.mark.parametrize("mode", ["inverse", "data_augmented"])
def test_one_launch_list_step_against_the_reference_fixture(mode, dev):
    a, sd, obs = _load()
    cfg, model, pde, tr = _product(mode, dev, a, sd, obs, fast_step=True)
    assert tr._manual_step_unsupported() is None, tr._manual_step_unsupported()
    tr._build_flat_state()
    x, t = torch.from_numpy(a["x"]).to(dev), torch.from_numpy(a["t"]).to(dev)
    losses = tr.train_step(x, t)
    torch.cuda.synchronize()
    for k in KEYS:
        want = float(a[f"{mode}/{k}"])
        got = float(losses[k])
        print(f"{mode}/{k}: {got!r} vs {want!r}")
        assert abs(got - want) <= 2e-5 * abs(want) + 1e-9, f"{mode}/{k}: {got} vs {want}"
    e = rel_l2(_flat_grad_by_parameter(tr, model), a[f"{mode}/grad"])
    print(f"{mode}: d total / d theta rel l2 {e:.2e}")
    assert e <= 2e-5, f"{mode}: d total / d theta {e:.2e}"
    if mode == "inverse":
        F = tr._flat
        lo, hi = F["coef_slice"]
        assert (lo, hi) == (0, 1)
        got, want = float(F["coef_grad"][0]), float(a["inverse/dnu"])
        print(f"inverse/dnu: {got!r} vs {want!r}")
        assert abs(got - want) <= 2e-5 * abs(want), f"d total / d nu: {got} vs {want}"
        assert float(pde.get_parameter("nu").detach()) != float(a["nu_guess"])  # the step moved the coefficient
    else:
        assert "coef" not in tr._flat


def _cpu_reference_run(a, sd, obs, batches, nu0, lr, checkpoints):
    """theta and nu after the checkpoint steps: fp32 CPU oracle, Adam over [theta, nu], clip_grad_norm_ over theta only."""
    import oracle as O

    spec = O.ArchSpec("fourier", hidden_dim=32, num_layers=3, mapping_size=16, scale=4.0)
    params = {k: v.clone().requires_grad_(k != "model.fourier.B") for k, v in sd.items()}
    names = [k for k in params if params[k].requires_grad]
    nu = torch.tensor(float(nu0), requires_grad=True)
    pde = O.PdeSpec(name="burgers", parameters={"nu": nu}, boundary_conditions={"dirichlet": {"type": "fixed", "value": 0.0}},
                    initial_condition={"type": "sine", "amplitude": -1.0, "frequency": 1.0}, loss_weights=dict(LW))
    opt = torch.optim.Adam([params[k] for k in names] + [nu], lr=lr, weight_decay=0.0)
    out = {}
    for step, (xb, tb) in enumerate(batches, start=1):
        opt.zero_grad()
        want = O.compute_loss_terms(pde, lambda z: O.network_forward(spec, params, z), xb, tb, observations=obs, mode="inverse")
        want["total"].backward()
        torch.nn.utils.clip_grad_norm_([params[k] for k in names], 1.0)
        opt.step()
        if step in checkpoints:
            out[step] = (torch.cat([params[k].detach().flatten() for k in names]).clone(), float(nu.detach()), float(want["total"].detach()))
    return out


@pytest.mark.parametrize("path", ["launch_list", "graph"])
def test_inverse_steps_match_the_cpu_reference_path(path, dev):
    """theta at 1e-5 (bar of tests/test_api_gpu.py::test_adam_training_steps_match_cpu_reference_path).  nu: relative 1e-5, or
    4x the CPU path's own sensitivity to a 1e-7 relative perturbation of nu_0 where that is larger (the control
    `bench.py --full` uses for theta): an Adam step divides by sqrt(v) of ONE scalar, so early steps amplify rounding."""
    import oracle as O

    a, sd, obs = _load()
    lr, nu0 = 1e-3, float(a["nu_guess"])
    ps = O.PdeSpec(name="burgers")
    torch.manual_seed(5)
    batches = [O.sample_uniform(ps, 400) for _ in range(10)]
    check = (1, 3, 10)
    ref = _cpu_reference_run(a, sd, obs, batches, nu0, lr, check)
    ctl = _cpu_reference_run(a, sd, obs, batches, nu0 * (1.0 + 1e-7), lr, check)
    cfg, model, pde, tr = _product("inverse", dev, a, sd, obs, lr=lr, fast_step=True)
    assert tr._manual_step_unsupported() is None
    tr._build_flat_state()
    if path == "graph":
        xs, ts = batches[0][0].to(dev).clone(), batches[0][1].to(dev).clone()
        tr._sample = lambda n, xs=xs, ts=ts: (xs, ts)
        theta0 = tr._flat["theta"].clone()
        coef0 = tr._flat["coef"].clone()
        replay, losses = tr.make_graphed_step(400, warmup=1)
        # the warm-up step moved the state: put theta_0, nu_0 and fresh optimiser state back (all in place)
        F = tr._flat
        F["theta"].copy_(theta0)
        F["coef"].copy_(coef0)
        for k in ("m", "v", "step", "coef_m", "coef_v", "coef_step"):
            F[k].zero_()
    for step, (xb, tb) in enumerate(batches, start=1):
        if path == "graph":
            xs.copy_(xb.to(dev))
            ts.copy_(tb.to(dev))
            replay()
        else:
            losses = tr.train_step(xb.to(dev), tb.to(dev))
        if step in check:
            torch.cuda.synchronize()
            want_theta, want_nu, want_total = ref[step]
            e = rel_l2(_theta(model), want_theta)
            got_nu = float(pde.get_parameter("nu").detach())
            e_nu = abs(got_nu - want_nu) / abs(want_nu)
            c_nu = abs(ctl[step][1] - want_nu) / abs(want_nu)
            bar = max(1e-5, 4.0 * c_nu)
            print(f"{path} step {step}: theta rel l2 {e:.2e}; nu {got_nu!r} vs {want_nu!r}: rel {e_nu:.2e}, control {c_nu:.2e}, bar {bar:.2e}; "
                  f"total {float(losses['total'])!r} vs {want_total!r}")
            assert e <= 1e-5, f"theta after {step} steps: {e:.2e}"
            assert e_nu <= bar, f"nu after {step} steps: {e_nu:.2e} (control {c_nu:.2e}, bar {bar:.2e})"
            assert abs(float(losses["total"]) - want_total) <= 5e-5 * abs(want_total), step


def test_graph_replay_equals_the_eager_launch_list(dev):
    a, sd, obs = _load()
    out = []
    for graphed in (False, True):
        cfg, model, pde, tr = _product("inverse", dev, a, sd, obs, lr=2e-3)
        torch.manual_seed(0)
        xb, tb = pde.generate_collocation_points(1000, strategy="uniform")
        tr._sample = lambda n, xb=xb, tb=tb: (xb, tb)
        if graphed:
            replay, losses = tr.make_graphed_step(1000, warmup=1)
            for _ in range(3):
                replay()
            torch.cuda.synchronize()
            assert set(losses) >= {"residual", "boundary", "initial", "data", "total"} and math.isfinite(float(losses["total"]))
        else:
            tr._build_flat_state()
            for _ in range(4):
                tr.train_step(xb, tb)
        nu = pde.get_parameter("nu")  # the live parameter is a view of the coefficient buffer: no rebuild
        assert nu.data_ptr() == tr._flat["coef"].data_ptr()
        out.append((_theta(model), float(nu.detach())))
    (t0, n0), (t1, n1) = out
    print(f"theta rel l2 {rel_l2(t1, t0):.2e}; nu {n1!r} vs {n0!r}")
    assert rel_l2(t1, t0) <= 1e-5
    assert abs(n1 - n0) <= 1e-5 * abs(n0)
    assert n0 != float(a["nu_guess"])


def test_train_takes_the_launch_list_for_inverse_burgers(dev):
    a, sd, obs = _load()
    hists = {}
    for fast in (None, False):
        cfg, model, pde, tr = _product("inverse", dev, a, sd, obs, validation_frequency=5, fast_step=fast)
        torch.manual_seed(0)
        hists[fast] = tr.train(num_epochs=2, batch_size=1000, num_points=4000)
        assert (getattr(tr, "_flat", None) is not None) == (fast is None)
    h = hists[None]
    assert len(h["param_nu"]) == 2 and h["param_nu"][0] != h["param_nu"][1] and all(math.isfinite(v) for v in h["param_nu"])
    assert len(h["data_loss"]) == 2
    for e in range(2):
        ref = hists[False]["train_loss"][e]
        print(f"epoch {e}: train_loss {h['train_loss'][e]!r} vs {ref!r}; nu {h['param_nu'][e]!r} vs {hists[False]['param_nu'][e]!r}")
        assert abs(h["train_loss"][e] - ref) <= 1e-4 * abs(ref)


def test_refusals_name_their_reason_and_train_falls_back(dev):
    from pinnrl_amd import pdes as P
    from pinnrl_amd.rl import RLAgent

    a, sd, obs = _load()
    # pendulum: g and L are trainable, the kernel's coefficient is g / L
    import pinnrl_amd  # noqa: F401
    from pinnrl_amd.config import Config, ModelConfig, TrainingConfig
    from pinnrl_amd.neural_networks import PINNModel
    from pinnrl_amd.training import PDETrainer

    cfg = Config.__new__(Config)
    cfg.device = dev
    cfg.model = ModelConfig(input_dim=2, hidden_dim=32, output_dim=1, num_layers=3, activation="tanh", architecture="feedforward")
    model = PINNModel(cfg, device=dev)
    trc = TrainingConfig(learning_rate=1e-3, gradient_clipping=1.0, mode="inverse")
    cfg.training = trc
    pend = P.PendulumEquation(P.PDEConfig(
        name="pendulum", domain=[(0.0, 1.0)], time_domain=(0.0, 2.0), parameters={"g": 9.81, "L": 1.3},
        boundary_conditions={"dirichlet": {"type": "fixed", "value": 0.0}},
        initial_condition={"type": "small_angle", "initial_angle": 0.5}, exact_solution={}, dimension=1, device=dev, training=trc,
        trainable_parameters=["g", "L"]))
    why = PDETrainer(model, pend, {}, cfg, device=dev)._manual_step_unsupported()
    assert why is not None and "not themselves kernel coefficients" in why

    cfg, model, pde, tr = _product("data_only", dev, a, sd, obs)
    assert tr._manual_step_unsupported() == "data_only mode"
    with pytest.raises(NotImplementedError, match="data_only mode"):
        tr.make_graphed_step(400)
    torch.manual_seed(0)
    hist = tr.train(num_epochs=1, batch_size=500, num_points=1000)  # default fast_step: falls back to the autograd step
    assert getattr(tr, "_flat", None) is None and len(hist["train_loss"]) == 1 and math.isfinite(hist["train_loss"][0])
    cfg, model, pde, tr = _product("data_only", dev, a, sd, obs, fast_step=True)
    with pytest.raises(NotImplementedError, match="data_only mode"):
        tr.train(num_epochs=1, batch_size=500, num_points=1000)

    cfg, model, pde, tr = _product("inverse", dev, a, sd, obs)
    pde.dimension = 2
    assert tr._manual_step_unsupported() == "multi-dimensional problem"
    pde.dimension = 1
    assert tr._manual_step_unsupported() is None
    tr.process_group = object()
    assert "process group" in tr._manual_step_unsupported()
    tr.process_group = None
    cfg.training.collocation_distribution = "residual_based"
    assert "residual-based or RL sampling with trainable coefficients" in tr._manual_step_unsupported()
    cfg.training.collocation_distribution = "uniform"
    tr.rl_agent = RLAgent(state_dim=2, action_dim=1, hidden_dim=16, device=dev)
    assert "residual-based or RL sampling with trainable coefficients" in tr._manual_step_unsupported()
    tr.rl_agent = None
    torch.manual_seed(0)
    cfg.training.collocation_distribution = "residual_based"
    hist = tr.train(num_epochs=1, batch_size=500, num_points=1000)
    assert getattr(tr, "_flat", None) is None and len(hist["param_nu"]) == 1
