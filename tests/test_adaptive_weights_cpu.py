"""CPU tests (no GPU) of adaptive loss weights (RBW / LRW) on the autograd-free step.

(a) the two EMA rules: the reference's recorded numbers (tests/golden/adaptive_weights.npz, written by
    tools/make_adaptive_golden.py) against the fp64 restatement of tests/adaptive_model.py and against the product's
    `_EmaLossWeights`;
(b) routing: `_manual_step_unsupported()` covers rbw / lrw on a 1-D forward problem and names what it does not cover;
(c) the host logic of `_manual_launches_adaptive` under an oracle-backed CPU stand-in for the engine (the pattern of
    tests/test_distributed_cpu.py) against eager steps of the same trainer class;
(d) the new symbol is declared, listed and exported."""

import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, load_case, rel_l2

import adaptive_model as AM
import test_distributed_cpu as tdc

import pinnrl_amd  # noqa: F401
from pinnrl_amd import _lib
from pinnrl_amd import pdes as P
from pinnrl_amd.config import AdaptiveWeightsConfig, Config, TrainingConfig
from pinnrl_amd.training import PDETrainer
from pinnrl_amd.training import trainer as T

STRATEGIES = ("rbw", "lrw")


# ---------------------------------------------------------------------------------------------------------------------
# (a) the rules against the reference's numbers
# ---------------------------------------------------------------------------------------------------------------------
def _fixture_runs():
    z = np.load(os.path.join(GOLDEN, "adaptive_weights.npz"), allow_pickle=False)
    for si, strategy in enumerate(STRATEGIES):
        for ci in range(len(z["alpha"])):
            init = z["initial_weights"][ci]
            init = None if np.isnan(init).any() else [float(v) for v in init]
            for qi in range(z["values"].shape[0]):
                yield strategy, float(z["alpha"][ci]), float(z["eps"][ci]), init, z["values"][qi], z["weights"][si, ci, qi]


def test_fixture_covers_the_cases():
    z = np.load(os.path.join(GOLDEN, "adaptive_weights.npz"), allow_pickle=False)
    assert z["values"].shape == (2, 6, 3) and z["weights"].shape == (2, 3, 2, 6, 3)
    assert (z["values"] > 0).all() and z["values"].min() < 1e-3 and z["values"].max() > 10.0
    assert list(z["alpha"]) == [0.9, 0.7, 0.9] and list(z["eps"]) == [1e-5, 1e-6, 1e-5]
    assert np.isnan(z["initial_weights"][2]).all() and not np.isnan(z["initial_weights"][:2]).any()
    assert len(list(_fixture_runs())) == 12


def test_fp64_restatement_matches_the_reference():
    for strategy, alpha, eps, init, values, want in _fixture_runs():
        rule = AM.EmaWeights(strategy, alpha, eps, init)
        for k in range(values.shape[0]):
            got = rule.update(values[k])
            assert np.abs(got - want[k]).max() <= 1e-6, (strategy, alpha, init, k, got, want[k])


def test_product_rule_matches_the_reference():
    for strategy, alpha, eps, init, values, want in _fixture_runs():
        rule = T._EmaLossWeights(strategy, alpha, eps, init)
        for k in range(values.shape[0]):
            v = torch.from_numpy(values[k].copy())
            got = rule.update(losses=v) if strategy == "rbw" else rule.update(gradients=v)
            assert np.abs(got.numpy().astype(np.float64) - want[k]).max() <= 1e-6, (strategy, alpha, init, k)


# ---------------------------------------------------------------------------------------------------------------------
# (b) routing
# ---------------------------------------------------------------------------------------------------------------------
def _cfg(strategy=None, mode="forward", initial_weights=(0.3, 0.4, 0.3)):
    cfg = Config.__new__(Config)
    cfg.device = torch.device("cpu")
    cfg.training = TrainingConfig(learning_rate=1e-3, gradient_clipping=1.0, mode=mode)
    if strategy is not None:
        cfg.training.adaptive_weights = AdaptiveWeightsConfig(enabled=True, strategy=strategy, alpha=0.7, eps=1e-6,
                                                              initial_weights=list(initial_weights) if initial_weights else None)
        cfg.training.adaptive_weights.initial_weights = list(initial_weights) if initial_weights else None
    return cfg


def _burgers(cfg, trainable=(), obs=None):
    return P.BurgersEquation(P.PDEConfig(
        name="b", domain=[(-1.0, 1.0)], time_domain=(0.0, 1.0), parameters={"nu": 0.01 / math.pi},
        boundary_conditions={"dirichlet": {"type": "fixed", "value": 0.0}},
        initial_condition={"type": "sine", "amplitude": -1.0, "frequency": 1.0}, exact_solution={}, dimension=1,
        device=torch.device("cpu"), training=cfg.training, trainable_parameters=list(trainable),
        parameter_initial_guesses={"nu": 0.02} if trainable else {}, observation_data=obs))


def _routing_trainer(cfg, **pde_kw):
    return PDETrainer(torch.nn.Linear(2, 1), _burgers(cfg, **pde_kw), {}, cfg, device=torch.device("cpu"))


def _obs():
    g = torch.Generator().manual_seed(0)
    return {"x": torch.rand(20, 1, generator=g) * 2 - 1, "t": torch.rand(20, 1, generator=g), "u": torch.rand(20, 1, generator=g)}


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_forward_burgers_with_adaptive_weights_takes_the_launch_list(strategy):
    assert _routing_trainer(_cfg(strategy))._manual_step_unsupported() is None
    assert _routing_trainer(_cfg(strategy, initial_weights=None))._manual_step_unsupported() is None


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_what_stays_on_the_eager_step_is_named(strategy):
    # the same configurations without adaptive weights are covered: the reason is the adaptive weights
    assert _routing_trainer(_cfg(None, mode="inverse"), trainable=["nu"], obs=_obs())._manual_step_unsupported() is None
    assert _routing_trainer(_cfg(None, mode="data_augmented"), obs=_obs())._manual_step_unsupported() is None
    for why in (_routing_trainer(_cfg(strategy, mode="inverse"), trainable=["nu"], obs=_obs())._manual_step_unsupported(),
                _routing_trainer(_cfg(strategy, mode="data_augmented"), obs=_obs())._manual_step_unsupported(),
                _routing_trainer(_cfg(strategy, initial_weights=(0.4, 0.3, 0.2, 0.1)))._manual_step_unsupported()):
        assert isinstance(why, str) and "adaptive loss weights" in why and why != "adaptive loss weights", why
    four = _routing_trainer(_cfg(strategy, initial_weights=(0.4, 0.3, 0.2, 0.1)))._manual_step_unsupported()
    assert "initial weights" in four


def test_other_strategies_and_the_smoothness_component_stay_eager():
    cfg = _cfg("rbw")
    cfg.training.loss_weights["smoothness"] = 0.1
    assert "smoothness" in _routing_trainer(cfg)._manual_step_unsupported()
    cfg = _cfg("rbw")
    cfg.training.adaptive_weights.strategy = "softadapt"
    assert "strategy" in _routing_trainer(cfg)._manual_step_unsupported()


# ---------------------------------------------------------------------------------------------------------------------
# (c) host logic of the adaptive launch list, engine replaced by an oracle-backed CPU stand-in
# ---------------------------------------------------------------------------------------------------------------------
class _AdaptiveEngine(tdc._FakeEngine):
    """`tdc._FakeEngine` + what the adaptive branch calls: `jet_losses` without a residual sum, and `adaptive_adam_step`
    (pinn_adaptive_adam_step) in torch: Gram matrix of the rows, EMA rule on the state, combine + clip + Adam."""

    @staticmethod
    def jet_losses(jets, terms, loss, huber_delta, term_losses, cot, residual_sum=None, residual_scale=0.0, residual_weight=0.0,
                   n_boundary_terms=0, summary4=None):
        rs = residual_sum if residual_sum is not None else torch.zeros(1)
        tdc._FakeEngine.jet_losses(jets, terms, loss, huber_delta, term_losses, cot, rs, residual_scale, residual_weight,
                                   n_boundary_terms, summary4)

    @staticmethod
    def adaptive_adam_step(params, comp_grads, comp_losses, exp_avg, exp_avg_sq, lr, step, scratch, state, strategy="rbw",
                           alpha=0.9, aw_eps=1e-5, initial_weights=None, loss_scales=None, weights_out=None, summary4=None,
                           beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, max_norm=0.0, grad_norm_out=None, grad_out=None):
        n, C = params.numel(), comp_grads.shape[0]
        L = torch.stack([comp_losses[c].reshape(()) * (loss_scales[c] if loss_scales is not None else 1.0) for c in range(C)])
        gram = comp_grads.double() @ comp_grads.double().T
        v = gram.diagonal().sqrt().float() if strategy == "lrw" else L
        if float(state[12]) == 0.0:
            state[0:C] = v
            w = torch.tensor(initial_weights, dtype=torch.float32) if initial_weights is not None else torch.ones(C)
        else:
            state[0:C] = alpha * state[0:C] + (1 - alpha) * v
            if strategy == "lrw":
                inv = 1.0 / (state[0:C] + aw_eps)
                w = inv / inv.sum()
            else:
                w = state[0:C] / (state[0:C].sum() + aw_eps)
                if float(state[13]) != 0.0:
                    w = alpha * state[4 : 4 + C] + (1 - alpha) * w
                state[4 : 4 + C] = w
                state[13] = 1.0
        state[8 : 8 + C] = w
        state[12] += 1.0
        weights_out.zero_()
        weights_out[:C] = w
        summary4[:3] = L[:3]
        summary4[3] = (w * L).sum()
        g = (w[:, None] * comp_grads[:, :n]).sum(0)
        norm = float((w.double() @ gram @ w.double()).clamp_min(0).sqrt())
        if grad_norm_out is not None:
            grad_norm_out[0] = norm
        if max_norm > 0:
            g = g * min(1.0, max_norm / (norm + 1e-6))
        if weight_decay:
            g = g + weight_decay * params
        step += 1
        k = float(step)
        exp_avg.mul_(beta1).add_(g, alpha=1 - beta1)
        exp_avg_sq.mul_(beta2).addcmul_(g, g, value=1 - beta2)
        params -= float(lr) / (1 - beta1**k) * exp_avg / (exp_avg_sq.sqrt() / math.sqrt(1 - beta2**k) + eps)


def _theta(model):
    return torch.cat([p.detach().flatten() for p in model.parameters() if p.requires_grad])


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_launch_list_host_logic_equals_the_eager_step(strategy, monkeypatch):
    spec, pde_s, sd, a, m = load_case("burgers_fourier_3x32")
    _AdaptiveEngine.spec = spec
    monkeypatch.setattr(T, "_E", _AdaptiveEngine)
    torch.manual_seed(11)
    batches = [(torch.from_numpy(a["x"])[i::3][:101].contiguous(), torch.from_numpy(a["t"])[i::3][:101].contiguous()) for i in range(3)]

    eager_model = tdc.OracleModel(spec, sd)
    eager = PDETrainer(eager_model, tdc._pde(), {}, _cfg(strategy), device=torch.device("cpu"), fast_step=False)
    for x, t in batches:
        eager.train_step(x, t)

    model = tdc._ManualOracleModel(spec, sd)
    tr = PDETrainer(model, tdc._pde(), {}, _cfg(strategy), device=torch.device("cpu"))
    assert tr._manual_step_unsupported() is None
    tr._build_flat_state()
    for x, t in batches:
        losses = tr.train_step(x, t)
    assert set(losses) >= {"residual", "boundary", "initial", "total", "weights"} and losses["weights"].shape == (4,)

    e = rel_l2(_theta(model), _theta(eager_model))
    assert e <= 1e-5, f"theta after 3 steps: {e:.2e}"
    want = np.stack(eager.get_training_history()["loss_weights"])
    got = np.stack(tr.get_training_history()["loss_weights"])
    assert got.shape == want.shape == (3, 4) and (got[:, 3] == 0).all()
    assert np.abs(got - want).max() <= 1e-5, (got, want)
    assert np.abs(losses["weights"].numpy() - want[-1]).max() <= 1e-5
    assert not np.allclose(want[0], want[2])  # the rule moved the weights: the comparison is not about constants


def test_eager_state_comes_along_into_the_device_state(monkeypatch):
    """Eager steps first, then the launch list: the EMA state (`running`, `prev_weights`, `weights`) moves into the flat
    state as the Adam moments do, so the next weights equal those of an all-eager run."""
    spec, pde_s, sd, a, m = load_case("burgers_fourier_3x32")
    _AdaptiveEngine.spec = spec
    monkeypatch.setattr(T, "_E", _AdaptiveEngine)
    x, t = torch.from_numpy(a["x"])[:101], torch.from_numpy(a["t"])[:101]
    eager_model = tdc.OracleModel(spec, sd)
    eager = PDETrainer(eager_model, tdc._pde(), {}, _cfg("rbw"), device=torch.device("cpu"), fast_step=False)
    for _ in range(4):
        eager.train_step(x, t)
    model = tdc._ManualOracleModel(spec, sd)
    tr = PDETrainer(model, tdc._pde(), {}, _cfg("rbw"), device=torch.device("cpu"))
    for _ in range(3):
        tr.train_step(x, t)  # eager: no flat state yet
    tr._build_flat_state()
    s = tr._flat["aw_state"]
    assert float(s[12]) != 0.0 and float(s[13]) == 1.0
    tr.train_step(x, t)
    want = np.stack(eager.get_training_history()["loss_weights"])
    got = np.stack(tr.get_training_history()["loss_weights"])
    assert got.shape == (4, 4) and np.abs(got - want).max() <= 1e-5
    assert rel_l2(_theta(model), _theta(eager_model)) <= 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# (d) exports
# ---------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_listed_and_exported():
    with open(os.path.join(ROOT, "include", "pinn_jet.h")) as f:
        header = f.read()
    assert "int pinn_adaptive_adam_step(" in header
    assert f"#define PINN_ADAPTIVE_SCRATCH_FLOATS {_lib.PINN_ADAPTIVE_SCRATCH_FLOATS}" in header
    assert "pinn_adaptive_adam_step" in _lib.EXPORTS
    lib = _lib.load()
    assert lib.pinn_adaptive_adam_step is not None and lib.pinn_adaptive_adam_step.argtypes is not None
    assert _lib.PINN_ABI_VERSION == 2 and lib.pinn_abi_version() == 2  # an additive change
